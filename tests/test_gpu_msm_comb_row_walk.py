"""The comb MSM's row walk (tests/msm_comb_row_walk_cases.py) on an MI355X: tiny forced combs with the row walk forced, and the
library's rule on the table it builds for the SRS by default."""
import pytest

import msm_comb_row_walk_cases as rw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("chunks", rw.CHUNKS)
@pytest.mark.parametrize("h,top", rw.COMBS)
def test_edge_cases(h, top, chunks):
    rw.edge_cases(h, top, chunks)


@pytest.mark.parametrize("h,top,M", [(7, True, 9), (8, False, 8)])
def test_rows_not_a_multiple_of_256_both_forms_equal(h, top, M):
    rw.both_forms(h, top, M)


@pytest.mark.parametrize("short", [0, 5])
@pytest.mark.parametrize("n,chunks", rw.VIRTUAL_CASES)
def test_chunk_boundaries_at_the_virtual_scalars(n, chunks, short):
    rw.virtual_chunks(n, chunks, short)


@pytest.mark.parametrize("chunks", [4, 5])
def test_redo_path_item_major(chunks):
    rw.redo_path(chunks)


def test_flag_arguments():
    rw.flag_arguments()


def test_rule_takes_the_row_walk_for_a_batch():
    from plonkathon_amd import Setup

    rw.rule_on_default_table(Setup.from_file(rw.PTAU))
