"""The comb MSM's row walk (tests/msm_comb_row_walk_cases.py) on the emulated kernels, whose lazy-limb operations assert their
operand ranges (csrc/fpl.h, PLONK_EMU): the smaller half of each list of the GPU file."""
import pytest

import msm_comb_row_walk_cases as rw


@pytest.mark.parametrize("chunks", rw.EMU_CHUNKS)
@pytest.mark.parametrize("h,top", rw.EMU_COMBS)
def test_edge_cases(emu, h, top, chunks):
    rw.edge_cases(h, top, chunks, sizes=rw.EMU_SIZES)


@pytest.mark.parametrize("h,top,M", [(7, True, 9), (8, False, 8)])
def test_rows_not_a_multiple_of_256_both_forms_equal(emu, h, top, M):
    """R = 324 and R = 256 exactly, as on the GPU, with fewer scalars.  (8, plain) has 32 columns: the one comb here whose item-major
    digits leave as 16-byte stores; identity bases through it as well."""
    rw.both_forms(h, top, M, n=13)
    if not top:
        rw.edge_cases(h, top, 2, sizes=rw.EMU_SIZES)


@pytest.mark.parametrize("n,chunks", rw.VIRTUAL_CASES[:2])
def test_chunk_boundaries_at_the_virtual_scalars(emu, n, chunks):
    rw.virtual_chunks(n, chunks, short=5 if chunks == 10 else 0)


def test_redo_path_item_major(emu):
    rw.redo_path(4)


def test_flag_arguments(emu):
    rw.flag_arguments()
