"""The comb MSM's edge cases (tests/msm_comb_edge_cases.py) on an MI355X: tiny forced combs, and the table the library builds
for the SRS by default."""
import pytest

import msm_comb_edge_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(mc.PTAU)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_special_scalars(h, top):
    mc.special_scalars(h, top)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_cancelling_pairs(h, top):
    mc.cancelling_pairs(h, top)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_identity_bases(h, top):
    mc.identity_bases(h, top)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_batch_of_three(setup, h, top):
    mc.batch_of_three(setup, h, top)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_special_scalars_wide_index(h, top):
    mc.special_scalars(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_cancelling_pairs_wide_index(h, top):
    mc.cancelling_pairs(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_identity_bases_wide_index(h, top):
    mc.identity_bases(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_batch_of_three_wide_index(setup, h, top):
    mc.batch_of_three(setup, h, top, wide=True)


def test_wide_flag_arguments():
    mc.wide_flag_arguments()


def test_default_table(setup):
    mc.default_table(setup)
    mc.batch_of_three(setup)
