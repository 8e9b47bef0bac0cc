"""The comb MSM's edge cases (tests/msm_comb_edge_cases.py) on the emulated kernels, whose lazy-limb operations assert their
operand ranges (csrc/fpl.h, PLONK_EMU)."""
import pytest

import msm_comb_edge_cases as mc


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_special_scalars(emu, h, top):
    mc.special_scalars(h, top)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_cancelling_pairs(emu, h, top):
    mc.cancelling_pairs(h, top)


@pytest.mark.parametrize("h,top", mc.TABLES)
def test_identity_bases(emu, h, top):
    mc.identity_bases(h, top)


@pytest.mark.parametrize("h,top", [(7, True), (5, False)])
def test_batch_of_three(emu, h, top):
    from plonkathon_amd import Setup

    mc.batch_of_three(Setup.from_file(mc.PTAU), h, top, sizes=(13,))


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_special_scalars_wide_index(emu, h, top):
    mc.special_scalars(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_cancelling_pairs_wide_index(emu, h, top):
    mc.cancelling_pairs(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_identity_bases_wide_index(emu, h, top):
    mc.identity_bases(h, top, wide=True)


@pytest.mark.parametrize("h,top", mc.WIDE_TABLES)
def test_batch_of_three_wide_index(emu, h, top):
    from plonkathon_amd import Setup

    mc.batch_of_three(Setup.from_file(mc.PTAU), h, top, sizes=(13,), wide=True)


def test_wide_flag_arguments(emu):
    mc.wide_flag_arguments()
