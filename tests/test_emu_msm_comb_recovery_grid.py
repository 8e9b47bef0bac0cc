"""The comb MSM's recovery list and the fixed grid of its recovery kernel (tests/msm_comb_recovery_grid_cases.py) on the emulated
kernels: n = 300 on the 9-tooth comb and on the 11-tooth comb with top tables."""
import pytest

import msm_comb_recovery_grid_cases as rg

combs = pytest.mark.parametrize("comb", rg.COMBS, ids=rg.comb_id)
forms = pytest.mark.parametrize("form", rg.FORMS, ids=["row walk, 2 chunks", "column lanes, 4 workgroups"])


@combs
@forms
def test_rows_0_17_39_of_40_flagged(emu, comb, form):
    rg.flagged_batch(comb, form)


@combs
def test_nothing_flagged_counter_reads_zero(emu, comb):
    """(through the row walk: the emulated column-lane kernel takes twenty seconds per batch of 40, and the flagged batch above has
    37 unflagged rows in it; the GPU suite runs both forms)"""
    rg.nothing_flagged(comb, rg.FORMS[0])


@combs
def test_deferred_list_overflow(emu, comb):
    rg.overflow(comb, "rows", 1)


@combs
def test_17_of_17_flagged_more_than_workgroups(emu, comb):
    rg.all_flagged(comb, rg.FORMS[0])


@combs
def test_counter_does_not_carry_over(emu, comb):
    rg.two_calls(comb, rg.FORMS[0])


@pytest.mark.parametrize("m", rg.EMU_OTHER_METHODS, ids=rg.ks.method_id)
def test_bucket_and_window_paths_17_overflow_then_none(emu, m):
    rg.other_methods(m)


@combs
def test_nothing_flagged_column_lanes_small_batch(emu, comb):
    """The column-lane kernel's route into finalize with an empty list, at 6 MSMs (the batch of 40 takes the emulator twenty seconds)."""
    rg.nothing_flagged(comb, rg.FORMS[1], M=6)
