"""The comb MSM's recovery list and the fixed grid of its recovery kernel (tests/msm_comb_recovery_grid_cases.py) on an MI355X:
n = 300 on the 9-tooth comb and on the 11-tooth comb with top tables."""
import pytest

import msm_comb_recovery_grid_cases as rg

pytestmark = pytest.mark.gpu
combs = pytest.mark.parametrize("comb", rg.COMBS, ids=rg.comb_id)
forms = pytest.mark.parametrize("form", rg.FORMS, ids=["row walk, 2 chunks", "column lanes, 4 workgroups"])


@combs
@forms
def test_rows_0_17_39_of_40_flagged(comb, form):
    rg.flagged_batch(comb, form)


@combs
@forms
def test_nothing_flagged_counter_reads_zero(comb, form):
    rg.nothing_flagged(comb, form)


@combs
def test_deferred_list_overflow(comb):
    rg.overflow(comb, "rows", 1)


@combs
def test_17_of_17_flagged_more_than_workgroups(comb):
    rg.all_flagged(comb, rg.FORMS[0])


@combs
def test_counter_does_not_carry_over(comb):
    rg.two_calls(comb, rg.FORMS[0])


@pytest.mark.parametrize("m", rg.OTHER_METHODS, ids=rg.ks.method_id)
def test_bucket_and_window_paths_17_overflow_then_none(m):
    rg.other_methods(m)
