"""The segmented per-proof scans of the lock-step prover (csrc/prover_scans.h) on the emulated kernels: the new lazy-limb code of the
segmented evaluation runs under fpl.h's range assertions here, and a forced S must give the bytes of S = 1."""
import pytest

import large_prover_cases as lc


@pytest.mark.parametrize("n,S", [(128, 2), (128, 8), (512, 8)])
def test_forced_segments_equal_one_workgroup(emu, n, S):
    """Two witnesses: S = 1 against forced S, proof 0 against the live oracle (2^7) or the committed fixture (2^9)."""
    from plonkathon_amd import Setup

    lc.forced_segments_equal_one_workgroup(Setup.from_file(lc.PTAU), n, S, B=2)


@pytest.mark.parametrize("log_n", [5, 8, 10])
def test_grand_product_one_workgroup_vs_integers(emu, log_n):
    """S = 1: fewer rows than lanes (idle lanes carry the neutral element), one row per lane, four rows per lane."""
    assert lc.plan_segments(log_n, 1) == 1
    assert lc.grand_product_vs_integers(log_n) == 1


def test_segment_options_are_checked(emu):
    """PLONK_PROVER_SEGMENTS_LOG2: segments of fewer than 16 rows, S = 512 and a stray option bit are PLONK_ERR_ARG."""
    from plonkathon_amd import Setup

    lc.segment_option_refusals(Setup.from_file(lc.PTAU))


def test_plan_leaves_the_benchmarked_shapes_alone(emu):
    lc.plan_is_one_for_benchmarked_shapes()
