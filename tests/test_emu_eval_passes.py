"""Round 4's evaluations in passes, with the sums reduced inside the waves (csrc/prover_scans.h), on the emulated kernels: the
lazy-limb chains run under fpl.h's range assertions here.  Bodies and shapes: tests/eval_passes_cases.py."""
import pytest

import eval_passes_cases as ec


@pytest.fixture(scope="module")
def shared():
    return {}


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(ec.pc.PTAU)


@pytest.mark.parametrize("n,S", ec.cases(ec.EMU_ORDERS))
def test_chain_batch(emu, setup, shared, n, S):
    ec.chain_batch(setup, shared, n, S)


def test_segments_refused_at_16(emu, setup, shared):
    ec.segments_refused_at_16(setup, shared)


@pytest.mark.parametrize("S", [1, 4])
def test_two_circuits(emu, setup, shared, S):
    ec.two_circuits(setup, shared, S)


@pytest.mark.parametrize("S", [1, 4])
def test_blinded(emu, setup, shared, S):
    ec.blinded(setup, shared, S)


def test_gate_failure_does_not_stick(emu, setup):
    ec.gate_failure_does_not_stick(setup)
