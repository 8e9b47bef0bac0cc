"""Round 4's evaluations in passes, with the sums reduced inside the waves (csrc/prover_scans.h), on an MI355X: the group orders
of the emulator suite and 2^11, the benchmarked order (eight rows per lane).  Bodies and shapes: tests/eval_passes_cases.py."""
import pytest

import eval_passes_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared():
    return {}


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(ec.pc.PTAU)


@pytest.mark.parametrize("n,S", ec.cases(ec.GPU_ORDERS))
def test_chain_batch(setup, shared, n, S):
    ec.chain_batch(setup, shared, n, S)


def test_segments_refused_at_16(setup, shared):
    ec.segments_refused_at_16(setup, shared)


@pytest.mark.parametrize("S", [1, 4])
def test_two_circuits(setup, shared, S):
    ec.two_circuits(setup, shared, S)


@pytest.mark.parametrize("S", [1, 4])
def test_blinded(setup, shared, S):
    ec.blinded(setup, shared, S)


def test_gate_failure_does_not_stick(setup):
    ec.gate_failure_does_not_stick(setup)

