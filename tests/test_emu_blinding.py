"""Zero-knowledge blinding of the lock-step prover (csrc/prover_blind.h; BatchProver(blinding=...)) on the emulated kernels: group
orders 8 and 16, batches of at most four, against the CPU model of tests/blinding_cases.py."""
import pytest

import blinding_cases as bc


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(bc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once: the circuits, the model and its proofs."""
    return {}


@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_model_is_the_oracle(shared, name):
    bc.model_is_the_oracle(shared, name)


@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_zero_blinders_are_unblinded_bytes(emu, setup, shared, name):
    bc.zero_blinders_are_unblinded_bytes(setup, shared, name)


@pytest.mark.parametrize("lagrange_commits", [False, True])
@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_bit_exact_against_the_model(emu, setup, shared, name, lagrange_commits):
    bc.bit_exact_against_the_model(setup, shared, name, lagrange_commits)


def test_seeded_against_the_model(emu, setup, shared):
    bc.seeded_against_the_model(setup, shared, "golden")


def test_segmented_scans_same_bytes(emu, setup):
    """n = 16: one workgroup per proof against the largest S set_options allows there (segments of 16 rows: S = 1 is all there is
    at 16 rows, so the segmented kernels run at n = 32 with S = 2)."""
    bc.segmented_scans_same_bytes(setup, 16, (1,))
    bc.segmented_scans_same_bytes(setup, 32, (1, 2), B=2)


def test_refusals(emu, setup, shared):
    bc.refusals(setup, shared)


def test_failure_bits_survive(emu, setup, shared):
    bc.failure_bits_survive(setup, shared)


def test_stream_equals_unpipelined(emu, setup, shared):
    bc.stream_equals_unpipelined(setup, shared)
