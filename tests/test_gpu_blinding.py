"""Zero-knowledge blinding of the lock-step prover (csrc/prover_blind.h; BatchProver(blinding=...)) on an MI355X: the cases of
tests/blinding_cases.py against its CPU model at group orders 8 and 16, acceptance and the closed forms at 2^10, the segmented
scans at 2^13."""
import pytest

import blinding_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(bc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once: the circuits, the model and its proofs."""
    return {}


@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_zero_blinders_are_unblinded_bytes(setup, shared, name):
    bc.zero_blinders_are_unblinded_bytes(setup, shared, name)


@pytest.mark.parametrize("lagrange_commits", [False, True])
@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_bit_exact_against_the_model(setup, shared, name, lagrange_commits):
    bc.bit_exact_against_the_model(setup, shared, name, lagrange_commits)


@pytest.mark.parametrize("name", ["golden", "factorisation"])
def test_seeded_against_the_model(setup, shared, name):
    bc.seeded_against_the_model(setup, shared, name)


def test_accepted_and_hidden_chain_1024(setup):
    """2^10 is the largest group order the golden .ptau allows with n + 6 <= 2048 powers."""
    bc.accepted_and_hidden_at_size(setup, bc.chain_lines(1024), 1024, [{"x0": 3 + 1000003 * i} for i in range(4)])


def test_accepted_and_hidden_poseidon_1024(setup):
    from witness_solve_cases import poseidon_program, poseidon_starts

    bc.accepted_and_hidden_at_size(setup, poseidon_program()[0], 1024, poseidon_starts(4))


def test_segmented_scans_same_bytes():
    """n = 2^13 on a from-tau SRS of 2^13 + 6 powers, B = 1: one workgroup per proof and S = 32 give the same bytes, and the proof
    verifies."""
    from large_prover_cases import device_tau_setup

    n = 1 << 13
    tau = device_tau_setup(n + 6)

    def verifies(program, wits, proofs):
        vk = tau.verification_key(program.common_preprocessed_input())
        assert vk.verify_proof(n, proofs[0], [wits[0]["x0"]])

    bc.segmented_scans_same_bytes(tau, n, (1, 32), verifies)


def test_refusals(setup, shared):
    bc.refusals(setup, shared)


def test_failure_bits_survive(setup, shared):
    bc.failure_bits_survive(setup, shared)


def test_stream_equals_unpipelined(setup, shared):
    """(65: one lane past the 64-lane workgroups of the per-proof corrections)"""
    bc.stream_equals_unpipelined(setup, shared, sizes=(2, 65, 1))
