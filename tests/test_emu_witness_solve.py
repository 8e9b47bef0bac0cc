"""The witness solver (csrc/witness_solve.h) on the emulated kernels: the plan, the solver's kernels and the Python layer above
them, against the oracle's fill_variable_assignments and the committed fixtures."""
import pytest

import witness_solve_cases as wc


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(wc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once (wc.poseidon_prover)."""
    return {}


def test_solved_values_class_circuit(emu, setup):
    wc.solved_values_class(setup)


def test_solved_values_factorisation(emu, setup):
    wc.solved_values_factorisation(setup)


def test_solved_values_chain(emu, setup):
    wc.solved_values_chain(setup, 32, 5)


@pytest.mark.parametrize("with_hash", [False, True])
def test_solved_values_poseidon(emu, setup, shared, with_hash):
    wc.solved_values_poseidon(setup, shared, with_hash)


def test_empty_cells_at_the_end_of_the_buffer(emu, setup):
    wc.empty_cells_at_the_end_of_the_buffer(setup)


def test_proof_bytes_equal_filled_witnesses(emu, setup):
    wc.proof_bytes_equal_filled_witnesses(setup, 128, 2)


def test_prove_inputs_matches_fixture(emu, setup):
    wc.prove_inputs_matches_fixture(setup, "chain_512_x0_3")


def test_failing_assertion(emu, setup, shared):
    wc.failing_assertion(setup, shared)


def test_plan_refusals(emu, setup):
    wc.plan_refusals(setup)


def test_non_canonical_inputs(emu, setup):
    wc.non_canonical_inputs(setup)


def test_existing_uploads_unchanged(emu, setup):
    wc.existing_uploads_unchanged(setup)
