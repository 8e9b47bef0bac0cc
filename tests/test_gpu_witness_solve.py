"""The witness solver (csrc/witness_solve.h) on an MI355X: a batch proved from the circuit's input values alone, against the
oracle's fill_variable_assignments and the committed fixtures."""
import pytest

import witness_solve_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(wc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once (wc.poseidon_prover)."""
    return {}


def test_solved_values_class_circuit(setup):
    wc.solved_values_class(setup)


def test_solved_values_factorisation(setup):
    wc.solved_values_factorisation(setup)


def test_solved_values_chain(setup):
    wc.solved_values_chain(setup, 32, 5)


@pytest.mark.parametrize("with_hash", [False, True])
def test_solved_values_poseidon(setup, shared, with_hash):
    wc.solved_values_poseidon(setup, shared, with_hash)


def test_empty_cells_at_the_end_of_the_buffer(setup):
    wc.empty_cells_at_the_end_of_the_buffer(setup)


def test_proof_bytes_equal_filled_witnesses(setup):
    wc.proof_bytes_equal_filled_witnesses(setup, 128, 2)


@pytest.mark.parametrize("name", ["chain_512_x0_3", "chain_2048_x0_3", "chain_2048_x0_4", "poseidon_1024"])
def test_prove_inputs_matches_fixture(setup, name):
    wc.prove_inputs_matches_fixture(setup, name)


def test_failing_assertion(setup, shared):
    wc.failing_assertion(setup, shared)


def test_plan_refusals(setup):
    wc.plan_refusals(setup)


def test_non_canonical_inputs(setup):
    wc.non_canonical_inputs(setup)


def test_existing_uploads_unchanged(setup):
    wc.existing_uploads_unchanged(setup)


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_lane_geometry(setup, B):
    """A lone lane, a full wave, a partial second workgroup, a partial third."""
    wc.lane_geometry(setup, B)


def test_two_async_batches_back_to_back(setup):
    wc.two_async_batches_back_to_back(setup)


def test_public_values_feed_the_verifier(setup, shared):
    wc.public_values_feed_the_verifier(setup, shared)


def test_batch_sizes_change_between_uploads(setup):
    wc.batch_sizes_change_between_uploads(setup)
