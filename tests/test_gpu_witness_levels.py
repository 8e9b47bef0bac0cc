"""The witness solver's levelised form (csrc/witness_solve.h: witness_solve_levels_kernel, one workgroup per proof) on an MI355X,
against the oracle's fill_variable_assignments and poseidon_hash."""
import pytest

import witness_levels_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(lc.wc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once (lc.braid_prover, lc.poseidon_levels_prover)."""
    return {}


@pytest.mark.parametrize("W", [255, 256, 300])
def test_level_width_against_T(setup, shared, W):
    lc.level_width_against_T(setup, shared, W)


def test_every_selector_class(setup):
    lc.every_selector_class(setup)


def test_width_one(setup):
    lc.width_one(setup)


@pytest.mark.parametrize("form", ["levels", "lanes"])
@pytest.mark.parametrize("with_hash", [False, True])
def test_poseidon_values(setup, shared, with_hash, form):
    lc.poseidon_values(setup, shared, with_hash, form)


@pytest.mark.parametrize("form", ["levels", "lanes"])
def test_poseidon_failing_assertion(setup, shared, form):
    lc.poseidon_failing_assertion(setup, shared, form)


def test_first_failure_in_program_order(setup):
    lc.first_failure_in_program_order(setup)


def test_plan_query(setup, shared):
    lc.plan_query(setup, shared)


def test_plan_query_poseidon_multi(setup):
    lc.plan_query_poseidon_multi(setup)


def test_options(setup):
    lc.options(setup)


def test_proof_bytes(setup):
    lc.proof_bytes(setup)


def test_two_async_batches_back_to_back(setup, shared):
    lc.two_async_batches_back_to_back(setup, shared)


@pytest.mark.parametrize("B", [1, 2, 65])
def test_grid_geometry(setup, shared, B):
    """A lone workgroup, two, and more workgroups than one launch wave of a CU row holds side by side."""
    lc.grid_geometry(setup, shared, B)


def test_above_2_11():
    from large_prover_cases import device_tau_setup

    lc.above_2_11(device_tau_setup(8192))
