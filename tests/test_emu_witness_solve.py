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


def test_batch_sizes_change_between_uploads(emu, setup):
    wc.batch_sizes_change_between_uploads(setup)


def test_intake_lifetime_program(emu_cdll, tmp_path):
    """tests/emu/intake_lifetime.cpp — the stand-alone program of `make -C tests/emu intake-sanitize` — built plain against the
    emulator library and run: batches of 2, 5 and 1 through every kind of upload, two plans, a prover destroyed without an upload.
    The emulator's events are heap objects, so an event destroyed twice or never created ends the program."""
    import os
    import subprocess

    emu_dir = os.path.dirname(os.path.abspath(emu_cdll._name))
    repo = os.path.dirname(os.path.dirname(emu_dir))
    exe = str(tmp_path / "intake_lifetime")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(repo, "include"), os.path.join(emu_dir, "intake_lifetime.cpp"), "-o", exe,
                    emu_cdll._name, "-Wl,-rpath," + emu_dir], check=True, timeout=120)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "intake_lifetime ok", (done.returncode, done.stdout, done.stderr)
