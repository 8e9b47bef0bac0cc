"""The witness solver's levelised form (csrc/witness_solve.h: witness_solve_levels_kernel, the plan's levels, the rule and the
option that choose a form) on the emulated kernels, against the oracle's fill_variable_assignments."""
import os
import subprocess

import pytest

import witness_levels_cases as lc


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(lc.wc.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once (lc.braid_prover, lc.poseidon_levels_prover)."""
    return {}


@pytest.mark.parametrize("W", [255, 256, 300])
def test_level_width_against_T(emu, setup, shared, W):
    lc.level_width_against_T(setup, shared, W)


def test_every_selector_class(emu, setup):
    lc.every_selector_class(setup)


def test_width_one(emu, setup):
    lc.width_one(setup)


@pytest.mark.parametrize("form", ["levels", "lanes"])
@pytest.mark.parametrize("with_hash", [False, True])
def test_poseidon_values(emu, setup, shared, with_hash, form):
    lc.poseidon_values(setup, shared, with_hash, form)


@pytest.mark.parametrize("form", ["levels", "lanes"])
def test_poseidon_failing_assertion(emu, setup, shared, form):
    lc.poseidon_failing_assertion(setup, shared, form)


def test_first_failure_in_program_order(emu, setup):
    lc.first_failure_in_program_order(setup)


def test_plan_query(emu, setup, shared):
    lc.plan_query(setup, shared)


def test_plan_query_poseidon_multi(emu, setup):
    lc.plan_query_poseidon_multi(setup)


def test_options(emu, setup):
    lc.options(setup)


def test_levels_lifetime_program(emu_cdll, tmp_path):
    """tests/emu/levels_lifetime.cpp — the stand-alone program of `make -C tests/emu -f levels_sanitize.mk levels-sanitize` — built plain against the
    emulator library and run: a plan, a second plan with other inputs, a new wiring, uploads under both forms, a prover destroyed
    with a plan and no upload."""
    emu_dir = os.path.dirname(os.path.abspath(emu_cdll._name))
    repo = os.path.dirname(os.path.dirname(emu_dir))
    exe = str(tmp_path / "levels_lifetime")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(repo, "include"), os.path.join(emu_dir, "levels_lifetime.cpp"), "-o", exe,
                    emu_cdll._name, "-Wl,-rpath," + emu_dir], check=True, timeout=120)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "levels_lifetime ok", (done.returncode, done.stdout, done.stderr)
