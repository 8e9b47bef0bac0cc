"""The two-slot intake (csrc/prover_intake.h: stage, staged, advance; batch.py: stage_*, advance, prove_inputs_stream) on the
emulated kernels: a batch staged beside the resident one, against a fresh prover's prove_inputs and the oracle."""
import os
import subprocess

import pytest

import intake_pipeline_cases as ic


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(ic.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once: the circuits, the fresh provers' references, the oracle's proof."""
    return {}


# A proof costs about a second on the emulated kernels at 2^7 and several at 2^10: here the full list of batches runs at 2^5 through every
# entry point, at 2^7 through one, and the wide circuit proves batches of 2 and 1 under each form (its batch of 5 is read back, not
# proved: test_reads_go_to_the_resident_batch).  tests/test_gpu_intake_pipeline.py runs every combination with the full list.
@pytest.mark.parametrize("name,mode", [("chain32", "inputs"), ("chain32", "input_values"), ("chain32", "values"), ("chain128", "input_values")])
def test_bytes_chain(emu, setup, shared, name, mode):
    ic.bytes_through_the_pipeline(setup, shared, name, mode, oracle=name == "chain32")


@pytest.mark.parametrize("name", ["wide-lanes", "wide-levels"])
def test_bytes_wide(emu, setup, shared, name):
    ic.bytes_through_the_pipeline(setup, shared, name, "input_values", sizes=(2, 1))


def test_stream(emu, setup, shared):
    ic.stream_yields_the_same_bytes(setup, shared, "chain32")


def test_failing_batch_then_clean(emu, setup):
    ic.failing_batch_then_clean(setup)


def test_clean_batch_then_failing(emu, setup):
    ic.clean_batch_then_failing(setup)


def test_staged_value_not_below_r(emu, setup):
    ic.staged_value_not_below_r(setup)


def test_status_stride_stays_with_its_batch(emu, setup):
    ic.status_stride_stays_with_its_batch(setup)


@pytest.mark.parametrize("name,mode", [("chain32", "inputs"), ("chain32", "values"), ("wide-lanes", "input_values"), ("wide-levels", "input_values")])
def test_reads_go_to_the_resident_batch(emu, setup, shared, name, mode):
    ic.reads_go_to_the_resident_batch(setup, shared, name, mode)


def test_state_errors(emu, setup, shared):
    ic.state_errors(setup, shared)


@pytest.mark.parametrize("mode", ["inputs", "values"])
def test_sizes_change_under_it(emu, setup, shared, mode):
    ic.sizes_change_under_it(setup, shared, "chain32", mode)


def test_pipeline_lifetime_program(emu_cdll, tmp_path):
    """tests/emu/pipeline_lifetime.cpp — the stand-alone program of `make -C tests/emu -f pipeline_sanitize.mk pipeline-sanitize` — built
    plain against the emulator library and run: stage, advance, a larger batch staged, a new plan with nothing staged, a prover
    destroyed with a batch staged."""
    emu_dir = os.path.dirname(os.path.abspath(emu_cdll._name))
    repo = os.path.dirname(os.path.dirname(emu_dir))
    exe = str(tmp_path / "pipeline_lifetime")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(repo, "include"), os.path.join(emu_dir, "pipeline_lifetime.cpp"), "-o", exe,
                    emu_cdll._name, "-Wl,-rpath," + emu_dir], check=True, timeout=120)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "pipeline_lifetime ok", (done.returncode, done.stdout, done.stderr)
