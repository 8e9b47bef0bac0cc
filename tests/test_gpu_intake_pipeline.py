"""The two-slot intake (csrc/prover_intake.h: stage, staged, advance; batch.py: stage_*, advance, prove_inputs_stream) on an MI355X:
a batch staged on the copy stream while the resident one proves, against a fresh prover's prove_inputs and the oracle."""
import pytest

import intake_pipeline_cases as ic

pytestmark = pytest.mark.gpu

GPU_BATCHES = ic.BATCHES + (65,)  # one lane past a 64-lane workgroup of the one-lane solver


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(ic.PTAU)


@pytest.fixture(scope="module")
def shared():
    """What the cases of this module build once: the circuits, the fresh provers' references, the oracle's proof."""
    return {}


@pytest.mark.parametrize("mode", ["inputs", "input_values", "values"])
@pytest.mark.parametrize("name", ["chain32", "chain128"])
def test_bytes_chain(setup, shared, name, mode):
    ic.bytes_through_the_pipeline(setup, shared, name, mode, sizes=GPU_BATCHES, oracle=name == "chain32")


@pytest.mark.parametrize("mode", ["input_values", "values"])
@pytest.mark.parametrize("name", ["wide-lanes", "wide-levels"])
def test_bytes_wide(setup, shared, name, mode):
    ic.bytes_through_the_pipeline(setup, shared, name, mode, sizes=GPU_BATCHES)


@pytest.mark.parametrize("name", ["chain32", "chain128", "wide-levels"])
def test_stream(setup, shared, name):
    ic.stream_yields_the_same_bytes(setup, shared, name, sizes=GPU_BATCHES)


def test_failing_batch_then_clean(setup):
    ic.failing_batch_then_clean(setup)


def test_clean_batch_then_failing(setup):
    ic.clean_batch_then_failing(setup)


def test_staged_value_not_below_r(setup):
    ic.staged_value_not_below_r(setup)


def test_status_stride_stays_with_its_batch(setup):
    ic.status_stride_stays_with_its_batch(setup)


@pytest.mark.parametrize("name,mode", [("chain32", "inputs"), ("chain32", "values"), ("wide-lanes", "input_values"), ("wide-levels", "input_values")])
def test_reads_go_to_the_resident_batch(setup, shared, name, mode):
    ic.reads_go_to_the_resident_batch(setup, shared, name, mode)


def test_state_errors(setup, shared):
    ic.state_errors(setup, shared)


@pytest.mark.parametrize("name,mode", [("chain32", "inputs"), ("chain32", "values"), ("wide-levels", "input_values")])
def test_sizes_change_under_it(setup, shared, name, mode):
    ic.sizes_change_under_it(setup, shared, name, mode)
