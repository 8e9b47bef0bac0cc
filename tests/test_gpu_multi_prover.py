"""GPU suite: the lock-step prover over a table of circuits on the MI355X.  Cases: multi_prover_cases.py.  Group orders: 8 (a proof
is smaller than a wave), 64 (the quotient kernel's Z_H is uniform per wave), 512 (a proof spans several 256-lane blocks of the
quotient and linearisation kernels and several rows per lane in the scans), and one batch at the benchmark's 2048."""
import pytest

import multi_prover_cases as mp
import parity_cases as pc

pytestmark = pytest.mark.gpu

_built = {}


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


@pytest.fixture
def fam(setup, request):
    """one Family per group order, built by the first test that asks: by then the device library is the bound one"""
    n = request.param
    if n not in _built:
        _built[n] = mp.Family(setup, n)
    return _built[n]


sizes = pytest.mark.parametrize("fam", [8, 64, 512], indirect=True)
at = lambda *ns: pytest.mark.parametrize("fam", list(ns), indirect=True)


@sizes
def test_bytes_by_every_route(fam):
    mp.bytes_by_every_route(fam, routes=("upload", "values", "raw", "async"))


def test_bytes_at_the_benchmark_order(setup):
    mp.mixed_batch_at_2048(setup)


@at(64)
def test_pinned_to_the_oracle(fam):
    mp.oracle_pin(fam)


@sizes
def test_a_table_of_one_circuit_is_the_batch_prover(fam):
    mp.table_of_one(fam)


@pytest.mark.parametrize("fam,segments", [(64, 2), (64, 4), (512, 8)], indirect=["fam"])
def test_forced_segments(fam, segments):
    mp.bytes_by_every_route(fam, routes=("upload",), segments=segments)


@at(64)
def test_lagrange_commits(fam):
    mp.bytes_by_every_route(fam, routes=("upload",), lagrange_commits=True)


@at(8, 64)
def test_blinded_with_explicit_rows(fam):
    mp.blinded_with_explicit_rows(fam)


@at(8)
def test_blinded_with_a_seed(fam):
    mp.blinded_with_a_seed(fam)


@sizes
def test_statuses_are_per_proof(fam):
    mp.statuses_are_per_proof(fam)


@at(64)
def test_batches_in_sequence(fam):
    mp.batches_in_sequence(fam)


@at(8)
def test_refusals(fam):
    mp.refusals(fam)


@at(8, 64)
def test_the_verifier_loads_the_resident_batch(fam):
    mp.verifier_loads_the_resident_batch(fam)
