"""CPU suite: the lock-step prover over a table of circuits on the emulated kernels, where the lazy-limb bounds (FPL_CHECK) are
asserted on every operand (group_order 8 and 16, batches of at most 7).  Cases: multi_prover_cases.py."""
import pytest

import multi_prover_cases as mp
import parity_cases as pc

_built = {}


@pytest.fixture
def fam(emu, request):
    """one Family per group order, built by the first test that asks: by then the emulated library is the bound one"""
    from plonkathon_amd import Setup

    n = request.param
    if n not in _built:
        _built.setdefault("setup", Setup.from_file(pc.PTAU))
        _built[n] = mp.Family(_built["setup"], n)
    return _built[n]


sizes = pytest.mark.parametrize("fam", [8, 16], indirect=True)
at_16 = pytest.mark.parametrize("fam", [16], indirect=True)
at_8 = pytest.mark.parametrize("fam", [8], indirect=True)


@sizes
def test_bytes_by_every_route(fam):
    mp.bytes_by_every_route(fam)


@at_16
def test_pinned_to_the_oracle(fam):
    mp.oracle_pin(fam)


@sizes
def test_a_table_of_one_circuit_is_the_batch_prover(fam):
    mp.table_of_one(fam)


@at_16
def test_lagrange_commits(fam):
    mp.bytes_by_every_route(fam, routes=("upload",), lagrange_commits=True)


@at_16
def test_one_segment_forced(fam):
    mp.bytes_by_every_route(fam, routes=("upload",), segments=1)


@sizes
def test_blinded_with_explicit_rows(fam):
    mp.blinded_with_explicit_rows(fam)


@at_8
def test_blinded_with_a_seed(fam):
    mp.blinded_with_a_seed(fam, check=(3,))


@sizes
def test_statuses_are_per_proof(fam):
    mp.statuses_are_per_proof(fam)


@at_16
def test_batches_in_sequence(fam):
    mp.batches_in_sequence(fam)


@at_8
def test_refusals(fam):
    mp.refusals(fam)


@at_8
def test_the_verifier_loads_the_resident_batch(fam):
    mp.verifier_loads_the_resident_batch(fam)
