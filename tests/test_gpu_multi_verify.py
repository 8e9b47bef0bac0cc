"""GPU suite: the batch verifier over a table of circuits on the MI355X.  Cases: multi_verify_cases.py."""
import pytest

import batch_verify_cases as bc
import multi_verify_cases as mc
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


_built = {}


@pytest.fixture
def table(setup):
    """built once, by the first test that asks: by then the device library is the bound one"""
    if "table" not in _built:
        _built["table"] = mc.tiny_table(setup)
    return _built["table"]


@pytest.fixture
def large(setup):
    """chain x 256, Poseidon x 2, A x 64, and A x 4 from a blinding prover: each resident in its prover (built once)"""
    if "large" not in _built:
        _built["large"] = {"chain": bc.chain_circuit(setup, 256), "Poseidon": bc.poseidon_circuit(setup), "A": mc.tiny_circuit(setup, "A", 64),
                           "A blinded": mc.tiny_circuit(setup, "A", 4, blinding=bytes(range(1, 33)))}
    return _built["large"]


def test_bit_exact_folds(table):
    mc.bit_exact_folds(table)


def test_bit_exact_folds_of_large_circuits(large):
    t = mc.Table({n: large[n] for n in ("chain", "Poseidon", "A")})
    mc.bit_exact_folds(t, names=["chain", "A", "Poseidon", "chain", "Poseidon"], ranges=((0, 5), (1, 4)))


def test_a_table_of_one_circuit_equals_the_batch_verifier(table):
    mc.one_circuit_equals_batch_verifier(table)


@pytest.mark.parametrize("of", ["A", "F", "Z", "A'", "P2"])
def test_verdicts_agree_with_the_per_proof_verifier(table, of):
    mc.verdicts(table, [of])


def test_a_wrong_label_is_a_bad_proof(table):
    mc.wrong_label(table)


def test_localisation_across_circuits(setup):
    # 300 proofs dealt A, A', F in turn: a 256-lane strided loop wraps and every sub-range cuts across circuits.  Three bad
    # proofs in three circuits and three fields: 2 * z_1 (A), c_eval + 1 (A'), the public input + 1 (F)
    t = mc.Table({n: mc.tiny_circuit(setup, n, 100) for n in ("A", "A'", "F")})
    mc.localisation(t, ["A", "A'", "F"] * 100, {0: 3, 256: 12, 299: 16}, max_checks=2 * 3 * 9 + 1)


def test_malformed_input_is_a_verdict(table):
    mc.malformed(table)


def test_resident_provers(setup, table, large):
    t = mc.Table({n: large[n] for n in ("chain", "Poseidon", "A")})
    # the per-proof verifier on two proofs of each large circuit and two of A, one of them blinded
    mc.resident_provers(t, [("chain", large["chain"]), ("Poseidon", large["Poseidon"]), ("A", large["A"]), ("A", large["A blinded"])],
                        sample=[1, 255, 256, 257, 258, 325])
    small = mc.Table({n: table.circuits[n] for n in ("A", "F", "Z")})
    mc.resident_prover_errors(small, setup)


def test_limits(table):
    mc.limits(table)


def test_arguments(table):
    mc.arguments(table)
