"""CPU suite: the batch verifier over a table of circuits on the emulated kernels (group_order 8 and 16, batches of at most 8).
Cases: multi_verify_cases.py."""
import pytest

import multi_verify_cases as mc
import parity_cases as pc


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


_built = {}


@pytest.fixture
def table(emu, setup):
    """built once, by the first test that asks: by then the emulated library is the bound one"""
    if "table" not in _built:
        _built["table"] = mc.tiny_table(setup)
    return _built["table"]


def test_bit_exact_folds(emu, table):
    mc.bit_exact_folds(table)


def test_a_table_of_one_circuit_equals_the_batch_verifier(emu, table):
    mc.one_circuit_equals_batch_verifier(table)


@pytest.mark.parametrize("of", ["A", "F", "Z", "A'", "P2"])
def test_verdicts_agree_with_the_per_proof_verifier(emu, table, of):
    mc.verdicts(table, [of])


def test_a_wrong_label_is_a_bad_proof(emu, table):
    mc.wrong_label(table)


def test_localisation_across_circuits(emu, table):
    # one bad proof of 8 (b_eval + 1) over three circuits: 2 * 1 * 3 + 1 checks
    mc.localisation(table, ["A", "F", "Z", "A", "F", "Z", "A", "A'"], {4: 11}, max_checks=7)


def test_malformed_input_is_a_verdict(emu, table):
    mc.malformed(table)


def test_resident_provers(emu, setup, table):
    small = mc.Table({n: table.circuits[n] for n in ("A", "F", "Z")})
    f1 = mc.tiny_circuit(setup, "F", 1)
    mc.resident_provers(small, [("A", table.circuits["A"]), ("F", f1), ("Z", table.circuits["Z"])], sample=[0, 3, 5])
    mc.resident_prover_errors(small, setup)


def test_limits(emu, table):
    mc.limits(table)


def test_arguments(emu, table):
    mc.arguments(table)
