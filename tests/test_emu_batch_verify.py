"""CPU suite: the batch verifier on the emulated kernels (group_order 8 and 16, batches of at most 8).  Cases: batch_verify_cases.py."""
import pytest

import batch_verify_cases as bc
import parity_cases as pc


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


def test_bit_exact_folds(emu, setup):
    bc.bit_exact_folds(bc.golden_circuit(setup), ranges=[(0, 2), (1, 2)])
    bc.bit_exact_folds(bc.factorization_circuit(setup))


def test_verdicts_agree_with_the_per_proof_verifier(emu, setup):
    bc.verdicts_agree(bc.golden_circuit(setup), [0, 1])
    bc.verdicts_agree(bc.factorization_circuit(setup), [0])


def test_whole_batch_and_localisation(emu, setup):
    circ = bc.small_batch_circuit(setup, 8)
    bc.whole_batch(circ)
    bc.localisation(circ, {5: 11}, max_checks=7)  # one bad proof of 8 (b_eval + 1): 2 * 1 * 3 + 1 checks


def test_malformed_input_is_a_verdict(emu, setup):
    bc.malformed(bc.small_batch_circuit(setup, 6))


def test_degenerate_arithmetic(emu, setup):
    bc.degenerate_proofs(bc.small_batch_circuit(setup, 1))
    bc.mul_many_cases(counts=(1, 63, 64, 65), big_count=1000)


def test_arguments(emu, setup):
    bc.arguments(bc.small_batch_circuit(setup, 2))
