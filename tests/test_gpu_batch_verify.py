"""GPU suite: the batch verifier at full size on the MI355X.  Cases: batch_verify_cases.py."""
import pytest

import batch_verify_cases as bc
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


@pytest.fixture(scope="module")
def chain512(setup):
    return bc.chain_circuit(setup, 512)


def test_bit_exact_folds(setup, chain512):
    bc.bit_exact_folds(bc.golden_circuit(setup), ranges=[(0, 2), (1, 2)])
    bc.bit_exact_folds(bc.factorization_circuit(setup))
    bc.bit_exact_folds(chain512, ranges=[(0, 8), (3, 7)], count=8)
    bc.bit_exact_folds(bc.poseidon_circuit(setup))


def test_verdicts_agree_with_the_per_proof_verifier(setup, chain512):
    bc.verdicts_agree(bc.golden_circuit(setup), [0, 1])
    bc.verdicts_agree(bc.factorization_circuit(setup), [0])
    bc.verdicts_agree(chain512, [1, 130, 257, 511])


def test_whole_batch_of_4096(setup):
    bc.whole_batch(bc.chain_circuit(setup, 4096))


def test_localisation(chain512):
    # four bad proofs in four different fields: 2 * z_1, W_zw_1 := W_z_1, c_eval + 1, the public input + 1
    bc.localisation(chain512, {0: 3, 255: 9, 256: 12, 511: 16}, max_checks=2 * 4 * 9 + 1)


def test_malformed_input_is_a_verdict(chain512):
    bc.malformed(chain512)


def test_degenerate_arithmetic(chain512):
    bc.degenerate_proofs(chain512)
    bc.mul_many_cases(counts=(1, 63, 64, 65), big_count=100000)


def test_arguments(chain512):
    bc.arguments(chain512)
