"""GPU suite: the per-lane pairing checks on the MI355X.  Cases: pairing_device_cases.py."""
import pytest

import batch_verify_cases as bc
import pairing_device_cases as dc
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


@pytest.fixture(scope="module")
def chain512(setup):
    return bc.chain_circuit(setup, 512)


def test_check_many_against_the_host_pairing():
    dc.check_many_against_host(counts=(1, 63, 64, 65, 1000))  # one wave short of full, full, one lane into the second, 16 waves


def test_check_many_against_the_oracle_pairing():
    dc.check_many_against_oracle()


def test_check_many_arguments():
    dc.check_many_arguments()


def test_verdicts_of_a_batch(chain512):
    # the four corruptions of the localisation test, on both sides of a wave boundary: 2 * z_1, W_zw_1 := W_z_1, c_eval + 1, public + 1
    dc.batch_verdicts(chain512, {0: 3, 255: 9, 256: 12, 511: 16}, others=[1, 130, 257, 510])
    dc.all_good_batch(chain512)


def test_every_corruption_in_one_batch(chain512):
    dc.every_corruption_in_one_batch(chain512, 130)


def test_malformed_and_degenerate_proofs(chain512):
    dc.malformed(chain512)
    dc.degenerate_proofs(chain512)


def test_a_table_of_circuits(setup):
    dc.table_verdicts(dc.table_of_two(setup))


def test_state_errors(chain512):
    dc.state_errors(chain512)
