"""CPU suite: the per-lane pairing checks on the emulated kernels (a lane costs about a host pairing there: well under a hundred
lanes in the whole file) and the tower of pairing_tower.h against Python integers.  Cases: pairing_device_cases.py."""
import ctypes
import os
import subprocess

import pytest

import batch_verify_cases as bc
import pairing_device_cases as dc
import parity_cases as pc
from conftest import EMU_DIR


@pytest.fixture(scope="module")
def setup(emu_cdll):
    from plonkathon_amd import Setup

    return Setup.from_file(pc.PTAU)


def test_tower_identities_and_generated_constants(emu_cdll):
    subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "pairing_probe.mk", "libpairing_probe.so"], check=True)  # the probe has a recipe of its own
    dc.tower_identities(ctypes.CDLL(os.path.join(EMU_DIR, "libpairing_probe.so")))


def test_check_many_against_the_host_pairing(emu):
    dc.check_many_against_host(counts=(1, 2, 7))


def test_check_many_against_the_oracle_pairing(emu):
    dc.check_many_against_oracle()


def test_check_many_arguments(emu):
    dc.check_many_arguments()


def test_verdicts_of_a_batch(emu, setup):
    circ = bc.small_batch_circuit(setup, 8)
    dc.batch_verdicts(circ, {5: 11})
    dc.batch_verdicts(circ, {0: 3, 5: 12, 7: 16})
    dc.all_good_batch(circ)


def test_malformed_and_degenerate_proofs(emu, setup):
    circ = bc.small_batch_circuit(setup, 6)
    dc.malformed(circ)
    dc.degenerate_proofs(circ)


def test_a_table_of_circuits(emu, setup):
    dc.table_verdicts(dc.table_of_two(setup))


def test_state_errors(emu, setup):
    dc.state_errors(bc.small_batch_circuit(setup, 1))
