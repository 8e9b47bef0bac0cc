"""The array tests of the field, curve and wave primitives (tests/primitive_cases.py) on the host build of
tests/probe/prim_probe.hip: the same kernels the MI355X run launches, compiled with g++ against tests/emu/hip_emu.h, one case
per emulated lane, with the range checks of csrc/fpl.h on."""
import subprocess

import pytest

import primitive_cases as pc


@pytest.fixture(scope="module")
def probe():
    subprocess.run(["make", "-s", "-C", pc.PROBE_DIR, "libprim_probe_emu.so"], check=True)
    return pc.load(pc.EMU_SO)


@pytest.mark.parametrize("name", list(pc.FIELDS))
def test_field_ops(probe, name):
    pc.field_ops(probe, name)


def test_signed_limb_arithmetic_at_the_bounds(probe):
    pc.signed_limb_arithmetic_at_the_bounds(probe)


def test_uniform_operand(probe):
    pc.uniform_operand(probe)


@pytest.mark.parametrize("name,gen,reach", [("fr", 5, 128), ("bls_fr", 7, 56)])
def test_shoup_multiplication_by_a_constant(probe, name, gen, reach):
    pc.shoup_multiplication_by_a_constant(probe, name, gen, reach)


def test_signed_unpack(probe):
    pc.signed_unpack(probe)


def test_g1_formulas_and_exceptional_cases(probe):
    pc.g1_formulas_and_exceptional_cases(probe)


@pytest.mark.parametrize("signed_entry", [False, True], ids=["madd_fast", "madd_signed"])
def test_lazy_accumulator_chain(probe, signed_entry):
    pc.lazy_accumulator_chain(probe, signed_entry)


def test_lazy_general_addition(probe):
    pc.lazy_general_addition(probe)


def test_wave_exchanges(probe):
    pc.wave_exchanges(probe)


def test_g1_wave_reductions(probe):
    pc.g1_wave_reductions(probe)


def test_g1l_wave_steps(probe):
    pc.g1l_wave_steps(probe)
