"""The array tests of the field, curve and wave primitives (tests/primitive_cases.py) on an MI355X: the gfx950 build of
tests/probe/prim_probe.hip, one case per lane.  What differs from the host build is what is under test here — v_mad_i64_i32,
the register constraints of FPL_ANY_SIGN / PLONK_CHAIN / fpl_neg_mod_limb, the readfirstlane of a uniform operand — and the
hardware's own DPP, ds_swizzle and v_permlane exchanges in place of the emulator's model of them.  The library is a build product
(__graft_entry__.build()); nothing is compiled here."""
import os

import pytest

import primitive_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(pc.HIP_SO):
        pytest.fail("%s is missing: __graft_entry__.build() (make -C tests/probe) builds it; it is not compiled on the GPU machine" % pc.HIP_SO)
    return pc.load(pc.HIP_SO)


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
