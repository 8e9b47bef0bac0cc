"""fpl_from_fp_signed (csrc/fpl.h): the sign of a table point's y applied to its packed words before the unpack to 29-bit limbs —
host build with the emulator's range checks, against Python integers.  Both signs: the limbs' value is +-y exactly (so congruent
mod m), every limb is inside the bound the header states, and the product with a normalised element (the only use the mixed
addition makes of these limbs) passes fpl_dbg_check_product and reduces to +-y z / R."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import EMU_DIR, REPO
from oracle import field

M = field.Q_MOD
R261 = 1 << 261


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fpl_signed") / "libfpl_signed_probe.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-DPLONK_EMU", "-I", EMU_DIR, "-I", os.path.join(REPO, "plonkathon_amd", "csrc"),
                    "-Wno-unknown-pragmas", "-shared", "-o", so, os.path.join(EMU_DIR, "fpl_signed_probe.cpp"), os.path.join(EMU_DIR, "hip_emu.cpp")],
                   check=True, timeout=300)
    return ctypes.CDLL(so)


def _w(x):
    return (ctypes.c_uint32 * 8)(*[(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)])


def test_signed_unpack(probe):
    rng = random.Random(29)
    ys = [1, M - 1, (M - 1) // 2, 1 << 29, 1 << 200, 1 << 229, 5 << 29, (rng.randrange(M) >> 29) << 29, (M >> 58) << 58]  # (2^29 k: low 29 bits zero)
    ys += [rng.randrange(M) for _ in range(64)]
    zs = [M - 1, 1, (1 << 232) - 1] + [rng.randrange(M) for _ in range(3)]  # (2^232 - 1: limbs 0..7 all at 2^29 - 1)
    Ri = pow(R261, -1, M)
    limbs, prod = (ctypes.c_int32 * 9)(), (ctypes.c_uint32 * 8)()
    reached_top = False
    for y in ys:
        assert 0 < y < M
        for s, sign in ((0, 1), (0xFFFFFFFF, -1)):
            for z in zs:
                probe.probe_fpl_signed(_w(y), ctypes.c_uint32(s), _w(z), limbs, prod)
                l = [int(v) for v in limbs]
                assert sum(v << (29 * i) for i, v in enumerate(l)) == sign * y, (hex(y), s, l)
                assert 0 <= l[0] <= 1 << 29 and all(0 <= v < 1 << 29 for v in l[1:8]) and -(1 << 23) <= l[8] < 1 << 23, (hex(y), s, l)
                reached_top |= l[0] == 1 << 29
                assert sum(int(prod[i]) << (32 * i) for i in range(8)) == sign * y * z * Ri % M, (hex(y), s, hex(z))
    assert reached_top  # limb 0 = 2^29 exactly: the negative of a y whose low 29 bits are zero
