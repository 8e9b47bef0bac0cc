"""Bodies of the comb MSM's edge-case tests (csrc/msm_comb.h), shared by tests/test_emu_msm_comb_edges.py (emulated kernels) and
tests/test_gpu_msm_comb_edges.py (MI355X): the paths on which an item's table entry is the identity and is passed over by its
DIGIT (MSM_COMB_SKIP: an identity base, a group of the top tables whose codes are all zero, a group past the last scalar), the
sign applied to the packed words of y, the 32-bit entry index (and, with wide=True, the 64-bit one that only a table of more than
2^32 entries selects by itself: plonk_msm_lookup_configure mode | 64), and the rows of a batch.  Tiny combs over arbitrary bases (forced
mode: a table per call) build in milliseconds.  The checker is the oracle's ec_lincomb, with the bucket method as second witness."""
import random

from helpers import R_MOD

import plonkathon_amd as pa
from plonkathon_amd.field import Fq
from oracle import g1 as og1
from parity_cases import PTAU, P, affine  # noqa: F401

# (teeth, top tables): 254 mod 4, 6, 7 = 2, so these take top tables (one base per group for 4 and 6 teeth, two for 7)
TABLES = [(4, True), (6, True), (7, True), (5, False), (8, False)]
WIDE_TABLES = [(4, True), (7, True), (8, False)]  # the same bodies through msm_comb_kernel<false>: one and two bases per group, no top tables
SIZES = [1, 2, 6, 7, 8, 13, 50]  # around a group of 7 (the 21-tooth comb's), of 2 and of 1: empty, partial, full, one over
ALT5 = int("55" * 32, 16) % R_MOD
ALTA = int("aa" * 32, 16) % R_MOD
# 2^252 - 1, 2^252, 2^253: top-table codes 0, 1, 2 (two bits left over); 0x55.., 0xaa..: every tooth of every column both ways
SPECIAL = [0, 1, 2, R_MOD - 1, R_MOD - 2, (R_MOD - 1) // 2, (1 << 252) - 1, 1 << 252, 1 << 253, ALT5, ALTA]

_points = {}


def points(n, seed=77):
    """n distinct multiples of the generator (the oracle multiplies in pure Python: computed once per process)."""
    have = _points.setdefault(seed, [])
    rng = random.Random(seed * 1000 + len(have))
    while len(have) < n:
        have.append(og1.multiply((1, 2), rng.randrange(1, R_MOD)))
    return have[:n]


def _lincomb(pts, sc):
    got = pa.ec_lincomb([(None if q is None else (Fq(q[0]), Fq(q[1])), k) for q, k in zip(pts, sc)])
    return None if got is None else affine(got)


def _forced(h, top, body, wide=False):
    ctx = pa.get_context()
    try:
        ctx.msm_lookup(2, h, 0, top=top, wide=wide)
        body(ctx)
    finally:
        ctx.msm_lookup(0)  # (also clears `wide`)
        ctx.msm_configure(0, 0)


def special_scalars(h, top, wide=False):
    """Every size with the special scalars dealt round-robin from a different start, then three uniform vectors: all 1 (every
    top code zero: every group skipped), all 2^253 and all r - 1."""
    def body(ctx):
        for n in SIZES:
            pts = points(n)
            vectors = [[SPECIAL[(i + n) % len(SPECIAL)] for i in range(n)], [1 + 2 * i for i in range(n)], [1 << 253] * n, [R_MOD - 1] * n]
            for sc in vectors:
                assert _lincomb(pts, sc) == og1.ec_lincomb(list(zip(pts, sc))), (h, top, n, [hex(s) for s in sc[:4]])

    _forced(h, top, body, wide)


def cancelling_pairs(h, top, wide=False):
    """s P + (r - s) P on a duplicated base, the two side by side (with two bases per group they share a joint entry, which is the
    identity under NON-zero codes: s has bit 253 set) among other terms, and alone (the result is the identity)."""
    def body(ctx):
        rng = random.Random(h * 2 + top)
        for n in (2, 8, 13):
            base = points(n)
            pts, sc = [], []
            for i in range(0, n - 1, 2):
                s = (1 << 253) + (rng.randrange(1 << 252) | 1)
                pts += [base[i], base[i]]
                sc += [s, R_MOD - s]
            assert _lincomb(pts, sc) is None, (h, top, n, "pairs alone")
            rest, rs = base[n // 2:], [rng.randrange(R_MOD) for _ in base[n // 2:]]
            assert _lincomb(pts + rest, sc + rs) == og1.ec_lincomb(list(zip(rest, rs))), (h, top, n)

    _forced(h, top, body, wide)


def identity_bases(h, top, wide=False):
    """Base 0, a middle base and the last base are the identity: the result is the oracle's over the others, on the comb and on
    the bucket method."""
    def body(ctx):
        rng = random.Random(31 * h + top)
        for n in (1, 7, 13, 50):
            pts = list(points(n))
            for i in {0, n // 2, n - 1}:
                pts[i] = None
            for sc in ([SPECIAL[(i + 3) % len(SPECIAL)] for i in range(n)], [rng.randrange(R_MOD) for _ in range(n)]):
                want = og1.ec_lincomb(list(zip(pts, sc))) if any(q is not None for q in pts) else None
                assert _lincomb(pts, sc) == want, (h, top, n)
                ctx.msm_lookup(1)  # the bucket method
                assert _lincomb(pts, sc) == want, (h, top, n, "bucket method")
                ctx.msm_lookup(2, h, 0, top=top, wide=wide)

    _forced(h, top, body, wide)


def _rows(n, rng):
    return [[SPECIAL[(i + 5 * k) % len(SPECIAL)] if (i + k) % 2 else rng.randrange(R_MOD) for i in range(n)] for k in range(3)]


def batch_of_three(setup, h=0, top=False, sizes=(7, 13), wide=False):
    """Three MSMs in one call whose rows differ (commit_many of three coefficient vectors over the SRS): row pointers and strides.
    h = 0: the table the library chooses by itself."""
    def run(ctx):
        rng = random.Random(1234 + h)
        for n in sizes:
            rows = _rows(n, rng)
            got = setup.commit_many([P(r, pa.Basis.MONOMIAL) for r in rows])
            bases = [affine(p) for p in setup.powers_of_x[:n]]
            for k, r in enumerate(rows):
                assert (None if got[k] is None else affine(got[k])) == og1.ec_lincomb(list(zip(bases, r))), (h, top, n, k)

    if h:
        _forced(h, top, run, wide)
    else:
        run(pa.get_context())


def default_table(setup):
    """The table the library builds by default for the SRS: every size, the special scalars."""
    for n in SIZES:
        sc = [SPECIAL[(i + n) % len(SPECIAL)] for i in range(n)]
        got = setup.commit_coeffs(P(sc, pa.Basis.MONOMIAL))
        want = og1.ec_lincomb(list(zip([affine(p) for p in setup.powers_of_x[:n]], sc)))
        assert (None if got is None else affine(got)) == want, n
    info = setup.device_bases().lookup_info()
    assert info["layout"] == "comb", info


def wide_flag_arguments():
    """mode | 64 is a flag of the forced comb alone: with mode 0, mode 1 or the window tables the call returns PLONK_ERR_ARG and
    leaves the context as it was; with mode 2 and a comb it is accepted."""
    from plonkathon_amd import _lib

    ctx = pa.get_context()
    try:
        for mode, bits in ((0 | 64, 0), (1 | 64, 0), (0 | 64, 5), (1 | 64, 5), (2 | 16 | 64, 5), (0 | 16 | 64, 5)):
            assert ctx.L.plonk_msm_lookup_configure(ctx.handle, mode, bits, 0) == _lib.PLONK_ERR_ARG, (mode, bits)
        assert ctx.L.plonk_msm_lookup_configure(ctx.handle, 2 | 64, 5, 0) == _lib.PLONK_OK
        assert ctx.L.plonk_msm_lookup_configure(ctx.handle, 2 | 32 | 64, 7, 0) == _lib.PLONK_OK
        pts, sc = points(7), SPECIAL[:7]
        assert _lincomb(pts, sc) == og1.ec_lincomb(list(zip(pts, sc)))
    finally:
        ctx.msm_lookup(0)
        ctx.msm_configure(0, 0)
