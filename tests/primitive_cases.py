"""Bodies of the array tests of the field, curve and wave primitives (csrc/fp.h, fpl.h, g1.h, wave.h), shared by
tests/test_emu_primitive_arrays.py (the host build of tests/probe/prim_probe.hip, with the range checks of fpl.h on) and
tests/test_gpu_primitives.py (the gfx950 build of the same file, on an MI355X).  The cases are those of tests/test_emu_primitives.py
and tests/test_emu_fpl_signed.py with the same seeds, laid out one case per lane; every comparison is exact integer equality
against Python integers and oracle.g1.  Each function takes the loaded probe library (load())."""
import ctypes
import os
import random

from helpers import GOLDEN
from oracle import field, g1

PROBE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe")
EMU_SO = os.path.join(PROBE_DIR, "libprim_probe_emu.so")
HIP_SO = os.path.join(PROBE_DIR, "libprim_probe_hip.so")

R261 = 1 << 261
L = (1 << 29) - 1
BLS_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # BLS12-381 Fr (ntt_bls.hip): 255 bits, 4m > 2^256
FIELDS = {"fr": (0, field.R_MOD), "fq": (1, field.Q_MOD), "bls_fr": (2, BLS_R)}
Q = field.Q_MOD
QRM, QRI = R261 % Q, pow(R261 % Q, -1, Q)
MASKS = (1, 2, 4, 8, 16, 32)

_P = ctypes.c_void_p
_PROTOTYPES = {
    "probe_field": [ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_int],
    "probe_fpl": [ctypes.c_int, _P, _P, _P, _P, _P, ctypes.c_int],
    "probe_fpl_signed": [_P, _P, _P, _P, _P, ctypes.c_int],
    "probe_fpl_uniform": [_P, _P, _P, ctypes.c_int],
    "probe_fpl_shoup": [ctypes.c_int, _P, _P, _P, ctypes.c_int],
    "probe_g1": [ctypes.c_int, _P, _P, _P, ctypes.c_int],
    "probe_g1l_chain": [ctypes.c_int, _P, _P, _P, _P, _P, ctypes.c_int],
    "probe_g1l_pair": [ctypes.c_int, _P, _P, _P, _P, ctypes.c_int],
    "probe_wave_words": [ctypes.c_int, ctypes.c_uint, _P, _P, _P, _P],
    "probe_g1_wave": [ctypes.c_int, _P, _P],
    "probe_g1l_wave": [ctypes.c_uint, _P, _P, _P],
}


def load(path):
    lib = ctypes.CDLL(path)
    for name, args in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args
    return lib


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
def _u32(vals):
    return (ctypes.c_uint32 * max(len(vals), 1))(*vals)


def _i32(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _words(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _elems(xs):  # packed words of a list of field elements
    return _u32([w for x in xs for w in _words(x)])


def _limb_rows(rows):  # rows of 9 signed limbs
    return _i32([v for r in rows for v in r])


def _elem_at(buf, i, stride=8, off=0):
    return sum((int(buf[stride * i + off + k]) & 0xFFFFFFFF) << (32 * k) for k in range(8))


def _limbs_at(buf, i, stride=9, off=0):
    return [int(buf[stride * i + off + k]) for k in range(9)]


def val(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def limbs_of(v):  # normalised limbs of a (possibly negative) value
    out = []
    for _ in range(8):
        out.append(v & L)
        v >>= 29
    return out + [v]


def _ok(rc):
    assert rc == 0, "the probe returned HIP status %d" % rc


def _same(got, want, what, cases=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, "lane %d" % i, cases[i] if cases is not None else None, g, w)


# ---- packed field operations -----------------------------------------------------------------------------------------------------
def _field_pairs(m):
    """The 1500-iteration mix of test_emu_primitives.test_field_ops (seed 1), then all 64 ordered pairs of its edge list."""
    Rm = R261 % m
    rng = random.Random(1)
    edge = [0, 1, 2, m - 1, m - 2, Rm, (m - 1) // 2, (1 << 253) % m]
    pairs = []
    for it in range(1500):
        a = rng.choice(edge) if it < 64 and it % 2 else rng.randrange(m)
        b = rng.choice(edge) if it < 64 else rng.randrange(m)
        pairs.append((a, b))
    pairs += [(a, b) for a in edge for b in edge]
    assert len(pairs) == 1564 and len(pairs) % 64  # the last wave is partial
    return pairs


def field_ops(lib, name):
    fid, m = FIELDS[name]
    Rm, Ri = R261 % m, pow(R261 % m, -1, m)
    pairs = _field_pairs(m)
    A, B = [a for a, _ in pairs], [b for _, b in pairs]

    def call(op, xs, ys=None):
        out = (ctypes.c_uint32 * (8 * len(xs)))()
        _ok(lib.probe_field(fid, op, _elems(xs), _elems(ys if ys is not None else [0] * len(xs)), out, len(xs)))
        return [_elem_at(out, i) for i in range(len(xs))]

    _same(call(0, A, B), [(a + b) % m for a, b in pairs], "add", pairs)
    _same(call(1, A, B), [(a - b) % m for a, b in pairs], "sub", pairs)
    _same(call(2, A, B), [a * b * Ri % m for a, b in pairs], "mul", pairs)
    _same(call(7, A), [a * a * Ri % m for a in A], "sqr", A)
    _same(call(4, A), [a * Rm % m for a in A], "to_mont", A)
    _same(call(5, A), [a * Ri % m for a in A], "from_mont", A)
    _same(call(6, A), [(-a) % m for a in A], "neg", A)
    # inversion (of 0: 0): the division steps on the whole mix and on the inputs that make them take unusually many / few rounds;
    # Fermat as the cross-check
    inv_in = A + [x % m for x in [1 << k for k in range(0, 254, 7)] + [m - (1 << k) for k in range(0, 254, 11)] + [3, m // 3, (m + 1) // 2]]
    mont = [a * Rm % m for a in inv_in]
    want = [field.inv(a, m) * Rm % m for a in inv_in]
    _same(call(3, mont), want, "inv", inv_in)
    _same(call(8, mont), want, "inv_fermat", inv_in)


# ---- raw signed limbs at the bounds ------------------------------------------------------------------------------------------------
def _limb_bound_cases():
    """The operands of test_emu_primitives.test_signed_limb_arithmetic_at_the_bounds (seed 9, the same draws in the same order).
    The operand-range filters are applied here, before anything is launched."""
    m = Q
    rng = random.Random(9)

    def diff_operand(kind, top):
        """difference of two normalised values: limbs 0..7 within [-L, L]; limb 8 sets the size (|value| ~ top * m)"""
        if kind == 0:
            lo = [L] * 8
        elif kind == 1:
            lo = [-L] * 8
        elif kind == 2:
            lo = [L if i % 2 else -L for i in range(8)]
        else:
            lo = [rng.randrange(-L, L + 1) for _ in range(8)]
        return lo + [(top * m) >> 232]

    mul, sqr, mad = [], [], []
    tops = [-9, -6, -3, -1, 0, 1, 2, 5, 9]
    for ka in range(4):
        for kb in range(4):
            for ta in tops:
                for tb in tops:
                    a, b = diff_operand(ka, ta), diff_operand(kb, tb)
                    if abs(val(a)) * abs(val(b)) > 128 * m * m:
                        continue
                    mul.append((a, b))
                    if ta == tb and ka == kb:
                        sqr.append(a)
                    c, d = diff_operand(kb, -tb), diff_operand(ka, ta)
                    if abs(val(a) * val(b)) + abs(val(c) * val(d)) <= 128 * m * m:
                        mad.append((a, b, c, d))
    # what the filters pass with this seed (1296 of 1296, 36, 1232 of 1296): a loosened or tightened filter cannot hide cases
    assert len(mul) >= 1296 and len(sqr) >= 36 and len(mad) >= 1200, (len(mul), len(sqr), len(mad))
    # one operand a SUM of two normalised values (limbs to 2^30), the other normalised
    mul.append(([2 * L] * 8 + [(3 * m) >> 232], [L] * 8 + [(2 * m) >> 232]))
    # carry sweep of the X3 shape: r2 - ppp - 2q
    norm = [[rng.randrange(-3 * L, L + 1) for _ in range(8)] + [rng.randrange(-(1 << 26), 1 << 26)] for _ in range(200)]
    # canonical conversion and the piece form, over the accumulator's ranges
    conv = {}
    for lo, hi, op in ((-127, 127, 4), (-7, 5, 5), (-1, 2, 6)):
        vs = [rng.randrange(lo * m + 1, hi * m) for _ in range(200)]
        vs += [v for v in (lo * m + 1, hi * m - 1, 0, -1, 1, m, -m) if lo * m < v < hi * m]
        conv[op] = vs
    return mul, sqr, mad, norm, conv


def _check_products(rows, wants, what, cases):
    for i, (r, want) in enumerate(zip(rows, wants)):
        assert all(0 <= v <= L for v in r[:8]), (what, i, cases[i], r)
        assert -Q < val(r) < 2 * Q, (what, i, cases[i], r)
        assert val(r) % Q == want % Q, (what, i, cases[i], r)


def signed_limb_arithmetic_at_the_bounds(lib):
    mul, sqr, mad, norm, conv = _limb_bound_cases()
    zero = [0] * 9

    def call(op, a, b=None, c=None, d=None):
        n = len(a)
        out = (ctypes.c_int32 * (9 * n))()
        _ok(lib.probe_fpl(op, _limb_rows(a), _limb_rows(b or [zero] * n), _limb_rows(c or [zero] * n), _limb_rows(d or [zero] * n), out, n))
        return [_limbs_at(out, i) for i in range(n)]

    _check_products(call(0, [a for a, _ in mul], [b for _, b in mul]), [val(a) * val(b) * QRI for a, b in mul], "fpl_mul", mul)
    _check_products(call(1, sqr), [val(a) * val(a) * QRI for a in sqr], "fpl_sqr", sqr)
    _check_products(call(2, *[[t[k] for t in mad] for k in range(4)]), [(val(a) * val(b) + val(c) * val(d)) * QRI for a, b, c, d in mad],
                    "fpl_mul_add", mad)
    for i, (x, r) in enumerate(zip(norm, call(3, norm))):
        assert all(0 <= v <= L for v in r[:8]) and val(r) == val(x), ("fpl_norm", i, x, r)
    for op, vs in conv.items():
        rows = call(op, [limbs_of(v) for v in vs])
        for i, (v, r) in enumerate(zip(vs, rows)):
            got = sum((r[k] & 0xFFFFFFFF) << (32 * k) for k in range(8))
            if op == 4:
                assert got == v % Q, ("fpl_to_fp", i, v, got)
            else:
                assert got % Q == v % Q and 0 <= got < 4 * Q, ("fpl_pack_lt4m", op, i, v, got)


def uniform_operand(lib):
    """fpl_from_fp_uniform of a kernel argument (scalar registers through readfirstlane on the device) times a per-lane operand:
    the left operands of the fpl_mul grid above, whose |value| stays below 10 m, against u < m."""
    mul = _limb_bound_cases()[0]
    ops = [a for a, _ in mul]
    rng = random.Random(13)
    for u in [Q - 1, 1, (1 << 232) - 1, QRM] + [rng.randrange(Q) for _ in range(2)]:  # (2^232 - 1: limbs 0..7 all at 2^29 - 1)
        assert all(abs(val(a)) * u <= 128 * Q * Q for a in ops)
        out = (ctypes.c_int32 * (9 * len(ops)))()
        _ok(lib.probe_fpl_uniform(_elems([u]), _limb_rows(ops), out, len(ops)))
        _check_products([_limbs_at(out, i) for i in range(len(ops))], [val(a) * u * QRI for a in ops], "fpl_mul by a uniform operand %x" % u, ops)


def shoup_multiplication_by_a_constant(lib, name, gen, reach):
    """test_emu_primitives.test_shoup_multiplication_by_a_constant (seed 11), one (operand, constant) pair per lane."""
    fid, m = FIELDS[name]
    rng = random.Random(11)
    consts = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, gen, pow(gen, (m - 1) // 2048, m)] + [rng.randrange(m) for _ in range(24)]
    cases = []
    for w in consts:
        operands = []
        for top in (-120, -55, -17, -2, -1, 0, 1, 2, 16, 55, 127):  # |value| up to 128 r
            for kind in range(4):
                lo = [L] * 8 if kind == 0 else [-L] * 8 if kind == 1 else [2 * L if i % 2 else -L for i in range(8)] if kind == 2 else [rng.randrange(-L, 2 * L) for _ in range(8)]
                operands.append(lo + [(top * m) >> 232])
        operands.append([int(1.26 * (1 << 30))] * 8 + [0])   # the largest limbs fpl_mul's callers produce
        operands.append([-int(1.26 * (1 << 30))] * 8 + [0])
        cases += [(a, w) for a in operands if abs(val(a)) < reach * m]
    assert len(cases) >= 32 * 30
    n = len(cases)
    out = (ctypes.c_int32 * (27 * n))()
    _ok(lib.probe_fpl_shoup(fid, _limb_rows([a for a, _ in cases]), _elems([w * R261 % m for _, w in cases]), out, n))
    for i, (a, w) in enumerate(cases):
        r, wl, wp = _limbs_at(out, i, 27), _limbs_at(out, i, 27, 9), _limbs_at(out, i, 27, 18)
        assert val(wl) == w and val(wp) == (w << 261) // m, (i, a, w)
        assert all(0 <= v <= L for v in r[:8]), (i, a, w, r)
        assert val(r) % m == val(a) * w % m, (i, a, w, r)
        assert -1.8 * m < val(r) < 2.8 * m, (i, a, w, r)


def signed_unpack(lib):
    """test_emu_fpl_signed.test_signed_unpack (seed 29): ys x both signs x zs, one combination per lane."""
    M = Q
    rng = random.Random(29)
    ys = [1, M - 1, (M - 1) // 2, 1 << 29, 1 << 200, 1 << 229, 5 << 29, (rng.randrange(M) >> 29) << 29, (M >> 58) << 58]  # (2^29 k: low 29 bits zero)
    ys += [rng.randrange(M) for _ in range(64)]
    zs = [M - 1, 1, (1 << 232) - 1] + [rng.randrange(M) for _ in range(3)]  # (2^232 - 1: limbs 0..7 all at 2^29 - 1)
    Ri = pow(R261, -1, M)
    cases = [(y, s, sign, z) for y in ys for s, sign in ((0, 1), (0xFFFFFFFF, -1)) for z in zs]
    n = len(cases)
    limbs, prod = (ctypes.c_int32 * (9 * n))(), (ctypes.c_uint32 * (8 * n))()
    _ok(lib.probe_fpl_signed(_elems([c[0] for c in cases]), _u32([c[1] for c in cases]), _elems([c[3] for c in cases]), limbs, prod, n))
    reached_top = False
    for i, (y, s, sign, z) in enumerate(cases):
        assert 0 < y < M
        l = _limbs_at(limbs, i)
        assert val(l) == sign * y, (hex(y), s, l)
        assert 0 <= l[0] <= 1 << 29 and all(0 <= v < 1 << 29 for v in l[1:8]) and -(1 << 23) <= l[8] < 1 << 23, (hex(y), s, l)
        reached_top |= l[0] == 1 << 29
        assert _elem_at(prod, i) == sign * y * z * Ri % M, (hex(y), s, hex(z))
    assert reached_top  # limb 0 = 2^29 exactly: the negative of a y whose low 29 bits are zero


# ---- curve ---------------------------------------------------------------------------------------------------------------------------
def _pt_words(p):
    x, y = (0, 0) if p is None else (p[0] * QRM % Q, p[1] * QRM % Q)
    return _words(x) + _words(y)


def _pt_at(buf, i):
    x, y = _elem_at(buf, i, 16) * QRI % Q, _elem_at(buf, i, 16, 8) * QRI % Q
    return None if x == 0 and y == 0 else (x, y)


_cache = {}


def _formula_points():
    if "pts" not in _cache:
        G = g1.G1
        _cache["pts"] = [None, G, g1.multiply(G, 2), g1.multiply(G, 3), g1.neg(G), g1.multiply(G, 123456789), g1.neg(g1.multiply(G, 2))]
    return _cache["pts"]


def _srs():
    if "srs" not in _cache:
        from oracle.srs import Setup

        _cache["srs"] = Setup.from_file(os.path.join(GOLDEN, "srs_2048.ptau")).powers_of_x
    return _cache["srs"]


def g1_formulas_and_exceptional_cases(lib):
    """The 7 x 7 point table of test_emu_primitives through the five operations of probe_g1."""
    pts = _formula_points()
    pairs = [(p, q) for p in pts for q in pts]
    n = len(pairs)
    pw, qw = _u32([w for p, _ in pairs for w in _pt_words(p)]), _u32([w for _, q in pairs for w in _pt_words(q)])
    for op in range(5):
        out = (ctypes.c_uint32 * (16 * n))()
        _ok(lib.probe_g1(op, pw, qw, out, n))
        for i, (p, q) in enumerate(pairs):
            want = (g1.add(p, q), g1.add(p, q), g1.double(p), g1.add(g1.double(p), q), g1.add(g1.double(p), g1.double(q)))[op]
            assert _pt_at(out, i) == want, (op, p, q)


def _chains():
    """The chains of test_emu_primitives.test_lazy_accumulator_chain (seed 5) with the random ones capped at 40 points, and its ten
    hand-written exceptional lists."""
    P = _srs()
    rng = random.Random(5)
    chains = []
    for _ in range(12):
        n = 1 + rng.randrange(1, 300) % 40
        chains.append(([P[rng.randrange(2048)] for _ in range(n)], [rng.randrange(2) for _ in range(n)]))
    G = P[0]
    exceptional = [([G, G], [0, 0]), ([G, G], [0, 1]), ([G, G, P[1]], [0, 1, 0]), ([G] * 5, [0] * 5),
                   ([P[3], P[4], P[3], P[4]], [0, 0, 1, 1]), ([P[5]] * 9, [0] * 9), ([None, G, None], [0, 0, 0]),
                   # a negated point into the empty accumulator, then additions: R = S2 - Y1 with Y1 = -y
                   ([G, P[1], P[2]], [1, 0, 1]), ([P[7], P[8], P[9], P[10]], [1, 1, 0, 0]), ([None, P[6], P[5]], [0, 1, 0])]
    return chains + exceptional, len(chains)


def _chain_model(pts, negs, signed_entry):
    """-> (the sum, the number of steps the fast entry must refuse): an identity addend (the zero test of g1l_madd_fast; the signed
    entry never sees one), or an addend equal or opposite to the accumulator."""
    acc, refused = None, 0
    for p, ng in zip(pts, negs):
        q = g1.neg(p) if ng else p
        if q is None:
            refused += 0 if signed_entry else 1
            continue
        if acc is not None and acc[0] == q[0]:
            refused += 1
        acc = g1.add(acc, q)
    return acc, refused


def lazy_accumulator_chain(lib, signed_entry):
    chains, n_random = _chains()
    n = len(chains)
    start = [0]
    for pts, _ in chains:
        start.append(start[-1] + len(pts))
    out, info = (ctypes.c_uint32 * (16 * n))(), (ctypes.c_int32 * (2 * n))()
    _ok(lib.probe_g1l_chain(1 if signed_entry else 0, _u32([w for pts, _ in chains for p in pts for w in _pt_words(p)]),
                            _i32([v for _, negs in chains for v in negs]), _i32(start), out, info, n))
    total_refused = 0
    for i, (pts, negs) in enumerate(chains):
        want, refused = _chain_model(pts, negs, signed_entry)
        assert _pt_at(out, i) == want, (i, negs)
        assert info[2 * i + 1] == 15, ("piece routes that disagree with the direct route", i, info[2 * i + 1])
        # the exceptional lists prove they reached the packed fall-back; the random ones that they did not
        assert info[2 * i] == refused, (i, negs, info[2 * i], refused)
        total_refused += refused if i >= n_random else 0
    assert total_refused >= 6  # (the signed entry is not shown the three identity addends)


def _xyzz_words(p, z):
    """XYZZ words (Montgomery) of the affine point p scaled by z: (x z^2, y z^3, z^2, z^3); the identity is all zero."""
    if p is None:
        return [0] * 32
    zz, zzz = z * z % Q, z * z * z % Q
    return [w for v in (p[0] * zz, p[1] * zzz, zz, zzz) for w in _words(v * QRM % Q)]


def _lazy_at(buf, i):
    """-> (the four limb rows, the identity flag) of lane i of a 37-int32 lazy XYZZ."""
    return [_limbs_at(buf, i, 37, 9 * k) for k in range(4)], int(buf[37 * i + 36])


def _lazy_point(rows, inf):
    """The affine point of a lazy XYZZ, after checking the accumulator invariants of g1.h: limbs 0..7 normalised, x within
    (-7m, 5m), y, zz, zzz within (-m, 2m)."""
    if inf:
        return None
    for k, r in enumerate(rows):
        assert all(0 <= v <= L for v in r[:8]), (k, r)
        assert (-7 * Q < val(r) < 5 * Q) if k == 0 else (-Q < val(r) < 2 * Q), (k, r)
    x, y, zz, zzz = (val(r) % Q for r in rows)
    assert zz and zzz
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


def _unpacked(words32):
    """What g1l_from_xyzz makes of 32 canonical words: the plain 29-bit limbs, and the identity flag."""
    vs = [sum(words32[8 * k + i] << (32 * i) for i in range(8)) for k in range(4)]
    return [limbs_of(v) for v in vs], 1 if vs[2] == 0 else 0


def lazy_general_addition(lib):
    """g1l_add_fast<false>, <true> and g1l_dbl on the 7 x 7 table, with trivial and with random ZZ on both sides (equal and
    opposite points are then equal and opposite in different coordinates)."""
    pts = _formula_points()
    rng = random.Random(17)
    cases = []
    for p in pts:
        for q in pts:
            cases.append((p, 1, q, 1))
            cases.append((p, rng.randrange(2, Q), q, rng.randrange(2, Q)))
    n = len(cases)
    pw = [_xyzz_words(p, zp) for p, zp, _, _ in cases]
    qw = [_xyzz_words(q, zq) for _, _, q, zq in cases]
    seen = set()
    for op in range(3):
        out, ret = (ctypes.c_int32 * (37 * n))(), (ctypes.c_int32 * n)()
        _ok(lib.probe_g1l_pair(op, _u32([w for r in pw for w in r]), _u32([w for r in qw for w in r]), out, ret, n))
        for i, (p, _, q, _) in enumerate(cases):
            rows, inf = _lazy_at(out, i)
            what = (op, i, p, q)
            if op == 2:
                assert _lazy_point(rows, inf) == g1.double(p), what
                continue
            equal = p is not None and p == q
            opposite = p is not None and q is not None and p == g1.neg(q)
            if equal or (opposite and op == 0):  # refused, p untouched
                assert ret[i] == 0 and (rows, inf) == _unpacked(pw[i]), what
                seen.add("equal" if equal else "opposite refused")
            elif opposite:  # OPPOSITE_OK: resolved to the identity
                assert ret[i] == 1 and inf == 1, what
                seen.add("opposite resolved")
            else:
                assert ret[i] == 1 and _lazy_point(rows, inf) == g1.add(p, q), what
                if p is None or q is None:  # a copy: the other operand's limbs (or p's own) as they were
                    assert (rows, inf) == _unpacked(pw[i] if q is None else qw[i]), what
    assert seen == {"equal", "opposite refused", "opposite resolved"}


# ---- wave ----------------------------------------------------------------------------------------------------------------------------
def wave_exchanges(lib):
    """wave_lane_xor and wave_swap_words for the six masks, on distinct 32-bit tags per lane and register."""
    rng = random.Random(23)
    tags = rng.sample(range(1 << 32), 128)
    a, b = tags[:64], tags[64:]
    for mask in MASKS:
        for swap in (0, 1):
            oa, ob = (ctypes.c_uint32 * 64)(), (ctypes.c_uint32 * 64)()
            _ok(lib.probe_wave_words(swap, mask, _u32(a), _u32(b), oa, ob))
            for lane in range(64):
                if not swap:
                    want = (a[lane ^ mask], b[lane])
                elif lane & mask:  # bit set: keeps b, receives its partner's b into a
                    want = (b[lane ^ mask], b[lane])
                else:              # bit clear: keeps a, receives its partner's a into b
                    want = (a[lane], a[lane ^ mask])
                assert (oa[lane], ob[lane]) == want, ("wave_swap_words" if swap else "wave_lane_xor", mask, lane)


def _wave_points():
    """64 distinct multiples k_l G (computed once per process)."""
    if "wave" not in _cache:
        rng = random.Random(41)
        ks = rng.sample(range(1, 1 << 48), 64)
        _cache["wave"] = (ks, [g1.multiply(g1.G1, k) for k in ks])
    return _cache["wave"]


def _xyzz_point_at(buf, i):
    x, y, zz, zzz = (_elem_at(buf, i, 32, 8 * k) for k in range(4))
    if zz == 0:
        return None
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


def g1_wave_reductions(lib):
    ks, pts = _wave_points()

    def run(op, lanes):
        out = (ctypes.c_uint32 * (64 * 32))()
        _ok(lib.probe_g1_wave(op, _u32([w for p in lanes for w in _pt_words(p)]), out))
        return [_xyzz_point_at(out, i) for i in range(64)]

    total = g1.multiply(g1.G1, sum(ks))
    assert run(0, pts) == [total] * 64  # every lane holds the total
    got = run(1, pts)
    for lane in (0, 1, 7, 31, 32, 33, 62, 63):
        assert got[lane] == g1.multiply(g1.G1, sum(ks[lane:])), lane
    # identities in half the lanes
    rng = random.Random(43)
    empty = set(rng.sample(range(64), 32))
    lanes = [None if i in empty else p for i, p in enumerate(pts)]
    assert run(0, lanes) == [g1.multiply(g1.G1, sum(k for i, k in enumerate(ks) if i not in empty))] * 64
    assert run(0, [None] * 64) == [None] * 64


def g1l_wave_steps(lib):
    ks, pts = _wave_points()

    def run(mask, lanes):
        out, ret = (ctypes.c_int32 * (64 * 37))(), (ctypes.c_int32 * 64)()
        _ok(lib.probe_g1l_wave(mask, _u32([w for p in lanes for w in _pt_words(p)]), out, ret))
        return [_lazy_at(out, i) for i in range(64)], list(ret)

    for mask in MASKS:
        got, ret = run(mask, pts)
        assert ret == [1] * 64, mask
        for lane in range(64):
            assert _lazy_point(*got[lane]) == g1.add(pts[lane], pts[lane ^ mask]), (mask, lane)
        # lanes l and l ^ mask hold the same point: both refuse, and both are untouched
        same = [pts[lane & ~mask] for lane in range(64)]
        got, ret = run(mask, same)
        assert ret == [0] * 64, mask
        for lane in range(64):
            assert got[lane] == _unpacked(_xyzz_words(same[lane], 1)), (mask, lane)
    # the chain <1, true> .. <32, true> of msm_comb_finalize_kernel: every lane holds the total
    total = g1.multiply(g1.G1, sum(ks))
    got, ret = run(0, pts)
    assert ret == [1] * 64
    assert [_lazy_point(*g) for g in got] == [total] * 64
    rng = random.Random(47)
    empty = set(rng.sample(range(64), 32))
    got, ret = run(0, [None if i in empty else p for i, p in enumerate(pts)])
    assert ret == [1] * 64
    assert [_lazy_point(*g) for g in got] == [g1.multiply(g1.G1, sum(k for i, k in enumerate(ks) if i not in empty))] * 64
    # opposite points in lanes l and l ^ 1: resolved to the identity in the first step (OPPOSITE_OK), and the total is the identity
    got, ret = run(0, [g1.neg(pts[lane - 1]) if lane & 1 else pts[lane] for lane in range(64)])
    assert ret == [1] * 64 and all(inf == 1 for _, inf in got)
    # equal points in lanes l and l ^ 1: a doubling, which the chain refuses in every lane
    _, ret = run(0, [pts[lane & ~1] for lane in range(64)])
    assert ret == [0] * 64
