"""Cases of the per-lane pairing checks on the device (plonk_pairing_check_many, plonk_verifier_set_x2, plonk_verifier_check_each,
`verify_each(..., device=True)`).

The same bodies run on the emulated kernels (tests/test_emu_pairing_device.py, a handful of lanes: an emulated lane costs about a
host pairing) and on the MI355X (tests/test_gpu_pairing_device.py).  Every expected verdict comes from the host pairing product
(`plonk_pairing_check`) or from the per-proof verifier (`vk.verify_proof`), both pinned to the oracle by the existing suite; two
checks are also put to oracle.pairing itself.  No verdict comes from the code under test.
"""
import ctypes
import random

import batch_verify_cases as bc
import multi_verify_cases as mc
import plonkathon_amd as pa
from helpers import R_MOD
from oracle import c_oracle, g1 as og1, pairing as opairing
from plonkathon_amd.field import Q_MOD
from plonkathon_amd.kzg import Fq2, pairing_check_many

P = Q_MOD
U = 4965661367192848881  # the BN parameter: p, r and t are polynomials in it


# ------------------------------------------------------------------------------------------ 1. the tower, against Python integers
def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f12_mul(a, b):
    """a, b: the six Fq2 coefficients of w^0 .. w^5; w^6 = xi = 9 + i"""
    t = [(0, 0)] * 11
    for i in range(6):
        for j in range(6):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    return [f2_add(t[k], f2_mul((9, 1), t[k + 6])) if k < 5 else t[k] for k in range(6)]


def f12_add(a, b):
    return [f2_add(x, y) for x, y in zip(a, b)]


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


F12_ONE = [(1, 0)] + [(0, 0)] * 5


def f12_bytes(a):
    return b"".join(int(c).to_bytes(32, "little") for k in a for c in k)


def f12_of(raw):
    v = [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(12)]
    return [(v[2 * k], v[2 * k + 1]) for k in range(6)]


def tower_identities(probe):
    """`probe`: tests/emu/libpairing_probe.so"""
    def op(code, a, b=None):
        out = ctypes.create_string_buffer(384)
        probe.probe_f12(code, f12_bytes(a), f12_bytes(b if b is not None else F12_ONE), out)
        return f12_of(out.raw)

    mul, sqr, inv, frob2, conj = (lambda a, b: op(0, a, b)), (lambda a: op(1, a)), (lambda a: op(2, a)), (lambda a: op(3, a)), (lambda a: op(4, a))
    rng = random.Random(12)
    rand = lambda: [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    sparse = [(P - 1, 0)] + [(0, 0)] * 4 + [(0, 5)]  # zeros and p - 1 among the coefficients
    for a, b in ((rand(), rand()), (rand(), sparse), (sparse, F12_ONE)):
        assert mul(a, b) == f12_mul(a, b)
        assert sqr(a) == f12_mul(a, a)
        assert f12_mul(a, inv(a)) == F12_ONE and mul(a, inv(a)) == F12_ONE  # f f^-1 = 1
        assert frob2(a) == f12_pow(a, P * P)  # the map itself, by Python integers
        assert frob2(mul(a, b)) == mul(frob2(a), frob2(b)) and frob2(f12_add(a, b)) == f12_add(frob2(a), frob2(b))  # a ring map
        x = a
        for _ in range(6):
            x = frob2(x)
        assert x == a  # of order six
        assert conj(a) == [c if k % 2 == 0 else ((-c[0]) % P, (-c[1]) % P) for k, c in enumerate(a)]
        line = [(rng.randrange(P), 0), b[1], (0, 0), b[3], (0, 0), (0, 0)]  # y + b0 w + b1 w^3, y in Fq
        assert op(5, a, line) == f12_mul(a, line)
    a = rand()
    assert conj(a) == f12_pow(a, P ** 6)  # conj is the p^6 power
    # the generated constants against Python integers
    gamma, gamma2, g2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), ctypes.create_string_buffer(128)
    hard, ate, sizes = (ctypes.c_uint32 * 24)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 3)()
    probe.probe_pairing_constants(gamma, gamma2, hard, ate, g2, sizes)
    xi_pow = f12_pow([(9, 1)] + [(0, 0)] * 5, (P * P - 1) // 6)
    want_gamma = xi_pow[0][0]
    assert xi_pow == [(want_gamma, 0)] + [(0, 0)] * 5 and pow(want_gamma, 3, P) == P - 1
    assert int.from_bytes(gamma.raw, "little") == want_gamma and int.from_bytes(gamma2.raw, "little") == want_gamma * want_gamma % P
    H = (P ** 4 - P ** 2 + 1) // R_MOD
    assert (P ** 6 - 1) * (P ** 2 + 1) * H * R_MOD == P ** 12 - 1
    assert sum(int(w) << (32 * i) for i, w in enumerate(hard)) == H and sum(int(w) << (32 * i) for i, w in enumerate(ate)) == 6 * U * U
    T = 6 * U * U
    assert list(sizes) == [T.bit_length() - 1 + bin(T).count("1") - 1, H.bit_length(), 24] and list(sizes)[:2] == [195, 761]
    assert bin(H).count("1") == 389
    assert [int.from_bytes(g2.raw[32 * i : 32 * i + 32], "little") for i in range(4)] == [c for q in opairing.G2 for c in q.c]


# ------------------------------------------------------------------------------------------ 2. check_many against the host
def _fq2(q):
    return (Fq2(q[0].c), Fq2(q[1].c))


Q7 = _fq2(opairing.multiply(opairing.G2, 7))  # Q0 = [7]_2; Q1 = the generator
_pool = []


def _mul(k):
    return c_oracle.g1_lincomb([og1.G1], [k % R_MOD])


def pool():
    """37 checks (A, B) over (Q7, G2), each with the HOST's verdict: e(a G, [7]H) e(-7a G, H) is true, the same with 7a + 1 false,
    both sides the identity true, exactly one side false.  True and false alternate, and 37 is odd, so a batch that cycles through
    the pool puts both into every wave at shifting lanes.  a = 1 and a = r - 1 come first."""
    if not _pool:
        rng = random.Random(5)
        for j in range(37):
            a = (1, 1, R_MOD - 1, R_MOD - 1)[j] if j < 4 else rng.randrange(1, R_MOD)
            A, B = _mul(a), _mul(-7 * a - (j % 2))  # odd j: off by one generator, a false check
            if j == 8:
                A = B = None
            elif j == 9:
                B = None
            elif j == 11:
                A = None
            want = pa.pairing_check([(A, Q7), (B, pa.G2)])
            _pool.append((A, B, want))
        wants = [w for _, _, w in _pool]
        assert wants[:4] == [True, False, True, False] and wants[8] and not wants[9] and not wants[11]
        assert all(w == (j % 2 == 0) for j, w in enumerate(wants))
    return _pool


def check_many_against_host(counts):
    for n in counts:
        checks = [pool()[i % 37] for i in range(n)]
        got = pairing_check_many((Q7, pa.G2), [(A, B) for A, B, _ in checks])
        assert got == [w for _, _, w in checks], n


def check_many_against_oracle():
    """a true and a false check of the pool under oracle.pairing (seconds each: no more than these two)"""
    picks = [pool()[4], pool()[5]]
    got = pairing_check_many((Q7, pa.G2), [(A, B) for A, B, _ in picks])
    q7 = opairing.multiply(opairing.G2, 7)
    for (A, B, _), verdict in zip(picks, got):
        assert verdict == (opairing.pairing(q7, A) * opairing.pairing(opairing.G2, B) == opairing.FQ12.one())
    assert got == [True, False]


def _g2_bytes(q):
    return b"".join(int(c).to_bytes(32, "little") for c in q[0].coeffs + q[1].coeffs)


def _g1_bytes(p):
    return int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little")


def check_many_arguments():
    ctx = pa.get_context()
    A, B, _ = pool()[0]
    g2 = _g2_bytes(Q7) + _g2_bytes(pa.G2)
    g1 = _g1_bytes(A) + _g1_bytes(B)

    def rc(g2=g2, g1=g1, flags=bytes(2), count=1):
        out = ctypes.create_string_buffer(max(count, 1))
        return ctx.L.plonk_pairing_check_many(ctx.handle, g2, g1, flags, count, out), out.raw

    assert rc() == (pa._lib.PLONK_OK, b"\1")
    assert rc(g1=_g1_bytes(A) + _g1_bytes((1, 3)))[0] == pa._lib.PLONK_ERR_ARG  # a G1 point off the curve
    assert rc(g1=_g1_bytes((P, 2)) + _g1_bytes(B))[0] == pa._lib.PLONK_ERR_ARG  # a coordinate >= p
    assert rc(g1=_g1_bytes((P, 2)) + _g1_bytes(B), flags=b"\1\0")[0] == pa._lib.PLONK_ERR_ARG  # ... even under an identity flag, as the host
    off = bytearray(g2)
    off[64:96] = ((int.from_bytes(off[64:96], "little") + 1) % P).to_bytes(32, "little")
    assert rc(g2=bytes(off))[0] == pa._lib.PLONK_ERR_ARG  # Q0 off the twist
    assert rc(g2=g2[:128] + bytes(128))[0] == pa._lib.PLONK_ERR_ARG  # Q1 the identity
    assert rc(g2=g2[:32] + b"\xff" * 32 + g2[64:])[0] == pa._lib.PLONK_ERR_ARG  # a G2 coordinate >= p
    assert rc(count=0)[0] == pa._lib.PLONK_ERR_ARG
    assert rc(flags=b"\0\1") == (pa._lib.PLONK_OK, b"\0")  # exactly one side the identity, through the flag


# ------------------------------------------------------------------------------------------ 3. verdicts of a batch
def batch_verdicts(circ, bad, others=None):
    """`bad`: {index: corruption number (0..16 of bc.corruptions)}; `others`: honest indices put to the per-proof verifier too
    (None: every proof)"""
    B = len(circ.recs)
    recs, pubs = list(circ.recs), [list(p) for p in circ.pubs]
    for i, which in bad.items():
        _, recs[i], pubs[i] = list(bc.corruptions(recs[i], pubs[i]))[which]
    _compare(circ.bv, b"".join(recs), pubs, B, circ.accepted_one_by_one, recs,
             range(B) if others is None else sorted(set(bad) | set(others)), [i not in bad for i in range(B)])


def _compare(bv, blob, pubs, B, one_by_one, recs, sample, want):
    bisected = bv.verify_each(blob, pubs, seed=bc.SEED)
    assert bisected == want and bv.device_checks == 0 and (bv.pairing_checks > 1) == (not all(want))
    for i in sample:
        assert one_by_one(recs[i], pubs[i]) == want[i], i  # the reference-pinned route
    assert bv.verify_each(blob, pubs, seed=bc.SEED, device=True) == bisected
    if all(want):
        assert bv.pairing_checks == 1 and bv.device_checks == 0  # the whole batch passed: that is the answer
        return
    assert bv.pairing_checks == 1 and bv.device_checks == B
    # nothing a fold reads has changed: folds before and after a check_each are the same
    bv.load(blob, pubs, bc.SEED)
    ranges = [(0, B), (B // 3, B - B // 4)]
    before = [bv.fold(lo, hi) for lo, hi in ranges]
    assert bv.check_each_device() == bisected and bv.device_checks == B
    assert [bv.fold(lo, hi) for lo, hi in ranges] == before and bv.status == bytes(B)


def every_corruption_in_one_batch(circ, index):
    """the 17 corruptions of proof `index` as one batch of 17 bad copies"""
    cases = list(bc.corruptions(circ.recs[index], circ.pubs[index]))
    assert len(cases) == 17
    recs, pubs = [r for _, r, _ in cases], [list(p) for _, _, p in cases]
    _compare(circ.bv, b"".join(recs), pubs, 17, circ.accepted_one_by_one, recs, range(17), [False] * 17)


def all_good_batch(circ):
    B = len(circ.recs)
    bv = circ.bv
    assert bv.verify_each(b"".join(circ.recs), circ.pubs, device=True) == [True] * B
    assert bv.pairing_checks == 1 and bv.device_checks == 0
    assert bv.verify_each_prover(circ.prover, device=True) == [True] * B and bv.device_checks == 0
    # and with nothing failed, the lanes agree: every proof's own check passes
    assert bv.check_each_device() == [True] * B and bv.device_checks == B


# ------------------------------------------------------------------------------------------ 4. malformed and degenerate proofs
def malformed(circ):
    """the six-proof batch of bc.malformed: proofs 1..4 spoilt, 0 and 5 honest"""
    recs, pubs = [bytearray(r) for r in circ.recs[:6]], circ.pubs[:6]
    circ.assert_valid(range(6))
    recs[1][64 * 3 : 64 * 3 + 32] = Q_MOD.to_bytes(32, "little")                    # z_1.x = p
    recs[2][576 + 32 : 576 + 64] = (R_MOD + 5).to_bytes(32, "little")                # b_eval >= r
    y = int.from_bytes(recs[3][64 * 4 + 32 : 64 * 5], "little")
    recs[3][64 * 4 + 32 : 64 * 5] = ((y + 1) % Q_MOD).to_bytes(32, "little")         # t_lo_1 off the curve
    recs[4][64 * 8 : 64 * 9] = bytes(64)                                             # W_zw_1 = 64 zero bytes
    blob = b"".join(bytes(r) for r in recs)
    want_status, want = bytes([0, 1, 1, 2, 4, 0]), [True, False, False, False, False, True]
    bv = circ.bv
    assert bv.verify_each(blob, pubs, device=True) == want and bv.status == want_status
    assert bv.pairing_checks == 1 and bv.device_checks == 0  # the spoilt proofs take part in no fold: the rest passes at once
    assert bv.check_each_device() == want and bv.status == want_status  # the lanes skip them: False without a pairing
    # one honest proof made bad as well: now the device route runs, over spoilt and bad proofs side by side
    _, bad_rec, bad_pub = list(bc.corruptions(bytes(recs[5]), pubs[5]))[11]
    blob2, pubs2 = blob[: 768 * 5] + bad_rec, pubs[:5] + [bad_pub]
    assert bv.verify_each(blob2, pubs2, device=True) == want[:5] + [False] and bv.status == want_status and bv.device_checks == 6
    assert bv.verify_each(blob2, pubs2) == want[:5] + [False]


def degenerate_proofs(circ):
    rec, pub = circ.recs[0], circ.pubs[0]
    circ.assert_valid([0])
    bv = circ.bv
    flat = bc.flat_of(rec)
    for name, bad in (("b_1 := a_1", dict(flat, b_1=flat["a_1"])), ("W_zw_1 := -W_z_1", dict(flat, W_zw_1=og1.neg(flat["W_z_1"])))):
        assert not circ.accepted_one_by_one(bc.record(bad), pub), name
        assert bv.verify_each(rec + bc.record(bad) + rec, [pub] * 3, device=True) == [True, False, True], name
        assert bv.pairing_checks == 1 and bv.device_checks == 3, name


# ------------------------------------------------------------------------------------------ 5. a table of circuits
def table_of_two(setup):
    """F: group order 16, one public input; P2: group order 8, two"""
    return mc.Table({"F": mc.tiny_circuit(setup, "F", 2), "P2": mc.tiny_circuit(setup, "P2", 2)})


def table_verdicts(table):
    ids, recs, pubs = table.deal_names(["F", "P2", "F", "P2"])
    table.assert_valid(ids, recs, pubs)
    bad = {1: 11, 2: 12}  # one bad proof in each circuit: b_eval + 1 in P2's first, c_eval + 1 in F's second
    for i, which in bad.items():
        _, recs[i], pubs[i] = list(bc.corruptions(recs[i], pubs[i]))[which]
        assert not table.accepted_one_by_one(ids[i], recs[i], pubs[i]), i
    mv, blob = table.mv, b"".join(recs)
    bisected = mv.verify_each(blob, ids, pubs, seed=bc.SEED)
    assert bisected == [True, False, False, True] and mv.device_checks == 0
    before = mv.fold(0, 4)
    assert mv.verify_each(blob, ids, pubs, seed=bc.SEED, device=True) == bisected
    assert mv.pairing_checks == 1 and mv.device_checks == 4 and mv.fold(0, 4) == before
    ids, recs, pubs = table.deal_names(["P2", "F", "F", "P2"])
    assert mv.verify_each(b"".join(recs), ids, pubs, device=True) == [True] * 4 and mv.device_checks == 0


# ------------------------------------------------------------------------------------------ 6. state errors
def state_errors(circ):
    ctx = pa.get_context()
    fresh = pa.BatchVerifier(circ.vk, len(circ.public_vars))
    out = ctypes.create_string_buffer(8)
    assert ctx.L.plonk_verifier_check_each(fresh._h, out) == pa._lib.PLONK_ERR_STATE  # before set_x2, before any load
    x2 = _g2_bytes(circ.vk.X_2)
    off = bytearray(x2)
    off[96:128] = ((int.from_bytes(off[96:128], "little") + 1) % P).to_bytes(32, "little")
    assert ctx.L.plonk_verifier_set_x2(fresh._h, bytes(off)) == pa._lib.PLONK_ERR_ARG  # off the twist
    assert ctx.L.plonk_verifier_set_x2(fresh._h, bytes(128)) == pa._lib.PLONK_ERR_ARG  # the identity
    assert ctx.L.plonk_verifier_check_each(fresh._h, out) == pa._lib.PLONK_ERR_STATE  # a refused point set nothing
    assert ctx.L.plonk_verifier_set_x2(fresh._h, x2) == pa._lib.PLONK_OK
    assert ctx.L.plonk_verifier_check_each(fresh._h, out) == pa._lib.PLONK_ERR_STATE  # tables, but no batch
    fresh.load(circ.recs[0], [circ.pubs[0]], bc.SEED)  # before the tables: load, then set_x2
    late = pa.BatchVerifier(circ.vk, len(circ.public_vars))
    late.load(circ.recs[0], [circ.pubs[0]], bc.SEED)
    assert ctx.L.plonk_verifier_check_each(late._h, out) == pa._lib.PLONK_ERR_STATE
    assert late.check_each_device() == [True] and fresh.check_each_device() == [True]
