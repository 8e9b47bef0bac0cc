"""Cases of the batch verifier (plonkathon_amd.BatchVerifier, plonk_verifier_*, plonk_g1_mul_many).

The same bodies run on the emulated kernels (tests/test_emu_batch_verify.py, small sizes) and on the MI355X
(tests/test_gpu_batch_verify.py, full size).  Every valid input is first shown valid by the per-proof verifier
(`vk.verify_proof`, pinned to the reference's by the golden tests), so no case passes by accepting or rejecting everything.
Expected fold points come from the oracle alone: the term table of the issue evaluated with oracle.field arithmetic,
oracle.g1.ec_lincomb, and weights recomputed by oracle.strobe_merlin.MerlinTranscript.
"""
import copy
import ctypes
import random

import pytest

import parity_cases as pc
import plonkathon_amd as pa
from helpers import R_MOD, load, pt
from oracle import c_oracle, g1 as og1, pairing as opairing
from oracle.field import inv, root_of_unity
from oracle.fr_poly import Basis as OBasis, Polynomial as OPoly
from oracle.strobe_merlin import MerlinTranscript
from oracle.verifier import VerificationKey as OVerificationKey
from plonkathon_amd import BatchProver, BatchVerifier, Program
from plonkathon_amd.field import Q_MOD

POINTS = ("a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "W_z_1", "W_zw_1")
EVALS = ("a_eval", "b_eval", "c_eval", "s1_eval", "s2_eval", "z_shifted_eval")
FIXED = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")
SEED = bytes(range(32))
K6_LINES = ["e public", "c <== a * b", "e <== c * d"]


# ------------------------------------------------------------------------------------------ records and fixtures
def record(flat):
    """768-byte record (plonk_prover_download's layout) of a flat proof: points = int pairs or None, evaluations = ints."""
    out = b""
    for k in POINTS:
        p = flat[k]
        out += bytes(64) if p is None else int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little")
    return out + b"".join(int(flat[k]).to_bytes(32, "little") for k in EVALS)


def flat_of(rec):
    f = {}
    for i, k in enumerate(POINTS):
        x, y = int.from_bytes(rec[64 * i : 64 * i + 32], "little"), int.from_bytes(rec[64 * i + 32 : 64 * i + 64], "little")
        f[k] = None if x == 0 and y == 0 else (x, y)
    for i, k in enumerate(EVALS):
        f[k] = int.from_bytes(rec[576 + 32 * i : 608 + 32 * i], "little")
    return f


class Circuit:
    """One circuit with proofs of it: the product's verification key, the oracle's view of the same key, records and public rows."""

    def __init__(self, setup, lines, n, witnesses=(), extra_records=(), extra_publics=()):
        self.n = n
        self.program = Program(lines, n)
        self.vk = setup.verification_key(self.program.common_preprocessed_input())
        x2 = (opairing.FQ2([c.n for c in self.vk.X_2[0].coeffs]), opairing.FQ2([c.n for c in self.vk.X_2[1].coeffs]))
        self.ovk = OVerificationKey(n, *[pc.affine(getattr(self.vk, k)) for k in FIXED], x2, self.vk.w.n)
        self.public_vars = self.program.get_public_assignments()
        self.recs, self.pubs = list(extra_records), [list(p) for p in extra_publics]
        self.prover = None
        if witnesses:
            self.prover = BatchProver(setup, self.program)
            self.prover.upload([dict(w) for w in witnesses])
            self.prover.run()
            blob, status = self.prover.download_raw()
            assert not any(status)
            self.recs += [blob[768 * i : 768 * (i + 1)] for i in range(len(witnesses))]
            self.pubs += [[w[v] % R_MOD for v in self.public_vars] for w in witnesses]
        self.bv = BatchVerifier(self.vk, len(self.public_vars))

    def accepted_one_by_one(self, rec, pub):
        """the per-proof verifier's verdict (the reference-pinned route)"""
        return self.vk.verify_proof(self.n, BatchProver.decode(rec), list(pub))

    def assert_valid(self, indices=None):
        for i in range(len(self.recs)) if indices is None else indices:
            assert self.accepted_one_by_one(self.recs[i], self.pubs[i]), i


def golden_circuit(setup):
    """The K6 proof of the reference and a second witness of the same circuit."""
    k6 = load("k6_proof.json")
    flat = {k: (pt(v) if isinstance(v, list) else int(v)) for k, v in k6["proof"].items()}
    program = Program(k6["program"], k6["group_order"])
    second = program.fill_variable_assignments({"a": 2, "b": 5, "d": 7})
    return Circuit(setup, k6["program"], k6["group_order"], [second], [record(flat)], [[int(k6["witness"]["e"])]])


def factorization_circuit(setup):
    program = Program(pc.FACTORIZATION, 16)
    return Circuit(setup, pc.FACTORIZATION, 16, [program.fill_variable_assignments(pc.FACTORIZATION_START)])


def small_batch_circuit(setup, B):
    """B distinct witnesses of the golden circuit"""
    program = Program(K6_LINES, 8)
    return Circuit(setup, K6_LINES, 8, [program.fill_variable_assignments({"a": 3 + i, "b": 4, "d": 5}) for i in range(B)])


def chain_circuit(setup, B):
    import bench

    bench.GROUP_ORDER = 2048
    return Circuit(setup, pc.chain_lines(2048), 2048, [bench.witness_for(i) for i in range(B)])


def poseidon_circuit(setup):
    lines = pc.poseidon_program_lines()
    program = Program(lines, 2048)
    return Circuit(setup, lines, 2048, [program.fill_variable_assignments({"L0": 1 + 2 * i, "M0": 2 + 2 * i}) for i in range(2)])


# ------------------------------------------------------------------------------------------ the oracle's fold
def weights(seed, B):
    t = MerlinTranscript(b"plonk-batch-verify")
    t.append_message(b"seed", seed)
    out = []
    for i in range(B):
        c = copy.deepcopy(t)
        c.append_message(b"index", i.to_bytes(8, "little"))
        out.append(int.from_bytes(c.challenge_bytes(b"rho", 16), "little"))
    return out


def terms(ovk, n, proof, public):
    """The issue's term table: scalars of the proof's own points in R, of the fixed points in R, of W_z_1 / W_zw_1 in L."""
    beta, gamma, alpha, zeta, v, u = ovk.compute_challenges(proof)
    a, b, c = proof["a_eval"], proof["b_eval"], proof["c_eval"]
    s1, s2, zw = proof["s1_eval"], proof["s2_eval"], proof["z_shifted_eval"]
    w = root_of_unity(n)
    zn = pow(zeta, n, R_MOD)
    ZH = (zn - 1) % R_MOD
    L0 = ZH * inv(n * (zeta - 1)) % R_MOD
    PI = OPoly([-x for x in public] + [0] * (n - len(public)), OBasis.LAGRANGE).barycentric_eval(zeta)
    r0 = (PI - L0 * alpha * alpha - alpha * (a + beta * s1 + gamma) * (b + beta * s2 + gamma) * (c + gamma) * zw) % R_MOD
    own = {"a_1": v, "b_1": v ** 2, "c_1": v ** 3,
           "z_1": (a + beta * zeta + gamma) * (b + beta * 2 * zeta + gamma) * (c + beta * 3 * zeta + gamma) * alpha + L0 * alpha * alpha + u,
           "t_lo_1": -ZH, "t_mid_1": -ZH * zn, "t_hi_1": -ZH * zn * zn, "W_z_1": zeta, "W_zw_1": u * zeta * w}
    fixed = {"Qm": a * b, "Ql": a, "Qr": b, "Qo": c, "Qc": 1, "S1": v ** 4, "S2": v ** 5,
             "S3": -(a + beta * s1 + gamma) * (b + beta * s2 + gamma) * alpha * beta * zw,
             "G1": r0 - (v * a + v ** 2 * b + v ** 3 * c + v ** 4 * s1 + v ** 5 * s2 + u * zw)}
    return own, fixed, {"W_z_1": 1, "W_zw_1": u}


def oracle_fold(circ, recs, pubs, rhos, lo, hi):
    L, R, fixed_sum = [], [], {}
    for i in range(lo, hi):
        proof = flat_of(recs[i])
        own, fixed, left = terms(circ.ovk, circ.n, proof, pubs[i])
        L += [(proof[k], s * rhos[i] % R_MOD) for k, s in left.items()]
        R += [(proof[k], s * rhos[i] % R_MOD) for k, s in own.items()]
        for k, s in fixed.items():
            fixed_sum[k] = (fixed_sum.get(k, 0) + s * rhos[i]) % R_MOD
    R += [(og1.G1 if k == "G1" else getattr(circ.ovk, k), s) for k, s in fixed_sum.items()]
    return og1.ec_lincomb(L), og1.ec_lincomb(R)


# ------------------------------------------------------------------------------------------ 1. bit-exact folds
def bit_exact_folds(circ, ranges=None, count=None):
    count = len(circ.recs) if count is None else count
    recs, pubs = circ.recs[:count], circ.pubs[:count]
    circ.assert_valid(range(count))
    circ.bv.load(b"".join(recs), pubs, SEED)
    assert circ.bv.status == bytes(count)
    rhos = weights(SEED, count)
    for lo, hi in ranges or [(0, count)]:
        L, R = circ.bv.fold(lo, hi)
        want_L, want_R = oracle_fold(circ, recs, pubs, rhos, lo, hi)
        assert pc.affine(L) == want_L and pc.affine(R) == want_R, (lo, hi)


# ------------------------------------------------------------------------------------------ 2. verdicts agree with the per-proof verifier
def corruptions(rec, pub):
    """the 17 single corruptions: each commitment doubled, W_zw_1 := W_z_1, each evaluation + 1, the first public input + 1"""
    flat = flat_of(rec)
    for k in POINTS:
        yield "2*" + k, record(dict(flat, **{k: og1.double(flat[k])})), pub
    yield "W_zw_1 := W_z_1", record(dict(flat, W_zw_1=flat["W_z_1"])), pub
    for k in EVALS:
        yield k + " + 1", record(dict(flat, **{k: (flat[k] + 1) % R_MOD})), pub
    yield "public[0] + 1", rec, [(pub[0] + 1) % R_MOD] + list(pub[1:])


def verdicts_agree(circ, indices):
    for i in indices:
        rec, pub = circ.recs[i], circ.pubs[i]
        assert circ.accepted_one_by_one(rec, pub)
        assert circ.bv.verify(rec, [pub]) and circ.bv.pairing_checks == 1, i
        n_cases = 0
        for name, bad_rec, bad_pub in corruptions(rec, pub):
            assert not circ.accepted_one_by_one(bad_rec, bad_pub), (i, name)
            assert not circ.bv.verify(bad_rec, [bad_pub]), (i, name)
            assert circ.bv.status == b"\0", (i, name)  # well-formed, and wrong
            n_cases += 1
        assert n_cases == 17


# ------------------------------------------------------------------------------------------ 3. a whole batch
def whole_batch(circ, sample=4):
    B = len(circ.recs)
    circ.assert_valid(random.Random(3).sample(range(B), min(sample, B)))
    bv, bp = circ.bv, circ.prover
    assert bv.verify_prover(bp) and bv.pairing_checks == 1 and bv.status == bytes(B)
    assert bv.verify_prover(bp, seed=SEED)
    fold_a = bv.fold(0, B)
    blob, _ = bp.download_raw()
    assert blob == b"".join(circ.recs)
    assert bv.verify(blob, circ.pubs, seed=SEED) and bv.pairing_checks == 1
    assert bv.fold(0, B) == fold_a  # the same proofs and weights whether they came through the host or not
    blob480, _ = bp.download_compressed()
    assert len(blob480) == 480 * B
    assert bv.verify(blob480, circ.pubs, seed=SEED) and bv.fold(0, B) == fold_a
    assert bv.verify(blob, circ.pubs, seed=bytes(32))  # another seed: other fold points, the same verdict
    assert bv.fold(0, B) != fold_a
    assert circ.vk.verify_batch(blob, circ.pubs)
    with pytest.raises(pa._lib.BackendError):  # as plonk_prover_run: the batch must be the resident one
        bv.verify_prover(bp, B=B - 1 if B > 1 else 2)


# ------------------------------------------------------------------------------------------ 4. localisation
def localisation(circ, bad, max_checks):
    """`bad`: {index: corruption number (0..16 of `corruptions`)}"""
    B = len(circ.recs)
    recs, pubs = list(circ.recs), [list(p) for p in circ.pubs]
    for i, which in bad.items():
        assert circ.accepted_one_by_one(recs[i], pubs[i])
        name, recs[i], pubs[i] = list(corruptions(recs[i], pubs[i]))[which]
        assert not circ.accepted_one_by_one(recs[i], pubs[i]), name
    blob = b"".join(recs)
    assert not circ.bv.verify(blob, pubs)
    got = circ.bv.verify_each(blob, pubs)
    assert got == [i not in bad for i in range(B)]
    assert circ.bv.pairing_checks <= max_checks, circ.bv.pairing_checks
    assert circ.bv.verify_each(b"".join(circ.recs), circ.pubs) == [True] * B and circ.bv.pairing_checks == 1


# ------------------------------------------------------------------------------------------ 5. malformed input is a verdict
def malformed(circ):
    """needs >= 6 proofs; proofs 1..4 are spoilt, 0 and 5 stay honest"""
    recs, pubs = [bytearray(r) for r in circ.recs[:6]], circ.pubs[:6]
    circ.assert_valid(range(6))
    recs[1][64 * 3 : 64 * 3 + 32] = Q_MOD.to_bytes(32, "little")                    # z_1.x = p
    recs[2][576 + 32 : 576 + 64] = (R_MOD + 5).to_bytes(32, "little")                # b_eval >= r
    y = int.from_bytes(recs[3][64 * 4 + 32 : 64 * 5], "little")
    recs[3][64 * 4 + 32 : 64 * 5] = ((y + 1) % Q_MOD).to_bytes(32, "little")         # t_lo_1 off the curve
    recs[4][64 * 8 : 64 * 9] = bytes(64)                                             # W_zw_1 = 64 zero bytes
    blob = b"".join(bytes(r) for r in recs)
    want_status = bytes([0, 1, 1, 2, 4, 0])
    bv = circ.bv
    assert not bv.verify(blob, pubs) and bv.status == want_status
    assert bv.verify_each(blob, pubs) == [True, False, False, False, False, True]
    assert bv.status == want_status and bv.pairing_checks == 1  # the spoilt proofs take part in no fold: the rest passes at once
    # every spoilt proof alone, and a batch of nothing but spoilt proofs
    for i in (1, 2, 3, 4):
        assert not bv.verify(bytes(recs[i]), [pubs[i]]) and bv.status == want_status[i : i + 1]
    assert bv.verify_each(blob[768:768 * 5], pubs[1:5]) == [False] * 4
    # compressed records: flag bits 00 (malformed), and an x whose x^3 + 3 is not a square (off the curve)
    proofs = [BatchProver.decode(bytes(r)) for r in circ.recs[:3]]
    comp = [bytearray(p.to_bytes()) for p in proofs]
    comp[1][32 * 2] &= 0x3F                                                          # c_1: flag bits 00
    x = 1
    while pow((x ** 3 + 3) % Q_MOD, (Q_MOD - 1) // 2, Q_MOD) == 1:
        x += 1
    comp[2][32 * 5 : 32 * 6] = (x | (2 << 254)).to_bytes(32, "big")                  # t_mid_1: no such point
    blob480 = b"".join(bytes(c) for c in comp)
    assert bv.verify_each(blob480, pubs[:3]) == [True, False, False] and bv.status == bytes([0, 1, 2])
    assert not bv.verify(blob480, pubs[:3])
    assert bv.verify(blob480[:480], pubs[:1])


# ------------------------------------------------------------------------------------------ 6. degenerate arithmetic
def degenerate_proofs(circ):
    rec, pub = circ.recs[0], circ.pubs[0]
    circ.assert_valid([0])
    bv = circ.bv
    assert bv.verify(rec * 3, [pub] * 3) and bv.pairing_checks == 1  # the same bases under three weights
    flat = flat_of(rec)
    for name, bad in (("b_1 := a_1", dict(flat, b_1=flat["a_1"])), ("W_zw_1 := -W_z_1", dict(flat, W_zw_1=og1.neg(flat["W_z_1"])))):
        assert not circ.accepted_one_by_one(record(bad), pub), name
        assert not bv.verify(record(bad), [pub]) and bv.status == b"\0", name
        assert bv.verify_each(rec + record(bad) + rec, [pub] * 3) == [True, False, True], name


def g1_mul_many(points, scalars):
    ctx = pa.get_context()
    n = len(points)
    xy = b"".join(bytes(64) if p is None else int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little") for p in points)
    ks = b"".join(int(k).to_bytes(32, "little") for k in scalars)
    out, fl = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    pa._lib.check(ctx.L.plonk_g1_mul_many(ctx.handle, xy, ks, n, out, fl))
    raw = out.raw
    return [None if fl.raw[i] else (int.from_bytes(raw[64 * i : 64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32 : 64 * i + 64], "little"))
            for i in range(n)]


EDGE_SCALARS = (0, 1, 2, R_MOD - 1, R_MOD - 2, 1 << 128, 1 << 253)


def mul_many_cases(counts, big_count):
    """Counts in `counts`: every product against oracle.g1.multiply.  `big_count` products: the edge entries and a seeded sample
    against oracle.g1.multiply, and EVERY entry through a random linear combination under the oracle's C group law —
    sum_j c_j out_j == sum_j (c_j k_j) P_j with 64-bit c_j (a wrong entry survives with probability 2^-64); oracle.g1.multiply on
    all of them would take Python tens of minutes."""
    rng = random.Random(77)
    pool = [og1.G1, None] + [c_oracle.g1_lincomb([og1.G1], [rng.randrange(1, R_MOD)]) for _ in range(61)]

    def inputs(n):
        pts = [pool[j % len(pool)] for j in range(n)]
        ks = [EDGE_SCALARS[(j // 3) % len(EDGE_SCALARS)] if j % 2 == 0 else rng.randrange(R_MOD) for j in range(n)]
        return pts, ks

    # the edge scalars on G1, the identity and a random point
    pts = [p for p in (og1.G1, None, pool[2]) for _ in EDGE_SCALARS]
    ks = list(EDGE_SCALARS) * 3
    assert g1_mul_many(pts, ks) == [og1.multiply(p, k) for p, k in zip(pts, ks)]
    for n in counts:
        pts, ks = inputs(n)
        assert g1_mul_many(pts, ks) == [og1.multiply(p, k) for p, k in zip(pts, ks)], n
    pts, ks = inputs(big_count)
    got = g1_mul_many(pts, ks)
    for j in list(range(24)) + rng.sample(range(big_count), 24):
        assert got[j] == og1.multiply(pts[j], ks[j]), j
    cs = [rng.getrandbits(64) for _ in range(big_count)]
    assert c_oracle.g1_lincomb(got, cs) == c_oracle.g1_lincomb(pts, [c * k % R_MOD for c, k in zip(cs, ks)])
    with pytest.raises(AssertionError):
        g1_mul_many([(1, 3)], [1])  # not on the curve
    with pytest.raises(AssertionError):
        g1_mul_many([og1.G1], [R_MOD])


# ------------------------------------------------------------------------------------------ 7. arguments
def arguments(circ):
    bv, rec, pub = circ.bv, circ.recs[0], circ.pubs[0]
    bv.load(rec * 2, [pub, pub], SEED)
    for lo, hi in ((2, 1), (0, 3), (3, 3)):
        with pytest.raises(AssertionError):
            bv.fold(lo, hi)
    assert bv.fold(1, 1) == (None, None)  # an empty range
    with pytest.raises(AssertionError):
        bv.verify(rec, [list(pub) + [1]])  # a row of the wrong length
    with pytest.raises(AssertionError):
        bv.verify(rec, [[R_MOD] + list(pub[1:])])  # a public input not below r
    with pytest.raises(AssertionError):
        bv.verify(rec[:-1], [pub])
    assert circ.prover is not None
    with pytest.raises(pa._lib.BackendError):
        bv.verify_prover(circ.prover, B=len(circ.recs) + 1)
    other = BatchVerifier(circ.vk, len(pub) + 1)
    with pytest.raises(AssertionError):
        other.verify_prover(circ.prover)  # another circuit shape than the prover's
    assert bv.verify(rec, [pub])
