"""Bodies of the tests of zero-knowledge blinding in the lock-step prover (csrc/prover_blind.h, PLONK_PROVER_BLINDING; batch.py:
BatchProver(blinding=...), set_blinders), shared by tests/test_emu_blinding.py (emulated kernels) and tests/test_gpu_blinding.py
(MI355X).

The expected values come from `Model`, a CPU prover of the blinded protocol (PLONK paper, section 8.3, blinders b1..b11) written
over oracle/ alone: polynomials are plain coefficient lists, products are naive, the quotient is a long division by X^n - 1, the
openings long divisions by a linear factor, and every commitment is one linear combination of setup.powers_of_x.  It never splits
a polynomial into p0 + q Z_H and uses no coset: what it shares with the device code is the protocol, not the method.
`model_is_the_oracle` first shows that with zero blinders it is oracle.plonk_prover.Prover in all 15 fields, and that its blinded
proofs pass oracle.verifier while a tampered one does not."""
import random

import pytest

import plonkathon_amd as pa
from helpers import R_MOD
from oracle import c_oracle
from oracle.circuit import Program as OProgram
from oracle.field import inv, root_of_unity, roots_of_unity
from oracle.fr_poly import Basis, Polynomial
from oracle.plonk_prover import Prover as OProver
from oracle.srs import Setup as OSetup
from oracle.strobe_merlin import MerlinTranscript, Transcript
from oracle.verifier import VerificationKey as OVerificationKey
from parity_cases import FACTORIZATION, FACTORIZATION_START, PTAU, chain_lines, flat

ERR_ARG, ERR_STATE = -1, -4
BLINDING = 1 << 20  # PLONK_PROVER_BLINDING
POINTS = ("a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "W_z_1", "W_zw_1")
EVALS = ("a_eval", "b_eval", "c_eval", "s1_eval", "s2_eval", "z_shifted_eval")
K6_LINES = ["e public", "c <== a * b", "e <== c * d"]
SEED = bytes(range(7, 39))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def p_add(a, b):
    m = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % R_MOD for i in range(m)]


def p_scale(a, k):
    return [x * k % R_MOD for x in a]


def p_sub(a, b):
    return p_add(a, p_scale(b, R_MOD - 1))


def p_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R_MOD
    return out


def p_eval(a, x):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % R_MOD
    return acc


def p_trim(a):
    a = list(a)
    while len(a) > 1 and a[-1] == 0:
        a.pop()
    return a


def p_div_zh(a, n):
    """a / (X^n - 1); the division must be exact."""
    a, q = list(a), [0] * max(len(a) - n, 1)
    for i in range(len(a) - 1, n - 1, -1):
        q[i - n] = a[i]
        a[i - n] = (a[i - n] + a[i]) % R_MOD
        a[i] = 0
    assert not any(a), "the quotient's numerator is not divisible by Z_H"
    return q


def p_div_linear(a, x0):
    """a / (X - x0); the division must be exact."""
    q, carry = [0] * (len(a) - 1), 0
    for i in range(len(a) - 1, 0, -1):
        carry = (a[i] + carry * x0) % R_MOD
        q[i - 1] = carry
    assert (a[0] + carry * x0) % R_MOD == 0, "the opening's numerator does not vanish at the point"
    return q


def wire_columns(oprog, witness):
    """The A, B, C columns of round 1 (prover.py:94-103): witness[None] = 0, zero padded to the group order."""
    witness = dict(witness)
    witness.setdefault(None, 0)
    cols = [[0] * oprog.group_order for _ in range(3)]
    for i, cells in enumerate(oprog.wires()):
        for k in range(3):
            cols[k][i] = witness[cells[k]] % R_MOD
    return cols


class Model:
    """The blinded prover on the CPU.  prove(witness, blinders) -> the flat proof; .polys keeps a, b, c, z, t_lo, t_mid, t_hi."""

    def __init__(self, osetup, oprog):
        self.setup, self.program, self.n = osetup, oprog, oprog.group_order
        pk = oprog.common_preprocessed_input()
        self.lag = {k: getattr(pk, k).values for k in ("QM", "QL", "QR", "QO", "QC", "S1", "S2", "S3")}
        self.fixed = {k: Polynomial(v, Basis.LAGRANGE).ifft().values for k, v in self.lag.items()}

    def commit(self, coeffs):
        coeffs = p_trim(coeffs)
        assert len(coeffs) <= len(self.setup.powers_of_x)
        return c_oracle.g1_lincomb(self.setup.powers_of_x[:len(coeffs)], coeffs)

    def prove(self, witness, blinders):
        n, f, b = self.n, self.fixed, [int(x) % R_MOD for x in blinders]
        assert len(b) == 11
        w, roots = root_of_unity(n), roots_of_unity(n)
        zh = [R_MOD - 1] + [0] * (n - 1) + [1]
        coef = lambda vals: Polynomial(vals, Basis.LAGRANGE).ifft().values
        cols = wire_columns(self.program, witness)
        public = [witness[v] for v in self.program.get_public_assignments()]
        PI = coef([-x for x in public] + [0] * (n - len(public)))
        t = Transcript(b"plonk")
        # round 1
        A, B, C = (p_add(coef(cols[k]), p_mul([b[2 * k + 1], b[2 * k]], zh)) for k in range(3))
        a_1, b_1, c_1 = self.commit(A), self.commit(B), self.commit(C)
        beta, gamma = t.round_1(a_1, b_1, c_1)
        # round 2
        rlc = lambda x, y: (x + beta * y + gamma) % R_MOD
        Zv = [1]
        for i in range(n):
            num = rlc(cols[0][i], roots[i]) * rlc(cols[1][i], 2 * roots[i]) * rlc(cols[2][i], 3 * roots[i]) % R_MOD
            den = rlc(cols[0][i], self.lag["S1"][i]) * rlc(cols[1][i], self.lag["S2"][i]) * rlc(cols[2][i], self.lag["S3"][i]) % R_MOD
            Zv.append(Zv[-1] * num % R_MOD * inv(den) % R_MOD)
        assert Zv.pop() == 1
        self.z0_values = list(Zv)
        Z = p_add(coef(Zv), p_mul([b[8], b[7], b[6]], zh))
        z_1 = self.commit(Z)
        alpha, _cof = t.round_2(z_1)
        # round 3
        Zw = [c * pow(w, i, R_MOD) % R_MOD for i, c in enumerate(Z)]
        lin = lambda p, k, s: p_add(p_add(p, p_scale(s, beta * k % R_MOD)), [gamma])
        X = [0, 1]
        gate = p_add(p_add(p_add(p_mul(A, f["QL"]), p_mul(B, f["QR"])), p_add(p_mul(p_mul(A, B), f["QM"]), p_mul(C, f["QO"]))), p_add(PI, f["QC"]))
        perm = p_sub(p_mul(p_mul(p_mul(lin(A, 1, X), lin(B, 2, X)), lin(C, 3, X)), Z),
                     p_mul(p_mul(p_mul(lin(A, 1, f["S1"]), lin(B, 1, f["S2"])), lin(C, 1, f["S3"])), Zw))
        L0 = [inv(n)] * n
        first = p_mul(p_sub(Z, [1]), L0)
        T = p_div_zh(p_add(gate, p_add(p_scale(perm, alpha), p_scale(first, alpha * alpha % R_MOD))), n)
        T = p_trim(T) + [0] * (3 * n + 6)
        assert not any(T[3 * n + 6:])
        self.t_coeffs = T[:3 * n + 6]
        t_lo = T[:n] + [b[9]]
        t_mid = p_add(T[n:2 * n] + [b[10]], [R_MOD - b[9]])
        t_hi = p_add(T[2 * n:3 * n + 6], [R_MOD - b[10]])
        t_lo_1, t_mid_1, t_hi_1 = self.commit(t_lo), self.commit(t_mid), self.commit(t_hi)
        zeta = t.round_3(t_lo_1, t_mid_1, t_hi_1)
        # round 4
        a, bb, c = p_eval(A, zeta), p_eval(B, zeta), p_eval(C, zeta)
        s1, s2, zw = p_eval(f["S1"], zeta), p_eval(f["S2"], zeta), p_eval(Z, zeta * w % R_MOD)
        v = t.round_4(a, bb, c, s1, s2, zw)
        # round 5
        zn = pow(zeta, n, R_MOD)
        zh_ev = (zn - 1) % R_MOD
        l0_ev = zh_ev * inv(n * (zeta - 1)) % R_MOD
        k1 = rlc(a, zeta) * rlc(bb, 2 * zeta) * rlc(c, 3 * zeta) % R_MOD
        k2 = rlc(a, s1) * rlc(bb, s2) * zw % R_MOD
        R = p_add(p_add(p_scale(f["QM"], a * bb % R_MOD), p_scale(f["QL"], a)), p_add(p_scale(f["QR"], bb), p_scale(f["QO"], c)))
        R = p_add(R, p_add([p_eval(PI, zeta)], f["QC"]))
        R = p_add(R, p_scale(p_sub(p_scale(Z, k1), p_scale(p_add(p_scale(f["S3"], beta), [(c + gamma) % R_MOD]), k2)), alpha))
        R = p_add(R, p_scale(p_sub(Z, [1]), l0_ev * alpha * alpha % R_MOD))
        R = p_sub(R, p_scale(p_add(t_lo, p_add(p_scale(t_mid, zn), p_scale(t_hi, zn * zn % R_MOD))), zh_ev))
        num = R
        for k, (poly, ev) in enumerate(((A, a), (B, bb), (C, c), (f["S1"], s1), (f["S2"], s2))):
            num = p_add(num, p_scale(p_sub(poly, [ev]), pow(v, k + 1, R_MOD)))
        W_z = p_div_linear(num, zeta)
        W_zw = p_div_linear(p_sub(Z, [zw]), zeta * w % R_MOD)
        self.polys = {"a": A, "b": B, "c": C, "z": Z, "t_lo": t_lo, "t_mid": t_mid, "t_hi": t_hi, "W_z": W_z, "W_zw": W_zw}
        self.challenges = {"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "v": v}
        return {"a_1": a_1, "b_1": b_1, "c_1": c_1, "z_1": z_1, "t_lo_1": t_lo_1, "t_mid_1": t_mid_1, "t_hi_1": t_hi_1,
                "a_eval": a, "b_eval": bb, "c_eval": c, "s1_eval": s1, "s2_eval": s2, "z_shifted_eval": zw,
                "W_z_1": self.commit(W_z), "W_zw_1": self.commit(W_zw)}


def derive_blinders(seed, run, index):
    """What plonk_prover_seed_blinders makes the device draw for proof `index` of blinded run number `run`."""
    t = MerlinTranscript(b"plonk-blinding")
    t.append_message(b"seed", seed)
    t.append_message(b"run", run.to_bytes(8, "little"))
    t.append_message(b"index", index.to_bytes(8, "little"))
    return [int.from_bytes(t.challenge_bytes(b"b", 255), "big") % R_MOD for _ in range(11)]


# ---- circuits ----------------------------------------------------------------------------------------------------------------------
class Circuit:
    def __init__(self, lines, n, starts):
        self.lines, self.n = lines, n
        self.program, self.oprog = pa.Program(lines, n), OProgram(lines, n)
        self.wits = [self.oprog.fill_variable_assignments(dict(s)) for s in starts]
        self.public_vars = self.oprog.get_public_assignments()

    def publics(self, i):
        return [self.wits[i][v] % R_MOD for v in self.public_vars]


def circuit(shared, name):
    """"golden": the reference's K6 circuit at n = 8; "factorisation": n = 16; both with three witnesses."""
    if ("circuit", name) not in shared:
        if name == "golden":
            c = Circuit(K6_LINES, 8, [{"a": 3 + i, "b": 4, "d": 5 + 2 * i} for i in range(3)])
        elif name == "factorisation":
            bits = lambda p, q: dict({"pb%d" % k: p >> k & 1 for k in range(4)}, **{"qb%d" % k: q >> k & 1 for k in range(4)})
            c = Circuit(FACTORIZATION, 16, [dict(FACTORIZATION_START), bits(3, 5), bits(15, 15)])
        else:
            n = int(name[5:])
            c = Circuit(chain_lines(n), n, [{"x0": 3 + 1000003 * i} for i in range(4)])
        shared[("circuit", name)] = c
    return shared[("circuit", name)]


def osetup(shared):
    if "osetup" not in shared:
        shared["osetup"] = OSetup.from_file(PTAU)
    return shared["osetup"]


def model(shared, name):
    if ("model", name) not in shared:
        c = circuit(shared, name)
        shared[("model", name)] = Model(osetup(shared), c.oprog)
    return shared[("model", name)]


def ovk_of(shared, name, setup_o=None):
    if ("ovk", name) not in shared:
        c = circuit(shared, name)
        shared[("ovk", name)] = OVerificationKey.from_setup(setup_o or osetup(shared), c.oprog.common_preprocessed_input())
    return shared[("ovk", name)]


def fixed_blinders(seed, rows):
    rng = random.Random(seed)
    return [[rng.randrange(R_MOD) for _ in range(11)] for _ in range(rows)]


def records(bp, B):
    raw, st = bp.download_raw()
    assert len(raw) == 768 * B and len(st) == B
    return [raw[768 * i:768 * (i + 1)] for i in range(B)], st


def flat_record(rec):
    return flat(pa.BatchProver.decode(rec))


# ---- 0. the model is a prover ------------------------------------------------------------------------------------------------------
def model_is_the_oracle(shared, name):
    """Zero blinders: the oracle prover's 15 fields.  Random blinders: another proof in all nine points and in a, b, c, z_shifted,
    accepted by the oracle's verifier, rejected with a_eval raised by one; the quotient has exactly 3n + 6 coefficients."""
    c, m, ovk = circuit(shared, name), model(shared, name), ovk_of(shared, name)
    want = OProver(osetup(shared), c.oprog).prove(dict(c.wits[0])).flatten()
    plain = m.prove(c.wits[0], [0] * 11)
    assert plain == want
    assert not any(m.t_coeffs[3 * c.n:])
    blinded = m.prove(c.wits[0], fixed_blinders(name, 1)[0])
    assert len(m.t_coeffs) == 3 * c.n + 6 and m.t_coeffs[-1] != 0 and len(p_trim(m.polys["W_z"])) == c.n + 5
    assert all(blinded[k] != plain[k] for k in POINTS + ("a_eval", "b_eval", "c_eval", "z_shifted_eval"))
    assert blinded["s1_eval"] != plain["s1_eval"]  # another zeta
    assert ovk.verify_proof(c.n, blinded, c.publics(0))
    assert not ovk.verify_proof(c.n, dict(blinded, a_eval=(blinded["a_eval"] + 1) % R_MOD), c.publics(0))


# ---- 1. zero blinders are today's bytes ------------------------------------------------------------------------------------------
def zero_blinders_are_unblinded_bytes(setup, shared, name, **kw):
    """Blinding on with all-zero blinders: the four-coset quotient, the fold and every correction leave the unblinded prover's
    768-byte records."""
    c = circuit(shared, name)
    B = len(c.wits)
    plain = pa.BatchProver(setup, c.program, **kw)
    plain.upload([dict(w) for w in c.wits])
    plain.run()
    want, st = records(plain, B)
    assert st == bytes(B)
    bp = pa.BatchProver(setup, c.program, blinding=SEED, **kw)
    bp.upload([dict(w) for w in c.wits])
    bp.set_blinders([[0] * 11] * B)
    bp.run()
    got, st = records(bp, B)
    assert st == bytes(B)
    assert got == want


# ---- 2. bit-exact against the model -----------------------------------------------------------------------------------------------
def blinder_rows(name):
    """Three rows: random; every blinder r - 1; random with the two t-split blinders (b9, b10) zero."""
    rows = fixed_blinders("rows " + name, 3)
    rows[1] = [R_MOD - 1] * 11
    rows[2][9] = rows[2][10] = 0
    return rows


def model_proofs(shared, name):
    if ("model proofs", name) not in shared:
        c, m = circuit(shared, name), model(shared, name)
        shared[("model proofs", name)] = [m.prove(c.wits[i], row) for i, row in enumerate(blinder_rows(name))]
    return shared[("model proofs", name)]


def bit_exact_against_the_model(setup, shared, name, lagrange_commits):
    c = circuit(shared, name)
    want = model_proofs(shared, name)
    bp = pa.BatchProver(setup, c.program, blinding=SEED, lagrange_commits=lagrange_commits)
    bp.upload([dict(w) for w in c.wits[:3]])
    bp.set_blinders(blinder_rows(name))
    bp.run()
    got, st = records(bp, 3)
    assert st == bytes(3), list(st)
    for i in range(3):
        g = flat_record(got[i])
        for k in POINTS + EVALS:
            assert g[k] == want[i][k], (name, lagrange_commits, i, k)
        assert ovk_of(shared, name).verify_proof(c.n, g, c.publics(i))


def seeded_against_the_model(setup, shared, name):
    """Under a seed the device draws derive_blinders(seed, run, index): proofs 0 and B - 1 of runs 0 and 1 are the model's under
    those, and the two runs of one witness differ in all 15 fields."""
    c, m = circuit(shared, name), model(shared, name)
    B = len(c.wits)
    bp = pa.BatchProver(setup, c.program, blinding=SEED)
    runs = []
    for run in range(2):
        got = [flat(p) for p in bp.prove_batch([dict(w) for w in c.wits])]
        for i in (0, B - 1):
            assert got[i] == m.prove(c.wits[i], derive_blinders(SEED, run, i)), (name, run, i)
        runs.append(got)
    # s1_eval and s2_eval are evaluations of fixed polynomials at another zeta
    assert all(runs[0][i][k] != runs[1][i][k] for i in range(B) for k in POINTS + EVALS)


# ---- 3. acceptance and hiding at size -----------------------------------------------------------------------------------------------
def accepted_and_hidden_at_size(setup, lines, n, starts, seed=SEED):
    """n = 2^10 under a seed, B = len(starts): every proof passes vk.verify_proof and the batch verifier; for proofs 0 and B - 1,
    a_1, b_1, c_1, z_1 are commit(p0) + sum_k q_k H_k and the six evaluations the closed forms, with the tails from
    derive_blinders; a second run of the same witnesses differs in all 15 fields."""
    osrs = OSetup.from_file(PTAU)
    program, oprog = pa.Program(lines, n), OProgram(lines, n)
    wits = [oprog.fill_variable_assignments(dict(s)) for s in starts]
    B = len(wits)
    public_vars = oprog.get_public_assignments()
    pubs = [[w[v] % R_MOD for v in public_vars] for w in wits]
    vk = setup.verification_key(program.common_preprocessed_input())
    bp = pa.BatchProver(setup, program, blinding=seed)
    bv = pa.BatchVerifier(vk, len(public_vars))
    runs = []
    for run in range(2):
        proofs = bp.prove_batch([dict(w) for w in wits])
        assert bv.verify_prover(bp), run  # load_prover + the fold's one pairing check
        for i, p in enumerate(proofs):
            assert run or vk.verify_proof(n, p, pubs[i]), (run, i)  # (one pairing check on the host per proof: the first run's)
        runs.append([flat(p) for p in proofs])
    assert all(runs[0][i][k] != runs[1][i][k] for i in range(B) for k in POINTS + EVALS)
    pk = oprog.common_preprocessed_input()
    w, roots = root_of_unity(n), roots_of_unity(n)
    H = [c_oracle.g1_lincomb([osrs.powers_of_x[n + k], osrs.powers_of_x[k]], [1, R_MOD - 1]) for k in range(6)]
    for i in (0, B - 1):
        b, g = derive_blinders(seed, 0, i), runs[0][i]
        cols = wire_columns(oprog, wits[i])
        tails = [[b[1], b[0]], [b[3], b[2]], [b[5], b[4]], [b[8], b[7], b[6]]]
        commit0 = lambda p0: c_oracle.g1_lincomb(osrs.powers_of_x[:n], Polynomial(p0, Basis.LAGRANGE).ifft().values)  # oracle.srs.Setup.commit's points
        blind = lambda p0, q: c_oracle.g1_lincomb([commit0(p0)] + H[:len(q)], [1] + q)
        for k, key in enumerate(("a_1", "b_1", "c_1")):
            assert g[key] == blind(cols[k], tails[k]), (i, key)
        t = Transcript(b"plonk")
        beta, gamma = t.round_1(g["a_1"], g["b_1"], g["c_1"])
        rlc = lambda x, y: (x + beta * y + gamma) % R_MOD
        Zv = [1]
        for j in range(n - 1):
            num = rlc(cols[0][j], roots[j]) * rlc(cols[1][j], 2 * roots[j]) * rlc(cols[2][j], 3 * roots[j]) % R_MOD
            den = rlc(cols[0][j], pk.S1.values[j]) * rlc(cols[1][j], pk.S2.values[j]) * rlc(cols[2][j], pk.S3.values[j]) % R_MOD
            Zv.append(Zv[-1] * num % R_MOD * inv(den) % R_MOD)
        assert g["z_1"] == blind(Zv, tails[3]), i
        t.round_2(g["z_1"])
        zeta = t.round_3(g["t_lo_1"], g["t_mid_1"], g["t_hi_1"])
        zh = (pow(zeta, n, R_MOD) - 1) % R_MOD
        ev = lambda vals, x: Polynomial(vals, Basis.LAGRANGE).barycentric_eval(x)
        for k, key in enumerate(("a_eval", "b_eval", "c_eval")):
            assert g[key] == (ev(cols[k], zeta) + p_eval(tails[k], zeta) * zh) % R_MOD, (i, key)
        assert g["s1_eval"] == pk.S1.barycentric_eval(zeta) and g["s2_eval"] == pk.S2.barycentric_eval(zeta)
        zw = zeta * w % R_MOD
        assert g["z_shifted_eval"] == (ev(Zv, zw) + p_eval(tails[3], zw) * zh) % R_MOD, i


# ---- 4. segmented scans -------------------------------------------------------------------------------------------------------------
def segmented_scans_same_bytes(setup, n, segments, vk_check=None, B=1):
    """The chain circuit at n under one seed with the scans forced to each S of `segments`: identical records, status 0."""
    program = pa.Program(chain_lines(n), n)
    wits = [program.fill_variable_assignments({"x0": 3 + 5 * i}) for i in range(B)]
    seen = []
    for S in segments:
        bp = pa.BatchProver(setup, program, blinding=SEED, segments=S)
        bp.upload([dict(w) for w in wits])
        bp.run()
        got, st = records(bp, B)
        assert st == bytes(B), (S, list(st))
        seen.append(got)
        if vk_check is not None and S == segments[0]:
            vk_check(program, wits, bp.download())
    assert all(s == seen[0] for s in seen[1:])
    return seen[0]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def refusals(setup, shared):
    c = circuit(shared, "golden")
    # n = 4
    small = pa.Program(["c <== a * b"], 4)
    bp4 = pa.BatchProver(setup, small)
    L = bp4.ctx.L
    assert L.plonk_prover_set_options(bp4._h, BLINDING) == ERR_ARG
    assert b"group_order 4 is below 8" in L.plonk_last_error()
    with pytest.raises(AssertionError, match="group_order 4 is below 8"):
        pa.BatchProver(setup, small, blinding=True)
    # an SRS of exactly n powers
    exact = pa.Setup(powers_of_x=list(setup.powers_of_x[:8]), X2=setup.X2)
    bp8 = pa.BatchProver(exact, c.program)
    assert L.plonk_prover_set_options(bp8._h, BLINDING) == ERR_ARG
    assert b"group_order 8 needs 14 powers of tau, the SRS has 8" in L.plonk_last_error()
    assert L.plonk_prover_set_options(bp8._h, 0) == 0
    assert bp8.prove(dict(c.wits[0])) is not None  # still an unblinded prover
    # run without blinders
    bp = pa.BatchProver(setup, c.program)
    assert L.plonk_prover_set_options(bp._h, BLINDING) == 0
    bp.upload([dict(c.wits[0])])
    assert L.plonk_prover_run(bp._h, 1) == ERR_STATE
    assert b"batch 1 is to be blinded, but neither plonk_prover_set_blinders nor plonk_prover_seed_blinders" in L.plonk_last_error()
    # a blinder equal to r
    row = [5] * 11
    row[7] = R_MOD
    blob = b"".join(v.to_bytes(32, "little") for v in [1] * 11 + row)
    assert L.plonk_prover_set_blinders(bp._h, blob, 2) == ERR_ARG
    assert b"blinder 7 of proof 1 is not below r" in L.plonk_last_error()
    assert L.plonk_prover_run(bp._h, 1) == ERR_STATE  # nothing was set
    # a blinder blob of the wrong batch
    bp.set_blinders([[1] * 11, [2] * 11])
    assert L.plonk_prover_run(bp._h, 1) == ERR_STATE
    assert b"batch 1, but the blinders were set for a batch of 2" in L.plonk_last_error()
    with pytest.raises(ValueError):
        bp.set_blinders(bytes(32 * 11 + 1))
    with pytest.raises(ValueError):
        bp.set_blinders([[1] * 10])
    with pytest.raises(ValueError):
        pa.BatchProver(setup, c.program, blinding=bytes(31))
    assert L.plonk_prover_set_blinders(bp._h, None, 1) == ERR_ARG and L.plonk_prover_seed_blinders(bp._h, None) == ERR_ARG
    # the right batch proves, once: explicit blinders serve one run
    bp.set_blinders([[1] * 11])
    bp.run()
    assert bp.download_raw()[1] == bytes(1)
    assert L.plonk_prover_run(bp._h, 1) == ERR_STATE


# ---- 6. failure bits survive -----------------------------------------------------------------------------------------------------
def failure_bits_survive(setup, shared):
    """Proof 0 honest, proof 1 breaks a gate (c != a b), proof 2 breaks a copy constraint (the two cells of c differ, each row's
    gate satisfied): status 0, 4, 2 — blinded as unblinded."""
    c = circuit(shared, "golden")
    good = c.wits[0]
    for blinding in (False, SEED):
        bp = pa.BatchProver(setup, c.program, blinding=blinding)
        cols = [bp.wire_columns(good) for _ in range(3)]
        rows = [tuple(cells) for cells in c.oprog.wires()]
        mul, out = rows.index(("a", "b", "c")), rows.index(("c", "d", "e"))
        cols[1][2][mul] = (cols[1][2][mul] + 1) % R_MOD  # c <== a * b: its output is no longer a b
        # e <== c * d: another c in this row alone, with e = c' d there so that every gate holds
        cprime = (cols[2][0][out] + 1) % R_MOD
        cols[2][0][out] = cprime
        cols[2][2][out] = cprime * cols[2][1][out] % R_MOD
        le = lambda v: b"".join(int(x).to_bytes(32, "little") for x in v)
        abc = b"".join(le(cols[b][k]) for k in range(3) for b in range(3))
        pub = b"".join(le(c.publics(0)) for _ in range(3))
        bp.upload_raw(abc, pub, 3)
        bp.run()
        st = bp.download_raw()[1]
        assert st[0] == 0 and st[1] & 4 and st[2] == 2, (blinding, list(st))
        if not blinding:
            plain = st
        else:
            assert st == plain


# ---- 7. two-slot intake ----------------------------------------------------------------------------------------------------------
def stream_equals_unpipelined(setup, shared, n=32, sizes=(2, 3, 1), verify_up_to=3):
    """prove_inputs_stream over three batches under a seed: batch k's proofs are those of an unpipelined prover with the same
    seed in its k-th run, and every proof verifies."""
    c = circuit(shared, "chain%d" % n)
    starts = lambda k, B: [{"x0": 3 + 1000003 * b + 7919 * k} for b in range(B)]
    plain = pa.BatchProver(setup, c.program, blinding=SEED)
    want = [[flat(p) for p in plain.prove_inputs(starts(k, B))] for k, B in enumerate(sizes)]
    bp = pa.BatchProver(setup, c.program, blinding=SEED)
    vk = setup.verification_key(c.program.common_preprocessed_input())
    seen = 0
    for k, proofs in enumerate(bp.prove_inputs_stream(starts(k, B) for k, B in enumerate(sizes))):
        assert [flat(p) for p in proofs] == want[k], k
        for b, p in enumerate(proofs[:verify_up_to]):
            assert vk.verify_proof(n, p, [starts(k, sizes[k])[b]["x0"]]), (k, b)
        assert pa.BatchVerifier(vk, 1).verify_prover(bp), k
        seen += 1
    assert seen == len(sizes)
    assert want[0][0] != want[1][0]
