"""Bodies of the tests of round 4's evaluations (csrc/prover_scans.h: eval_chunk_sums walks a lane's rows in three passes and adds
the lanes' values up inside each wave, then across the four waves), shared by tests/test_emu_eval_passes.py (emulated kernels,
fpl.h's range assertions on) and tests/test_gpu_eval_passes.py (MI355X).

Shapes.  The chain circuit at the group orders where the reduction can go wrong: 2^4 (fewer rows than one wave: lanes 16..255 are
empty), 2^6 (exactly one wave holds rows, three contribute zeros), 2^8 (one row per lane), 2^9 (two rows per lane: the chunk
power x^(chunk start) matters), 2^11 (eight rows per lane; GPU only).  Each in the one-workgroup form (S = 1) and with the scans
forced into S segments (PLONK_PROVER_SEGMENTS_MASK), among them at every order that allows it the S that leaves a segment 16 rows,
fewer than lanes.  At 2^4 the library refuses every S > 1 (a segment holds at least 16 rows): that refusal is asserted instead.

References.  Up to 2^8 the oracle prover's proof of the same witness.  At every order, for each of three distinct witnesses, the
six evaluations of the record against Horner evaluations in Python integers at the proof's own zeta (plonk_prover_challenges), of
polynomials rebuilt from the witness through oracle/fr_poly.py — independent of both device forms.  At 2^9 and 2^11 every proof
also passes the pairing check."""
import pytest

import blinding_cases as bc
import parity_cases as pc
import plonkathon_amd as pa
from helpers import R_MOD
from oracle.circuit import Program as OProgram
from oracle.field import inv, root_of_unity, roots_of_unity
from oracle.fr_poly import Basis, Polynomial
from oracle.plonk_prover import Prover as OProver

X0S = (3, 77, R_MOD - 2)  # three distinct witnesses; x0 = 3 is the one the oracle's cached proofs cover
EVALS = ("a_eval", "b_eval", "c_eval", "s1_eval", "s2_eval", "z_shifted_eval")
# n -> the segment counts: L = n / S rows per segment.  64: L = 32, 16.  256: L = 128 (two waves hold rows), 16.  512: L = 256 (one
# row per lane, the chunk starts differ by segment), 16.  2048: L = 1024 (four rows per lane), 16.
SEGMENTS = {16: (1,), 64: (1, 2, 4), 256: (1, 2, 16), 512: (1, 2, 32), 2048: (1, 2, 128)}
EMU_ORDERS = (16, 64, 256, 512)
GPU_ORDERS = EMU_ORDERS + (2048,)
ORACLE_UP_TO = 256


def cases(orders):
    return [(n, S) for n in orders for S in SEGMENTS[n]]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R_MOD
    return acc


def chain(shared, n):
    """The chain circuit at n, once: the product's and the oracle's program, the three witnesses, the coefficient forms of S1, S2."""
    if ("chain", n) not in shared:
        lines = pc.chain_lines(n)
        program, oprog = pa.Program(lines, n), OProgram(lines, n)
        wits = [oprog.fill_variable_assignments({"x0": x0}) for x0 in X0S]
        pk = oprog.common_preprocessed_input()
        coef = lambda vals: Polynomial(list(vals), Basis.LAGRANGE).ifft().values
        shared[("chain", n)] = {"program": program, "oprog": oprog, "wits": wits, "pk": pk, "sigma": [pk.S1.values, pk.S2.values, pk.S3.values],
                                "s1": coef(pk.S1.values), "s2": coef(pk.S2.values)}
    return shared[("chain", n)]


def verification_key(setup, shared, n):
    """The chain circuit's verification key with its eight commitments from the C oracle's group arithmetic (the device commits
    none of them), for the product's pairing check."""
    if ("vk", n) not in shared:
        from oracle import c_oracle
        from plonkathon_amd.field import Fq

        c, powers = chain(shared, n), bc.osetup(shared).powers_of_x[:n]
        coef = lambda vals: Polynomial(list(vals), Basis.LAGRANGE).ifft().values
        pts = [c_oracle.g1_lincomb(powers, coef(getattr(c["pk"], k).values)) for k in ("QM", "QL", "QR", "QO", "QC", "S1", "S2", "S3")]
        fq = lambda p: None if p is None else (Fq(p[0]), Fq(p[1]))
        shared[("vk", n)] = pa.VerificationKey(n, *[fq(p) for p in pts], setup.X2, pa.Scalar.root_of_unity(n))
    return shared[("vk", n)]


def expected_evals(shared, n, i, beta, gamma, zeta):
    """The six evaluations of witness i's proof under these challenges, in Python integers: A, B, C, S1, S2 at zeta, Z at zeta w."""
    key = ("evals", n, i, beta, gamma, zeta)
    if key not in shared:
        c = chain(shared, n)
        cols = bc.wire_columns(c["oprog"], c["wits"][i])
        coef = lambda vals: Polynomial(list(vals), Basis.LAGRANGE).ifft().values
        roots, sig = roots_of_unity(n), c["sigma"]
        rlc = lambda x, y: (x + beta * y + gamma) % R_MOD
        Z = [1]
        for j in range(n - 1):
            num = rlc(cols[0][j], roots[j]) * rlc(cols[1][j], 2 * roots[j]) * rlc(cols[2][j], 3 * roots[j]) % R_MOD
            den = rlc(cols[0][j], sig[0][j]) * rlc(cols[1][j], sig[1][j]) * rlc(cols[2][j], sig[2][j]) % R_MOD
            Z.append(Z[-1] * num % R_MOD * inv(den) % R_MOD)
        want = [horner(coef(cols[k]), zeta) for k in range(3)] + [horner(c["s1"], zeta), horner(c["s2"], zeta)]
        want.append(horner(coef(Z), zeta * root_of_unity(n) % R_MOD))
        shared[key] = dict(zip(EVALS, want))
    return shared[key]


def records(bp, B):
    raw, st = bp.download_raw()
    assert st == bytes(B), list(st)
    assert len(raw) == 768 * B
    return [raw[768 * i:768 * (i + 1)] for i in range(B)]


def chain_batch(setup, shared, n, S):
    """The three witnesses with the scans in S segments: every status 0; each proof's six evaluations are the Python-integer Horner
    values at its own zeta; the records are the bytes of the S = 1 run; up to 2^8 the proofs are the oracle's (all three up to 2^6,
    x0 = 3 at 2^8); at 2^9 and above every proof passes the pairing check."""
    c = chain(shared, n)
    B = len(X0S)
    bp = pa.BatchProver(setup, c["program"], segments=S)
    bp.upload([dict(w) for w in c["wits"]])
    bp.run()
    recs = records(bp, B)
    assert len(set(recs)) == B
    flats = [pc.flat(pa.BatchProver.decode(r)) for r in recs]
    for i in range(B):
        ch = {k: v.n for k, v in bp.challenges(i).items()}
        want = expected_evals(shared, n, i, ch["beta"], ch["gamma"], ch["zeta"])
        for k in EVALS:
            assert flats[i][k] == want[k], (n, S, i, k)
    if S == 1:
        shared[("one workgroup", n)] = recs
    elif ("one workgroup", n) in shared:
        assert recs == shared[("one workgroup", n)], (n, S)
    else:
        chain_batch(setup, shared, n, 1)
        assert recs == shared[("one workgroup", n)], (n, S)
    if n <= ORACLE_UP_TO:
        for i in range(B if n <= 64 else 1):
            assert flats[i] == pc.oracle_chain_proof(n, X0S[i]), (n, S, i)
    else:
        vk = verification_key(setup, shared, n)
        for i in range(B):
            assert vk.verify_proof(n, pa.BatchProver.decode(recs[i]), [X0S[i]]), (n, S, i)


def segments_refused_at_16(setup, shared):
    """2^4 has the one-workgroup form alone: S = 2 would leave a segment 8 rows, and the library refuses it."""
    with pytest.raises(Exception):
        pa.BatchProver(setup, chain(shared, 16)["program"], segments=2)


# ---- a table of two circuits: S1 and S2 come from each proof's own circuit ---------------------------------------------------------
def two_circuits(setup, shared, S, n=64):
    """Circuit 0 the chain, circuit 1 the factorisation circuit padded to n; the batch is labelled 1, 0, 1.  Every proof is the
    oracle's proof of its own circuit: s1_eval and s2_eval read fixed_coef at the proof's circuit, not at circuit 0."""
    if "two circuits" not in shared:
        tables = [pc.chain_lines(n), pc.FACTORIZATION]
        oprogs = [OProgram(lines, n) for lines in tables]
        bits = lambda p, q: dict({"pb%d" % k: p >> k & 1 for k in range(4)}, **{"qb%d" % k: q >> k & 1 for k in range(4)})
        ids = [1, 0, 1]
        wits = [oprogs[1].fill_variable_assignments(dict(pc.FACTORIZATION_START)), oprogs[0].fill_variable_assignments({"x0": 3}),
                oprogs[1].fill_variable_assignments(bits(3, 5))]
        osetup = bc.osetup(shared)
        want = [pc.oracle_chain_proof(n, 3) if cid == 0 else OProver(osetup, oprogs[cid]).prove(dict(w)).flatten() for w, cid in zip(wits, ids)]
        assert want[0]["s1_eval"] != want[2]["s1_eval"]  # (another zeta) and neither is the chain's polynomial
        shared["two circuits"] = ([pa.Program(lines, n) for lines in tables], ids, wits, want)
    programs, ids, wits, want = shared["two circuits"]
    mp = pa.MultiBatchProver(setup, programs, segments=S)
    got = [pc.flat(p) for p in mp.prove_batch([dict(w) for w in wits], ids)]
    for i in range(len(ids)):
        assert got[i] == want[i], (S, i)


# ---- a blinded batch: blind_evals_kernel corrects the new sums ---------------------------------------------------------------------
def blinded(setup, shared, S, name="chain64"):
    """Three witnesses under explicit blinders (random; all r - 1; the t-split blinders zero) against the blinded prover's model on
    the CPU (blinding_cases.Model): the nine points and the six evaluations."""
    c = bc.circuit(shared, name)
    want = bc.model_proofs(shared, name)
    bp = pa.BatchProver(setup, c.program, blinding=bc.SEED, segments=S)
    bp.upload([dict(w) for w in c.wits[:3]])
    bp.set_blinders(bc.blinder_rows(name))
    bp.run()
    recs = records(bp, 3)
    for i in range(3):
        g = bc.flat_record(recs[i])
        for k in bc.POINTS + bc.EVALS:
            assert g[k] == want[i][k], (S, i, k)


# ---- the gate flags are zeroed by the batch's own first kernel -----------------------------------------------------------------------
def gate_failure_does_not_stick(setup):
    """A batch of three whose proof 1 breaks a gate (status bit 2), then an honest batch of three on the SAME prover: every status
    0.  gate_check_kernel only ever ORs into its words, so without the zeroing in front of it proof 1 of the second batch inherits
    the flag."""
    lines = ["e public", "c <== a * b", "e <== c * d"]
    program, oprog = pa.Program(lines, 8), OProgram(lines, 8)
    wits = [oprog.fill_variable_assignments({"a": 3 + i, "b": 4, "d": 5 + 2 * i}) for i in range(3)]
    bp = pa.BatchProver(setup, program)
    cols = [bp.wire_columns(w) for w in wits]
    mul = [tuple(cells) for cells in oprog.wires()].index(("a", "b", "c"))
    le = lambda v: b"".join(int(x).to_bytes(32, "little") for x in v)
    pub = b"".join(le([w["e"] % R_MOD]) for w in wits)
    good = b"".join(le(cols[b][k]) for k in range(3) for b in range(3))
    cols[1][2][mul] = (cols[1][2][mul] + 1) % R_MOD  # c <== a * b: its output is no longer a b
    bad = b"".join(le(cols[b][k]) for k in range(3) for b in range(3))
    bp.upload_raw(bad, pub, 3)
    bp.run()
    st = bp.download_raw()[1]
    assert st[0] == 0 and st[1] & 4 and st[2] == 0, list(st)
    bp.upload_raw(good, pub, 3)
    bp.run()
    raw, st = bp.download_raw()
    assert st == bytes(3), list(st)
    osetup = pc.OSetup.from_file(pc.PTAU)
    assert pc.flat(pa.BatchProver.decode(raw[768:2 * 768])) == OProver(osetup, oprog).prove(dict(wits[1])).flatten()
