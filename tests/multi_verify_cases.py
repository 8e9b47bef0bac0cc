"""Cases of the batch verifier over a table of circuits (plonkathon_amd.MultiBatchVerifier, plonk_verifier_create_multi,
plonk_verifier_load_multi, plonk_verifier_load_provers).

The same bodies run on the emulated kernels (tests/test_emu_multi_verify.py) and on the MI355X (tests/test_gpu_multi_verify.py).
All circuits are of ONE setup.  Every valid input is first shown valid by the per-proof verifier (`vk.verify_proof`).  Expected
fold points come from the oracle alone: `terms()` with each proof's own key and group order, the fixed-point sums kept per
circuit, oracle.g1.ec_lincomb, and the weights of `weights(SEED, B)` — the index is the proof's position in the mixed batch.
"""
import ctypes
import dataclasses
import itertools

import pytest

import parity_cases as pc
import plonkathon_amd as pa
from batch_verify_cases import SEED, Circuit, corruptions, flat_of, record, terms, weights
from helpers import R_MOD
from oracle import g1 as og1
from plonkathon_amd import BatchProver, BatchVerifier, MultiBatchVerifier, Program
from plonkathon_amd.field import Q_MOD
from plonkathon_amd.kzg import G2

TINY = {  # group order 8
    "A": ["e public", "c <== a * b", "e <== c * d"],
    "A'": ["e public", "c <== a * b", "e <== c * d + 3"],  # the shape of A: only Qc differs
    "Z": ["c <== a * b", "e <== c * d"],  # no public input
    "P2": ["e public", "a public", "c <== a * b", "e <== c * d + 7"],
}
MIXED = ["A", "F", "Z", "A'", "P2", "A", "F"]  # odd, so the last workgroup has a shadow proof; its pairs mix orders and public counts


def tiny_circuit(setup, name, count, **prover_args):
    """`count` distinct proofs of one of the TINY circuits or of F = the factorization circuit (group order 16)"""
    if name == "F":
        program = Program(pc.FACTORIZATION, 16)
        bits = sorted(pc.FACTORIZATION_START)  # proof i flips bit j of the start where i has bit j: 256 distinct witnesses
        starts = [{k: pc.FACTORIZATION_START[k] ^ ((i >> j) & 1) for j, k in enumerate(bits)} for i in range(count)]
        return Circuit(setup, pc.FACTORIZATION, 16, [program.fill_variable_assignments(s) for s in starts])
    program = Program(TINY[name], 8)
    wits = [program.fill_variable_assignments({"a": 3 + i, "b": 4, "d": 5}) for i in range(count)]
    if not prover_args:
        return Circuit(setup, TINY[name], 8, wits)
    circ = Circuit(setup, TINY[name], 8)  # a prover of its own options: prove here what Circuit proves with the defaults
    circ.prover = BatchProver(setup, circ.program, **prover_args)
    circ.prover.upload([dict(w) for w in wits])
    circ.prover.run()
    blob, status = circ.prover.download_raw()
    assert not any(status)
    circ.recs = [blob[768 * i : 768 * (i + 1)] for i in range(count)]
    circ.pubs = [[w[v] % R_MOD for v in circ.public_vars] for w in wits]
    return circ


class Table:
    """Circuits by name, a MultiBatchVerifier over them (ids in the order of `names`) and batches dealt from their proofs."""

    def __init__(self, circuits, names=None):
        self.circuits = circuits
        self.names = list(circuits) if names is None else list(names)
        self.mv = MultiBatchVerifier([(circuits[n].vk, len(circuits[n].public_vars)) for n in self.names])

    def circuit_of(self, cid):
        return self.circuits[self.names[cid]]

    def deal(self, ids):
        """(ids, records, public rows): position i takes the next unused proof of circuit ids[i]"""
        used = {}
        recs, pubs = [], []
        for cid in ids:
            circ = self.circuit_of(cid)
            j = used.get(id(circ), 0)
            used[id(circ)] = j + 1
            recs.append(circ.recs[j])
            pubs.append(circ.pubs[j])
        return list(ids), recs, pubs

    def deal_names(self, names):
        return self.deal([self.names.index(n) for n in names])

    def accepted_one_by_one(self, cid, rec, pub):
        return self.circuit_of(cid).accepted_one_by_one(rec, pub)

    def assert_valid(self, ids, recs, pubs, sample=None):
        for i in range(len(ids)) if sample is None else sample:
            assert self.accepted_one_by_one(ids[i], recs[i], pubs[i]), i


def tiny_table(setup):
    """The five small circuits with the proofs the cases deal from"""
    return Table({n: tiny_circuit(setup, n, c) for n, c in (("A", 3), ("F", 2), ("Z", 2), ("A'", 2), ("P2", 1))})


# ------------------------------------------------------------------------------------------ the oracle's fold
def oracle_fold(table, ids, recs, pubs, rhos, lo, hi):
    L, R, fixed_sum = [], [], {}
    for i in range(lo, hi):
        circ = table.circuit_of(ids[i])
        proof = flat_of(recs[i])
        own, fixed, left = terms(circ.ovk, circ.n, proof, pubs[i])
        L += [(proof[k], s * rhos[i] % R_MOD) for k, s in left.items()]
        R += [(proof[k], s * rhos[i] % R_MOD) for k, s in own.items()]
        for k, s in fixed.items():
            key = k if k == "G1" else (ids[i], k)  # the key points are the circuit's, G1 is everybody's
            fixed_sum[key] = (fixed_sum.get(key, 0) + s * rhos[i]) % R_MOD
    R += [(og1.G1 if key == "G1" else getattr(table.circuit_of(key[0]).ovk, key[1]), s) for key, s in fixed_sum.items()]
    return og1.ec_lincomb(L), og1.ec_lincomb(R)


def assert_folds(table, ids, recs, pubs, ranges):
    rhos = weights(SEED, len(ids))
    for lo, hi in ranges:
        L, R = table.mv.fold(lo, hi)
        assert (pc.affine(L), pc.affine(R)) == oracle_fold(table, ids, recs, pubs, rhos, lo, hi), (lo, hi)


# ------------------------------------------------------------------------------------------ 1. bit-exact folds
def bit_exact_folds(table, names=MIXED, ranges=((0, 7), (1, 2), (2, 3), (3, 7))):
    """MIXED: (2, 3) holds only the circuit without public inputs, (3, 7) no proof of it (its sums are zero)"""
    ids, recs, pubs = table.deal_names(names)
    table.assert_valid(ids, recs, pubs)
    table.mv.load(b"".join(recs), ids, pubs, SEED)
    assert table.mv.status == bytes(len(ids))
    assert_folds(table, ids, recs, pubs, ranges)
    assert table.mv.fold(4, 4) == (None, None)


# ------------------------------------------------------------------------------------------ 2. a table of one circuit
def one_circuit_equals_batch_verifier(table):
    circ = table.circuits["A"]
    recs, pubs = circ.recs[:3], circ.pubs[:3]
    circ.assert_valid(range(3))
    mv = MultiBatchVerifier([(circ.vk, 1)])
    mv.load(b"".join(recs), [0, 0, 0], pubs, SEED)
    circ.bv.load(b"".join(recs), pubs, SEED)
    assert mv.status == circ.bv.status == bytes(3)
    for lo, hi in ((0, 3), (1, 3)):
        assert mv.fold(lo, hi) == circ.bv.fold(lo, hi), (lo, hi)
    assert mv.verify(b"".join(recs), [0, 0, 0], pubs) and mv.pairing_checks == 1


# ------------------------------------------------------------------------------------------ 3. verdicts
def verdicts(table, of, names=MIXED):
    """`of`: the names of the circuits whose first proof in the batch is corrupted, one corruption at a time"""
    ids, recs, pubs = table.deal_names(names)
    table.assert_valid(ids, recs, pubs)
    mv = table.mv
    assert mv.verify(b"".join(recs), ids, pubs) and mv.pairing_checks == 1
    B = len(ids)
    for pos in [names.index(n) for n in of]:
        # the 17th corruption moves the first public input: a circuit without public inputs has the other 16
        n_cases = 17 if pubs[pos] else 16
        done = 0
        for name, bad_rec, bad_pub in itertools.islice(corruptions(recs[pos], pubs[pos]), n_cases):
            assert not table.accepted_one_by_one(ids[pos], bad_rec, bad_pub), (pos, name)
            blob = b"".join(recs[:pos] + [bad_rec] + recs[pos + 1 :])
            rows = pubs[:pos] + [bad_pub] + pubs[pos + 1 :]
            assert not mv.verify(blob, ids, rows), (pos, name)
            assert mv.status == bytes(B), (pos, name)  # well-formed, and wrong
            assert mv.verify_each(blob, ids, rows) == [i != pos for i in range(B)], (pos, name)
            done += 1
        assert done == n_cases


# ------------------------------------------------------------------------------------------ 4. a wrong label
def wrong_label(table):
    """A valid proof of A under the label of A' (same shape, another key) and under that of F (another group order)"""
    names = ["A", "A", "F", "A'", "Z", "A", "F"]
    ids, recs, pubs = table.deal_names(names)
    table.assert_valid(ids, recs, pubs)
    wrong = {1: table.names.index("A'"), 5: table.names.index("F")}
    for pos, cid in wrong.items():
        assert not table.accepted_one_by_one(cid, recs[pos], pubs[pos]), pos
        ids[pos] = cid
    mv = table.mv
    blob = b"".join(recs)
    assert not mv.verify(blob, ids, pubs) and mv.status == bytes(7)
    assert mv.verify_each(blob, ids, pubs) == [i not in wrong for i in range(7)]


# ------------------------------------------------------------------------------------------ 5. localisation across circuits
def localisation(table, names, bad, max_checks):
    """`bad`: {position: corruption number (0..16 of `corruptions`)}"""
    ids, recs, pubs = table.deal_names(names)
    B = len(ids)
    table.assert_valid(ids, recs, pubs, sample=list(bad))
    bad_recs, bad_pubs = list(recs), [list(p) for p in pubs]
    for i, which in bad.items():
        name, bad_recs[i], bad_pubs[i] = list(corruptions(recs[i], pubs[i]))[which]
        assert not table.accepted_one_by_one(ids[i], bad_recs[i], bad_pubs[i]), name
    mv = table.mv
    assert mv.verify_each(b"".join(bad_recs), ids, bad_pubs) == [i not in bad for i in range(B)]
    assert mv.pairing_checks <= max_checks, mv.pairing_checks
    assert mv.verify_each(b"".join(recs), ids, pubs) == [True] * B and mv.pairing_checks == 1


# ------------------------------------------------------------------------------------------ 6. malformed input is a verdict
def malformed(table):
    """The four spoilings of batch_verify_cases.malformed, each in another circuit; P2's only proof of the batch is one of them"""
    names = ["A", "A'", "F", "Z", "P2", "A"]
    ids, recs, pubs = table.deal_names(names)
    table.assert_valid(ids, recs, pubs)
    recs = [bytearray(r) for r in recs]
    recs[1][64 * 3 : 64 * 3 + 32] = Q_MOD.to_bytes(32, "little")                    # z_1.x = p
    recs[2][576 + 32 : 576 + 64] = (R_MOD + 5).to_bytes(32, "little")                # b_eval >= r
    y = int.from_bytes(recs[3][64 * 4 + 32 : 64 * 5], "little")
    recs[3][64 * 4 + 32 : 64 * 5] = ((y + 1) % Q_MOD).to_bytes(32, "little")         # t_lo_1 off the curve
    recs[4][64 * 8 : 64 * 9] = bytes(64)                                             # W_zw_1 = 64 zero bytes
    blob = b"".join(bytes(r) for r in recs)
    want_status = bytes([0, 1, 1, 2, 4, 0])
    mv = table.mv
    assert not mv.verify(blob, ids, pubs) and mv.status == want_status
    assert mv.verify_each(blob, ids, pubs) == [True, False, False, False, False, True]
    assert mv.status == want_status and mv.pairing_checks == 1  # the spoilt proofs take part in no fold: the rest passes at once
    assert mv.verify_each(blob[768 : 768 * 5], ids[1:5], pubs[1:5]) == [False] * 4  # nothing but spoilt proofs
    # compressed records: flag bits 00 (malformed) in the only proof of F, an x whose x^3 + 3 is not a square in the only one of Z
    ids, recs, pubs = table.deal_names(["A", "F", "Z"])
    comp = [bytearray(BatchProver.decode(r).to_bytes()) for r in recs]
    honest = b"".join(bytes(c) for c in comp)
    assert mv.verify(honest, ids, pubs) and mv.pairing_checks == 1
    comp[1][32 * 2] &= 0x3F                                                          # c_1: flag bits 00
    x = 1
    while pow((x ** 3 + 3) % Q_MOD, (Q_MOD - 1) // 2, Q_MOD) == 1:
        x += 1
    comp[2][32 * 5 : 32 * 6] = (x | (2 << 254)).to_bytes(32, "big")                  # t_mid_1: no such point
    blob480 = b"".join(bytes(c) for c in comp)
    assert mv.verify_each(blob480, ids, pubs) == [True, False, False] and mv.status == bytes([0, 1, 2]) and mv.pairing_checks == 1
    assert not mv.verify(blob480, ids, pubs)


# ------------------------------------------------------------------------------------------ 7. resident provers
def resident_provers(table, provers, sample):
    """`provers`: [(circuit name, Circuit whose prover holds its batch)]; load_provers == load of the downloaded bytes"""
    labelled = [(table.names.index(n), c.prover) for n, c in provers]
    ids = [cid for cid, bp in labelled for _ in range(bp._resident)]
    recs = [r for _, c in provers for r in c.recs]
    pubs = [p for _, c in provers for p in c.pubs]
    B = len(ids)
    table.assert_valid(ids, recs, pubs, sample=sample)
    mv = table.mv
    assert mv.verify_provers(labelled, seed=SEED) and mv.pairing_checks == 1 and mv.status == bytes(B)
    fold = mv.fold(0, B)
    blob = b"".join(c.prover.download_raw()[0] for _, c in provers)
    assert blob == b"".join(recs)
    assert mv.verify(blob, ids, pubs, seed=SEED) and mv.status == bytes(B)
    assert mv.fold(0, B) == fold  # the same proofs, labels and weights whether they came through the host or not
    assert mv.verify_each_provers(labelled) == [True] * B and mv.pairing_checks == 1


def resident_prover_errors(table, setup):
    """table: A, F, Z"""
    a, f = table.circuits["A"], table.circuits["F"]
    ia, i_f = table.names.index("A"), table.names.index("F")
    mv = table.mv
    with pytest.raises(AssertionError):
        mv.load_provers([(ia, a.prover), (ia, f.prover)])  # a prover under the label of a circuit of another shape
    with pytest.raises(pa._lib.BackendError):
        mv.load_provers([(ia, a.prover), (ia, BatchProver(setup, a.program))])  # nothing resident in the second
    ctx = mv.ctx
    rc = ctx.L.plonk_verifier_load(mv._h, a.recs[0], bytes(32), 1, SEED)  # the one-circuit calls on a table of three
    assert rc == pa._lib.PLONK_ERR_STATE
    rc = ctx.L.plonk_verifier_load_prover(mv._h, a.prover._h, a.prover._resident, SEED)
    assert rc == pa._lib.PLONK_ERR_STATE
    assert mv.verify_provers([(ia, a.prover), (i_f, f.prover)])


# ------------------------------------------------------------------------------------------ 8. limits and arguments
def limits(table):
    """A table of MAX_CIRCUITS circuits: A, A', F over and over (keys may repeat); seven proofs on ids spread over all of it"""
    K = MultiBatchVerifier.MAX_CIRCUITS
    cycle = ["A", "A'", "F"]
    names = [cycle[c % 3] for c in range(K)]
    full = Table(table.circuits, names)
    ids = [i * (K - 1) // 6 for i in range(6)]
    ids = [c + (i - c) % 3 for i, c in enumerate(ids)] + [K - 1]  # A, A', F, A, A', F at about every sixth of the table, and its last id
    assert len(set(ids)) == 7 and max(ids) == K - 1 and {names[c] for c in ids} == set(cycle)
    ids, recs, pubs = full.deal(ids)
    full.assert_valid(ids, recs, pubs)
    full.mv.load(b"".join(recs), ids, pubs, SEED)
    assert full.mv.status == bytes(7)
    assert_folds(full, ids, recs, pubs, [(0, 7), (2, 6)])
    key = lambda n: (table.circuits[n].vk, len(table.circuits[n].public_vars))
    with pytest.raises(AssertionError):
        MultiBatchVerifier([key(n) for n in names + ["A"]])
    with pytest.raises(AssertionError):
        MultiBatchVerifier([])
    ctx, h = full.mv.ctx, ctypes.c_void_p()  # and past the Python layer
    for k in (0, K + 1):
        rc = ctx.L.plonk_verifier_create_multi(ctx.handle, k, (ctypes.c_uint * (K + 1))(*[3] * (K + 1)), bytes(512 * (K + 1)),
                                               (ctypes.c_size_t * (K + 1))(), ctypes.byref(h))
        assert rc == pa._lib.PLONK_ERR_ARG and not h.value, k


def arguments(table):
    ids, recs, pubs = table.deal_names(["A", "Z", "P2"])
    blob = b"".join(recs)
    mv, K = table.mv, len(table.names)
    mv.load(blob, ids, pubs, SEED)
    for lo, hi in ((2, 1), (0, 4), (4, 4)):
        with pytest.raises(AssertionError):
            mv.fold(lo, hi)  # a range outside the batch
    assert mv.fold(3, 3) == (None, None)
    with pytest.raises(AssertionError):
        mv.verify(blob, [ids[0], K, ids[2]], pubs)  # a circuit id outside the table
    with pytest.raises(AssertionError):
        mv.verify(blob, ids, [pubs[0], [1], pubs[2]])  # a row of the wrong length for its circuit
    with pytest.raises(AssertionError):
        mv.verify(blob, ids, [[R_MOD], pubs[1], pubs[2]])  # a public input not below r
    with pytest.raises(AssertionError):
        mv.verify(blob[:-1], ids, pubs)
    ctx = mv.ctx  # through the raw C call: a circuit id outside the table, n_public_values off by one either way
    pub = b"".join(int(x).to_bytes(32, "little") for row in pubs for x in row)
    c_ids = lambda l: (ctypes.c_uint32 * 3)(*l)
    assert ctx.L.plonk_verifier_load_multi(mv._h, blob, c_ids([ids[0], K, ids[2]]), pub, 3, 3, SEED) == pa._lib.PLONK_ERR_ARG
    for count in (2, 4):
        assert ctx.L.plonk_verifier_load_multi(mv._h, blob, c_ids(ids), pub + bytes(32), count, 3, SEED) == pa._lib.PLONK_ERR_ARG
    assert ctx.L.plonk_verifier_load_multi(mv._h, blob, c_ids(ids), pub, 3, 3, SEED) == pa._lib.PLONK_OK
    other = dataclasses.replace(table.circuits["Z"].vk, X_2=G2)  # a key of another setup
    assert other.X_2 != table.circuits["A"].vk.X_2
    with pytest.raises(AssertionError):
        MultiBatchVerifier([(table.circuits["A"].vk, 1), (other, 0)])
    assert mv.verify(blob, ids, pubs)
