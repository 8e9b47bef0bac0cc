"""Cases of the lock-step prover over a table of circuits (plonkathon_amd.MultiBatchProver, plonk_prover_create_multi,
plonk_prover_set_wiring_multi, plonk_prover_set_labels, plonk_verifier_load_multi_prover).

The same bodies run on the emulated kernels (tests/test_emu_multi_prover.py) and on the MI355X (tests/test_gpu_multi_prover.py).
The reference is the one-circuit `BatchProver`, which the suite pins to the goldens and the oracle: every witness of a mixed batch
is also proved by a BatchProver of its own circuit with the same options, and the 768-byte records and the status bytes are
compared byte for byte.  One case is pinned to the oracle directly.

All circuits of a `Family` are compiled at one group order n: the four tiny circuits of multi_verify_cases (padded), the chain
(full height, one public input) and `two` (full height, two public inputs).  Batches are dealt unsorted, do not start at circuit 0
and are odd-sized (the transcript kernel shadows the last proof); the table holds a circuit that no proof of the batch uses.
"""
import ctypes
import random

import pytest

import parity_cases as pc
import plonkathon_amd as pa
from helpers import R_MOD
from multi_verify_cases import TINY
from plonkathon_amd import BatchProver, MultiBatchProver, MultiBatchVerifier, Program
from plonkathon_amd._lib import PLONK_ERR_ARG, PLONK_ERR_STATE, BackendError
from plonkathon_amd.batch import _pack_witnesses

NAMES = ["A", "chain", "Z", "P2", "two", "A'"]  # public inputs: 1, 1, 0, 2, 2, 1
IDS = [2, 0, 3, 4, 1, 0, 4]                      # Z, A, P2, two, chain, A, two; A' is in the table and not in the batch
SEED = bytes(range(32))
ST_Z_OPEN, ST_GATE = 2, 4                        # PROVER_ST_*


def two_lines(n):
    """full height, two public inputs: one for y, one for the chain's start"""
    return ["x0 public", "y public"] + ["x%d <== x%d * y + %d" % (i + 1, i, i + 1) if i % 2 else "x%d <== x%d + y" % (i + 1, i)
                                        for i in range(n - 2)]


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


class Family:
    """The circuits by name at one group order, their one-circuit provers and the provers over tables of them, each built once."""

    def __init__(self, setup, n):
        self.setup, self.n = setup, n
        self._programs, self._single, self._multi, self._vks = {}, {}, {}, {}

    def program(self, name):
        if name not in self._programs:
            lines = pc.chain_lines(self.n) if name == "chain" else two_lines(self.n) if name == "two" else TINY[name]
            self._programs[name] = Program(lines, self.n)
        return self._programs[name]

    def witness(self, name, j):
        """the j-th distinct witness of a circuit; chain, 0 is x0 = 3"""
        start = {"x0": 3 + j} if name == "chain" else {"x0": 5 + j, "y": 7 + 2 * j} if name == "two" else {"a": 3 + j, "b": 4, "d": 5}
        return self.program(name).fill_variable_assignments(start)

    def vk(self, name):
        if name not in self._vks:
            self._vks[name] = self.setup.verification_key(self.program(name).common_preprocessed_input())
        return self._vks[name]

    def single(self, name, **opts):
        key = (name, tuple(sorted(opts.items())))
        if key not in self._single:
            self._single[key] = BatchProver(self.setup, self.program(name), **opts)
        return self._single[key]

    def multi(self, names=NAMES, **opts):
        key = (tuple(names), tuple(sorted(opts.items())))
        if key not in self._multi:
            self._multi[key] = MultiBatchProver(self.setup, [self.program(x) for x in names], **opts)
        return self._multi[key]

    def deal(self, ids, names=NAMES):
        """position i takes the next unused witness of circuit ids[i]"""
        used, wits = {}, []
        for c in ids:
            wits.append(self.witness(names[c], used.get(c, 0)))
            used[c] = used.get(c, 0) + 1
        return wits

    def public_rows(self, ids, wits, names=NAMES):
        return [[w[v] % R_MOD for v in self.program(names[c]).get_public_assignments()] for c, w in zip(ids, wits)]

    def reference(self, ids, wits, names=NAMES, blinders=None, **opts):
        """(records, status bytes, challenges) by position, each circuit's proofs from a BatchProver of that circuit alone"""
        B = len(ids)
        recs, status, chal = [None] * B, [None] * B, [None] * B
        for c in sorted(set(ids)):
            pos = [i for i in range(B) if ids[i] == c]
            bp = self.single(names[c], **opts)
            bp.upload([dict(wits[i]) for i in pos])
            if blinders is not None:
                bp.set_blinders([blinders[i] for i in pos])
            bp.run()
            raw, st = bp.download_raw()
            for k, i in enumerate(pos):
                recs[i], status[i], chal[i] = raw[768 * k : 768 * (k + 1)], st[k], bp.challenges(k)
        return recs, bytes(status), chal

    # ---- the three ways a mixed batch comes in
    def blob(self, mp, ids, wits):
        return b"".join(_pack_witnesses([w], mp.variables(c), R_MOD) + bytes(32 * (mp.n_vars - len(mp.variables(c)))) for c, w in zip(ids, wits))

    def columns(self, ids, wits, names=NAMES):
        """[B] x [3][n] wire columns and the [B][l_max] public rows, zero padded"""
        l_max = max(len(self.program(x).get_public_assignments()) for x in names)
        cols = [self.single(names[c]).wire_columns(w) for c, w in zip(ids, wits)]
        rows = [row + [0] * (l_max - len(row)) for row in self.public_rows(ids, wits, names)]
        return cols, rows

    def upload(self, mp, ids, wits, route, names=NAMES):
        if route == "upload":
            mp.upload([dict(w) for w in wits], ids)
        elif route == "values":
            mp.upload_values(self.blob(mp, ids, wits), ids)
        elif route == "raw":
            cols, rows = self.columns(ids, wits, names)
            mp.upload_raw(b"".join(le(cols[b][k]) for k in range(3) for b in range(len(ids))), b"".join(le(r) for r in rows) or None, ids)
        else:
            assert route == "async"
            blob = self.blob(mp, ids, wits)
            self.pinned = mp.ctx.host_alloc(len(blob))  # alive until the download
            self.pinned[: len(blob)] = blob
            mp.upload_values_async(self.pinned, ids)


def records(mp):
    raw, st = mp.download_raw()
    return [raw[768 * i : 768 * (i + 1)] for i in range(len(st))], st


def compressed(rec):
    return BatchProver.decode(rec).to_bytes()


# ------------------------------------------------------------------------------------------ 1. bytes, by every route
def bytes_by_every_route(fam, routes=("upload", "values", "raw"), **opts):
    wits = fam.deal(IDS)
    want, want_st, want_chal = fam.reference(IDS, wits, **opts)
    assert want_st == bytes(len(IDS))
    mp = fam.multi(**opts)
    for route in routes:
        fam.upload(mp, IDS, wits, route)
        mp.run()
        got, st = records(mp)
        assert st == bytes(len(IDS)), (route, list(st))
        for i in range(len(IDS)):
            assert got[i] == want[i], (route, i, NAMES[IDS[i]])
            assert mp.challenges(i) == want_chal[i], (route, i)
        comp, st = mp.download_compressed()
        assert st == bytes(len(IDS)) and comp == b"".join(compressed(r) for r in got), route
        assert mp.circuit_ids == IDS
        if route != "raw":
            assert mp.public_values() == fam.public_rows(IDS, wits)


# ------------------------------------------------------------------------------------------ 2. pinned to the oracle
def oracle_pin(fam):
    """the chain proof for x0 = 3 at position 4 of the mixed batch is the oracle prover's"""
    assert NAMES[IDS[4]] == "chain"
    wits = fam.deal(IDS)
    assert wits[4]["x0"] == 3
    mp = fam.multi()
    mp.upload([dict(w) for w in wits], IDS)
    mp.run()
    got, st = records(mp)
    assert st == bytes(len(IDS))
    assert pc.flat(BatchProver.decode(got[4])) == pc.oracle_chain_proof(fam.n, 3)


# ------------------------------------------------------------------------------------------ 3. a table of one circuit
def table_of_one(fam, name="two"):
    wits = [fam.witness(name, j) for j in range(3)]
    want, want_st, want_chal = fam.reference([0] * 3, wits, names=[name])
    mp = fam.multi([name])
    for ids in ([0, 0, 0], None):  # labelled, and without labels
        mp.upload([dict(w) for w in wits], ids)
        mp.run()
        got, st = records(mp)
        assert got == want and st == want_st == bytes(3)
        assert [mp.challenges(i) for i in range(3)] == want_chal
        assert mp.circuit_ids == [0, 0, 0]
    mp.upload_values(fam.blob(mp, [0] * 3, wits), 3)  # packed values and a batch size alone
    mp.run()
    assert records(mp) == (want, want_st)


# ------------------------------------------------------------------------------------------ 4. options
def blinded_with_explicit_rows(fam, **opts):
    """a mixed blinded batch gives the bytes of one-circuit blinded provers handed the same rows"""
    rng = random.Random("multi prover blinders %d" % fam.n)
    rows = [[rng.randrange(R_MOD) for _ in range(11)] for _ in IDS]
    rows[1] = [R_MOD - 1] * 11
    wits = fam.deal(IDS)
    want, want_st, _ = fam.reference(IDS, wits, blinders=rows, blinding=SEED, **opts)
    plain, _, _ = fam.reference(IDS, wits, **opts)
    assert want_st == bytes(len(IDS)) and all(w != p for w, p in zip(want, plain))
    mp = fam.multi(blinding=SEED, **opts)
    mp.upload([dict(w) for w in wits], IDS)
    mp.set_blinders(rows)
    mp.run()
    got, st = records(mp)
    assert st == bytes(len(IDS))
    for i in range(len(IDS)):
        assert got[i] == want[i], (i, NAMES[IDS[i]])


def blinded_with_a_seed(fam, check=(0, 3, 4)):
    """two runs over one upload differ in every proof, and the per-proof verifier accepts both"""
    wits = fam.deal(IDS)
    pubs = fam.public_rows(IDS, wits)
    mp = fam.multi(blinding=SEED)
    mp.upload([dict(w) for w in wits], IDS)
    runs = []
    for _ in range(2):
        mp.run()
        got, st = records(mp)
        assert st == bytes(len(IDS))
        runs.append(got)
    assert all(a != b for a, b in zip(*runs))
    for got in runs:
        for i in check:
            assert fam.vk(NAMES[IDS[i]]).verify_proof(fam.n, BatchProver.decode(got[i]), pubs[i]), i


# ------------------------------------------------------------------------------------------ 5. statuses are per proof
def statuses_are_per_proof(fam):
    """A valid witness of A under the label of A' (only Qc differs) fails that proof's gates, a witness whose two cells of c differ
    (each row's gate satisfied) leaves that proof's Z open; every other proof keeps its bytes and its status 0."""
    ids = [2, 0, 5, 4, 1, 2, 0]
    wits = fam.deal(ids)
    a_prime, z_open = 2, 5
    wits[a_prime] = fam.witness("A", 2)  # a witness of A at the position labelled A'
    want, want_st, _ = fam.reference(ids, wits)  # (A and A' have the same variables: the one-circuit prover of A' takes it too)
    assert want_st == bytes([0, 0, ST_GATE, 0, 0, 0, 0])
    cols, rows = fam.columns(ids, wits)
    wires = [w.as_list() for w in fam.program("Z").wires()]
    out = wires.index(["c", "d", "e"])
    cprime = (cols[z_open][0][out] + 1) % R_MOD
    cols[z_open][0][out] = cprime
    cols[z_open][2][out] = cprime * cols[z_open][1][out] % R_MOD
    mp = fam.multi()
    mp.upload_raw(b"".join(le(cols[b][k]) for k in range(3) for b in range(7)), b"".join(le(r) for r in rows), ids)
    mp.run()
    got, st = records(mp)
    assert st == bytes([0, 0, ST_GATE, 0, 0, ST_Z_OPEN, 0]), list(st)
    for i in range(7):
        if i != z_open:
            assert got[i] == want[i], i


# ------------------------------------------------------------------------------------------ 6. batches in sequence
def batches_in_sequence(fam):
    """B = 7, then B = 3 under other labels, then B = 7 again on one prover: no label of an earlier batch is read, buffers regrow"""
    mp = MultiBatchProver(fam.setup, [fam.program(x) for x in NAMES])
    for ids in (IDS, [5, 1, 3], [4, 5, 0, 2, 3, 1, 5]):
        wits = fam.deal(ids)
        want, want_st, _ = fam.reference(ids, wits)
        mp.upload([dict(w) for w in wits], ids)
        mp.run()
        assert records(mp) == (want, want_st) and want_st == bytes(len(ids)), ids
        assert mp.circuit_ids == ids


# ------------------------------------------------------------------------------------------ 7. refusals
def refusals(fam):
    """Every refusal leaves the prover usable: the honest batch proves after each"""
    setup = fam.setup
    mp = fam.multi()
    L = mp.ctx.L
    K, B = len(NAMES), len(IDS)
    wits = fam.deal(IDS)
    want, want_st, _ = fam.reference(IDS, wits)
    blob = fam.blob(mp, IDS, wits)
    c_ids = lambda ids: (ctypes.c_uint32 * len(ids))(*ids)

    def still_proves():
        mp.upload([dict(w) for w in wits], IDS)
        mp.run()
        assert records(mp) == (want, want_st)

    # K = 0 and K = 65
    A = fam.program("A")
    for programs in ([], [A] * (MultiBatchProver.MAX_CIRCUITS + 1)):
        with pytest.raises(ValueError):
            MultiBatchProver(setup, programs)
    ctx, h = mp.ctx, ctypes.c_void_p()
    k_max = MultiBatchProver.MAX_CIRCUITS
    sel = pa.batch._selector_bytes(A) * (k_max + 1)
    for k in (0, k_max + 1):
        rc = L.plonk_prover_create_multi(ctx.handle, mp._bases.handle, fam.n.bit_length() - 1, k, sel, (ctypes.c_size_t * (k_max + 1))(*[1] * (k_max + 1)), ctypes.byref(h))
        assert rc == PLONK_ERR_ARG and not h.value, k
    # a label >= K
    assert L.plonk_prover_set_labels(mp._h, c_ids(IDS[:-1] + [K]), B) == PLONK_ERR_ARG
    with pytest.raises(AssertionError):
        mp.upload([dict(w) for w in wits], IDS[:-1] + [K])
    # K > 1 and no labels (the refused labels above are not pending)
    still_proves()
    assert L.plonk_prover_upload_variables(mp._h, blob, B) == PLONK_ERR_STATE
    assert b"plonk_prover_set_labels" in L.plonk_last_error()
    abc = bytes(32 * 3 * B * fam.n)
    assert L.plonk_prover_upload_witness(mp._h, abc, bytes(32 * 2 * B), B) == PLONK_ERR_STATE
    mp.run()  # the resident batch was not given up
    assert records(mp) == (want, want_st)
    # labels for another batch size: they stay pending until labels of the right size replace them
    assert L.plonk_prover_set_labels(mp._h, c_ids(IDS[:3]), 3) == pa._lib.PLONK_OK
    assert L.plonk_prover_upload_variables(mp._h, blob, B) == PLONK_ERR_STATE
    assert b"the labels were set for a batch of 3" in L.plonk_last_error()
    still_proves()
    # a non-zero public value beyond the circuit's own count: position 0 is of Z, which has none
    cols, rows = fam.columns(IDS, wits)
    abc = b"".join(le(cols[b][k]) for k in range(3) for b in range(B))
    for bad_at in ((0, 0), (1, 1), (4, 1)):  # Z's first, A's second, the chain's second
        bad = [list(r) for r in rows]
        bad[bad_at[0]][bad_at[1]] = 1
        with pytest.raises(AssertionError):
            mp.upload_raw(abc, b"".join(le(r) for r in bad), IDS)
    mp.upload_raw(abc, b"".join(le(r) for r in rows), IDS)
    mp.run()
    assert records(mp) == (want, want_st)
    # the wiring of one circuit on a table
    assert L.plonk_prover_set_wiring(mp._h, (ctypes.c_uint32 * (3 * fam.n))(), None, 1) == PLONK_ERR_STATE
    # the solver and the two-slot intake
    pinned = ctx.host_alloc(len(blob))
    pinned[: len(blob)] = blob
    for call in (lambda: mp.set_inputs([0]), lambda: mp.upload_input_values(blob, B), lambda: mp.solve_plan(B),
                 lambda: mp.stage_values_async(pinned, B), lambda: mp.advance()):
        with pytest.raises(BackendError, match="status %d" % PLONK_ERR_STATE):
            call()
    assert L.plonk_prover_stage_inputs(mp._h, blob, B) == PLONK_ERR_STATE and L.plonk_prover_upload_inputs_async(mp._h, blob, B) == PLONK_ERR_STATE
    mp.run()
    assert records(mp) == (want, want_st)
    # the loads of one-circuit provers
    vk = fam.vk("A")
    bv = pa.BatchVerifier(vk, 1)
    assert L.plonk_verifier_load_prover(bv._h, mp._h, B, SEED) == PLONK_ERR_ARG
    mv = MultiBatchVerifier([(vk, 1)])
    handles = (ctypes.c_void_p * 2)(fam.single("A")._h.value, mp._h.value)
    fam.single("A").upload([dict(fam.witness("A", 0))])
    fam.single("A").run()
    assert L.plonk_verifier_load_provers(mv._h, 2, handles, c_ids([0, 0]), SEED) == PLONK_ERR_ARG
    assert L.plonk_verifier_load_provers(mv._h, 1, handles, c_ids([0]), SEED) == pa._lib.PLONK_OK
    still_proves()


# ------------------------------------------------------------------------------------------ 8. the verifier on the resident batch
def verifier_table(fam, names=NAMES):
    return MultiBatchVerifier([(fam.vk(x), len(fam.program(x).get_public_assignments())) for x in names])


def verifier_loads_the_resident_batch(fam, devices=(False, True)):
    B = len(IDS)
    wits = fam.deal(IDS)
    mp, mv = fam.multi(), verifier_table(fam)
    mp.upload([dict(w) for w in wits], IDS)
    mp.run()
    assert mv.verify_prover(mp, seed=SEED) and mv.pairing_checks == 1 and mv.status == bytes(B)
    fold = mv.fold(0, B), mv.fold(1, 5)
    got, st = records(mp)
    pubs = mp.public_values()
    assert pubs == fam.public_rows(IDS, wits)
    mv.load(b"".join(got), IDS, pubs, SEED)
    assert (mv.fold(0, B), mv.fold(1, 5)) == fold  # the same proofs, labels, rows and weights as through the host
    assert mv.verify_each_prover(mp) == [True] * B
    # a verifier whose table is in another order: the map says where the prover's circuits are
    order = [3, 5, 0, 1, 4, 2]
    other = verifier_table(fam, [NAMES[c] for c in order])
    inverse = [order.index(c) for c in range(len(NAMES))]
    assert other.verify_prover(mp, inverse, seed=SEED)
    # the labels of A and A' exchanged (the same shape, so the map is accepted): the proofs of A are bad
    swapped = list(range(len(NAMES)))
    swapped[0], swapped[5] = 5, 0
    for device in devices:
        assert mv.verify_each_prover(mp, swapped, seed=SEED, device=device) == [NAMES[c] != "A" for c in IDS], device
    # a map onto a circuit of another shape, a map outside the table, a prover with nothing resident
    with pytest.raises(AssertionError):
        mv.load_prover(mp, [2, 1, 0, 3, 4, 5])
    rc = mv.ctx.L.plonk_verifier_load_multi_prover(mv._h, mp._h, (ctypes.c_uint32 * 6)(0, 1, 2, 3, 4, 6), SEED)
    assert rc == PLONK_ERR_ARG
    fresh = MultiBatchProver(fam.setup, [fam.program(x) for x in NAMES])
    with pytest.raises(BackendError, match="status %d" % PLONK_ERR_STATE):
        mv.load_prover(fresh)
    # one proof spoiled (a witness of A under the label of A'): named by bisection and by the device's own checks
    ids = [2, 0, 5, 4, 1, 2, 0]
    wits = fam.deal(ids)
    wits[2] = fam.witness("A", 2)
    mp.upload([dict(w) for w in wits], ids)
    mp.run()
    assert mp.download_raw()[1] == bytes([0, 0, ST_GATE, 0, 0, 0, 0])
    assert not mv.verify_prover(mp, seed=SEED)
    for device in devices:
        assert mv.verify_each_prover(mp, seed=SEED, device=device) == [i != 2 for i in range(7)], device


# ------------------------------------------------------------------------------------------ the benchmark's group order
def mixed_batch_at_2048(setup):
    """chain x 5, Poseidon x 2, A x 2 at 2^11 in one batch: the bytes of the three one-circuit provers; two proofs of each circuit
    under the per-proof verifier"""
    import batch_verify_cases as bc
    import bench

    bench.GROUP_ORDER = 2048
    a = Program(TINY["A"], 2048)
    circs = [bc.chain_circuit(setup, 5), bc.poseidon_circuit(setup), bc.Circuit(setup, TINY["A"], 2048, [a.fill_variable_assignments({"a": 3 + i, "b": 4, "d": 5}) for i in range(2)])]
    wits = {0: [bench.witness_for(i) for i in range(5)],  # the witnesses those three proved
            1: [circs[1].program.fill_variable_assignments({"L0": 1 + 2 * i, "M0": 2 + 2 * i}) for i in range(2)],
            2: [a.fill_variable_assignments({"a": 3 + i, "b": 4, "d": 5}) for i in range(2)]}
    ids = [1, 0, 2, 0, 0, 1, 0, 2, 0]
    used, batch, want, pubs = {}, [], [], []
    for c in ids:
        j = used.get(c, 0)
        used[c] = j + 1
        batch.append(dict(wits[c][j]))
        want.append(circs[c].recs[j])
        pubs.append(circs[c].pubs[j])
    mp = MultiBatchProver(setup, [c.program for c in circs])
    mp.upload(batch, ids)
    mp.run()
    got, st = records(mp)
    assert st == bytes(9)
    for i in range(9):
        assert got[i] == want[i], (i, ids[i])
    assert mp.public_values() == pubs
    for i in (0, 5, 1, 3, 2, 7):  # two of each circuit
        assert circs[ids[i]].accepted_one_by_one(got[i], pubs[i]), i
