"""Bodies of the tests of the two-slot intake (csrc/prover_intake.h: plonk_prover_stage_inputs / _stage_variables / _staged / _advance;
batch.py: stage_*, staged, advance, prove_inputs_stream), shared by tests/test_emu_intake_pipeline.py (emulated kernels) and
tests/test_gpu_intake_pipeline.py (MI355X).  The checkers are a FRESH prover's prove_inputs of the same batch, the oracle's prover
for proof 0 of the small chain (no committed fixture is this small), and the oracle's fill_variable_assignments."""
import ctypes

import numpy as np
import pytest

from helpers import R_MOD

import plonkathon_amd as pa
from oracle.circuit import Program as OProgram
from oracle.plonk_prover import Prover as OProver
from oracle.srs import Setup as OSetup
from parity_cases import PTAU, chain_lines, flat
from plonkathon_amd._lib import BackendError
from witness_levels_cases import braid, braid_starts
from witness_solve_cases import assert_variables, oracle_fill

ERR_ARG, ERR_STATE = -1, -4
BATCHES = (2, 5, 1, 5)  # the GPU adds 65: one lane past a 64-lane workgroup of the one-lane solver
WIDE_W, WIDE_N = 300, 1024  # witness_levels_cases.braid(300, 3): levels of 301, 300, 300 and 1 rows


def le(vals):
    return b"".join(int(v % R_MOD).to_bytes(32, "little") for v in vals)


class Circuit:
    """A circuit of these cases: its lines, its inputs, B distinct starts for batch number k, and the provers' `solve` form."""

    def __init__(self, name, lines, n, inputs, starts, solve=None):
        self.name, self.lines, self.n, self.inputs, self.starts, self.solve = name, lines, n, inputs, starts, solve
        self.program = pa.Program(lines, n)
        self.oprog = OProgram(lines, n)

    def prover(self, setup):
        bp = pa.BatchProver(setup, self.program, solve=self.solve)
        bp.set_inputs(self.inputs)
        return bp

    def fill(self, starts):
        return oracle_fill(self.lines, self.n, starts, self.oprog)


def circuit(shared, name):
    """"chain32" / "chain128": the chain at 2^5 / 2^7; "wide-lanes" / "wide-levels": braid(300, 3) at 2^10 under a forced form."""
    if ("circuit", name) not in shared:
        if name.startswith("chain"):
            n = int(name[5:])
            c = Circuit(name, chain_lines(n), n, ["x0"], lambda k, B: [{"x0": 3 + 1000003 * b + 7919 * k} for b in range(B)])
        else:
            c = Circuit(name, braid(WIDE_W, 3), WIDE_N, ["p", "q"], lambda k, B: braid_starts(B, salt=50 * k + 1), solve=name[5:])
        shared[("circuit", name)] = c
    return shared[("circuit", name)]


def proved(bp, B):
    """(records, status bytes, the six challenges of every proof) of the resident batch, which has been run."""
    raw, st = bp.download_raw()
    assert len(raw) == 768 * B and len(st) == B
    return raw, st, [tuple(v.n for v in bp.challenges(b).values()) for b in range(B)]


def references(setup, shared, c, sizes):
    """Per batch k of `sizes`: what a fresh prover's prove_inputs gives for c.starts(k, B) — once per circuit and module.  The fresh
    prover picks its solve form by the automatic rule: the two forced forms of the wide circuit are held to the same bytes."""
    refs = shared.setdefault(("refs", c.name.split("-")[0]), {})
    for k, B in enumerate(sizes):
        if (k, B) not in refs:
            fresh = pa.BatchProver(setup, c.program)
            fresh.prove_inputs([dict(s) for s in c.starts(k, B)])
            refs[(k, B)] = proved(fresh, B)
            assert refs[(k, B)][1] == bytes(B)
    assert len({refs[(k, B)][0] for k, B in enumerate(sizes)}) == len(sizes)  # every batch is another batch
    return [refs[(k, B)] for k, B in enumerate(sizes)]


def pinned_blob(bp, blob, keep):
    buf = bp.ctx.host_alloc(len(blob))
    buf[: len(blob)] = blob
    keep.append(buf)
    return buf


def stager(bp, c, mode, keep):
    """stage(k, B): batch k of the circuit into the second slot, by the entry point `mode` names."""
    def stage(k, B):
        starts = c.starts(k, B)
        if mode == "inputs":
            bp.stage_inputs([dict(s) for s in starts])
        elif mode == "input_values":
            bp.stage_input_values_async(pinned_blob(bp, le([s[v] for s in starts for v in bp.inputs]), keep), B)
        else:
            bp.stage_values_async(pinned_blob(bp, le([w[v] for w in c.fill(starts) for v in bp.variables]), keep), B)
        assert bp.staged == B
    return stage


# ---- 1. bytes ------------------------------------------------------------------------------------------------------------------
def oracle_proof_zero(shared, c, sizes):
    if ("oracle", c.name) not in shared:
        wit = c.fill(c.starts(0, sizes[0]))[0]
        shared[("oracle", c.name)] = OProver(OSetup.from_file(PTAU), c.oprog).prove(dict(wit)).flatten()
    return shared[("oracle", c.name)]


def bytes_through_the_pipeline(setup, shared, name, mode, sizes=BATCHES, oracle=False):
    """One prover, the batches of `sizes` through stage / run / download / advance, batch k + 1 staged with no host wait right after
    run(k) was enqueued; the first batch comes in through the second slot too.  Records, status and challenges of every batch are
    those of a fresh prover's prove_inputs; with `oracle`, proof 0 of batch 0 is the oracle prover's."""
    c = circuit(shared, name)
    want = references(setup, shared, c, sizes)
    bp = c.prover(setup)
    keep = []
    stage = stager(bp, c, mode, keep)
    assert bp.staged == 0
    stage(0, sizes[0])
    assert bp.advance() == sizes[0] and bp.staged == 0
    for k, B in enumerate(sizes):
        bp.run()
        if k + 1 < len(sizes):
            stage(k + 1, sizes[k + 1])
        got = proved(bp, B)
        assert got == want[k], (name, mode, k, B)
        if oracle and k == 0:
            assert flat(pa.BatchProver.decode(got[0][:768])) == oracle_proof_zero(shared, c, sizes)
        if k + 1 < len(sizes):
            assert bp.advance() == sizes[k + 1]
    for buf in keep:
        bp.ctx.host_free(buf)


def stream_yields_the_same_bytes(setup, shared, name, sizes=BATCHES):
    c = circuit(shared, name)
    want = references(setup, shared, c, sizes)
    bp = pa.BatchProver(setup, c.program, solve=c.solve)  # the first batch's keys set the inputs
    seen = 0
    for k, proofs in enumerate(bp.prove_inputs_stream([dict(s) for s in c.starts(k, B)] for k, B in enumerate(sizes))):
        assert [flat(p) for p in proofs] == [flat(pa.BatchProver.decode(want[k][0][768 * b:768 * (b + 1)])) for b in range(sizes[k])], k
        assert bp.download_raw() == want[k][:2]  # the batch just yielded is still the resident one
        assert bp.staged == (sizes[k + 1] if k + 1 < len(sizes) else 0)
        seen += 1
    assert seen == len(sizes) and list(bp.prove_inputs_stream([])) == []


# ---- 2. flags stay with their batch -------------------------------------------------------------------------------------------
def checked_chain(setup, n=32):
    """The chain with x0 AND x5 given: x5's row is a check.  (prover, lines, the row, clean starts(k, B), the oracle's program)"""
    lines = chain_lines(n)
    row = lines.index("x5 <== x4 * x4")
    bp = pa.BatchProver(setup, pa.Program(lines, n))
    bp.set_inputs(["x0", "x5"])

    def starts(k, B):
        return [{"x0": x, "x5": pow(x, 32, R_MOD)} for x in (3 + 11 * b + 1009 * k for b in range(B))]

    return bp, lines, row, starts, OProgram(lines, n)


def spoil(starts, b, oprog):
    starts = [dict(s) for s in starts]
    starts[b]["x5"] = (starts[b]["x5"] + 1) % R_MOD
    with pytest.raises(Exception, match="Failed assertion"):
        oprog.fill_variable_assignments(dict(starts[b]))
    return starts


def failing_batch_then_clean(setup):
    """Batch k fails a check in proof 1; k + 1 is staged clean before download(k): k keeps bit 4 and its row, k + 1 is all zero."""
    bp, lines, row, starts, oprog = checked_chain(setup)
    bp.upload_inputs(spoil(starts(0, 2), 1, oprog))
    bp.run()
    bp.stage_inputs(starts(1, 5))
    assert list(bp.download_raw()[1]) == [0, 16 | 4] and bp.solve_failures() == [None, row]  # before advance: batch k's
    with pytest.raises(pa.ProofError, match=r"proof 1: failed assertion at row %d \(x5 <== x4 \* x4\)" % row):
        bp.download()
    assert bp.advance() == 5
    assert bp.solve_failures() == [None] * 5  # after: batch k + 1's
    bp.run()
    assert bp.download_raw()[1] == bytes(5) and bp.solve_failures() == [None] * 5


def clean_batch_then_failing(setup):
    bp, lines, row, starts, oprog = checked_chain(setup)
    bp.upload_inputs(starts(0, 2))
    bp.run()
    bp.stage_inputs(spoil(starts(1, 5), 3, oprog))
    assert bp.download_raw()[1] == bytes(2) and bp.solve_failures() == [None, None]
    assert bp.advance() == 5
    assert bp.solve_failures() == [None, None, None, row, None]
    bp.run()
    assert list(bp.download_raw()[1]) == [0, 0, 0, 16 | 4, 0] and bp.solve_failures() == [None, None, None, row, None]


def staged_value_not_below_r(setup, n=32):
    """r itself as input 0 of proof 2 of the staged batch, then as variable 1 of proof 1 of a batch staged as packed variables: the
    resident batch's status stays 0 until advance, then PROVER_ST_BAD_INPUT is on that proof alone."""
    lines = chain_lines(n)
    bp = pa.BatchProver(setup, pa.Program(lines, n))
    bp.set_inputs(["x0"])
    V, keep = len(bp.variables), []
    assert V > 3
    clean = [{"x0": 5 + b} for b in range(3)]
    bp.upload_inputs(clean)
    bp.run()
    bp.stage_input_values_async(pinned_blob(bp, le([5, 6]) + R_MOD.to_bytes(32, "little"), keep), 3)
    assert bp.download_raw()[1] == bytes(3)
    bp.advance()
    bp.run()
    blob = bytearray(le([w[v] for w in oracle_fill(lines, n, clean) for v in bp.variables]))
    blob[32 * (V + 1):32 * (V + 2)] = R_MOD.to_bytes(32, "little")
    bp.stage_values_async(pinned_blob(bp, bytes(blob), keep), 3)
    st = bp.download_raw()[1]
    assert [s & 8 for s in st] == [0, 0, 8], list(st)
    bp.advance()
    bp.run()
    st = bp.download_raw()[1]
    assert [s & 8 for s in st] == [0, 8, 0], list(st)
    for buf in keep:
        bp.ctx.host_free(buf)


def status_stride_stays_with_its_batch(setup, n=32):
    """The index of a bad value is divided by the values per proof of ITS upload.  Resident: packed variables, r at variable 1 of
    proof 1 (index V + 1); staged from inputs (1 per proof): the resident download still names proof 1, not none.  The reverse:
    resident from inputs, r at proof 2 (index 2); staged as packed variables: still proof 2, not proof 0."""
    lines = chain_lines(n)
    bp = pa.BatchProver(setup, pa.Program(lines, n))
    bp.set_inputs(["x0"])
    V, keep = len(bp.variables), []
    clean = [{"x0": 5 + b} for b in range(3)]
    packed = le([w[v] for w in oracle_fill(lines, n, clean) for v in bp.variables])
    blob = bytearray(packed)
    blob[32 * (V + 1):32 * (V + 2)] = R_MOD.to_bytes(32, "little")
    bp.upload_values_async(pinned_blob(bp, bytes(blob), keep), 3)
    bp.run()
    assert [s & 8 for s in bp.download_raw()[1]] == [0, 8, 0]
    bp.stage_inputs(clean)
    assert [s & 8 for s in bp.download_raw()[1]] == [0, 8, 0]
    bp.advance()
    bp.run()
    assert bp.download_raw()[1] == bytes(3)
    # the reverse
    bp.upload_input_values_async(pinned_blob(bp, le([5, 6]) + R_MOD.to_bytes(32, "little"), keep), 3)
    bp.run()
    assert [s & 8 for s in bp.download_raw()[1]] == [0, 0, 8]
    bp.stage_values_async(pinned_blob(bp, packed, keep), 3)
    assert [s & 8 for s in bp.download_raw()[1]] == [0, 0, 8]
    bp.advance()
    bp.run()
    assert bp.download_raw()[1] == bytes(3)
    for buf in keep:
        bp.ctx.host_free(buf)


# ---- 3. reads go to the resident batch -----------------------------------------------------------------------------------------
def reads_go_to_the_resident_batch(setup, shared, name, mode):
    c = circuit(shared, name)
    bp = c.prover(setup)
    keep = []
    first, second = c.starts(0, 2), c.starts(1, 5)
    bp.upload_inputs([dict(s) for s in first])
    stager(bp, c, mode, keep)(1, 5)
    publics = c.program.get_public_assignments()
    for starts in (first, second):
        want = c.fill(starts)
        assert_variables(bp, want, (name, mode, len(starts)))
        assert bp.public_values() == [[w[v] % R_MOD for v in publics] for w in want] and publics
        assert bp.solve_failures() == [None] * len(starts)
        if starts is first:
            assert bp.advance() == 5
    for buf in keep:
        bp.ctx.host_free(buf)


# ---- 4. state errors -----------------------------------------------------------------------------------------------------------
def state_errors(setup, shared, n=32):
    c = circuit(shared, "chain%d" % n)
    size = ctypes.c_size_t(7)
    # before set_wiring: a prover created through the C ABI alone
    ref = c.prover(setup)
    L = ref.ctx.L
    h = ctypes.c_void_p()
    assert L.plonk_prover_create(ref.ctx.handle, ref._bases.handle, 3, bytes(32 * 8 * 8), 0, ctypes.byref(h)) == 0
    try:
        for fn in (L.plonk_prover_stage_inputs, L.plonk_prover_stage_variables):
            assert fn(h, bytes(32), 1) == ERR_STATE and b"plonk_prover_set_wiring has not been called" in L.plonk_last_error()
        assert L.plonk_prover_staged(h, ctypes.byref(size)) == 0 and size.value == 0
        assert L.plonk_prover_advance(h, ctypes.byref(size)) == ERR_STATE and b"no batch is staged" in L.plonk_last_error()
    finally:
        L.plonk_prover_destroy(h)
    bp = pa.BatchProver(setup, c.program)
    assert L.plonk_prover_stage_inputs(bp._h, bytes(32), 1) == ERR_STATE and b"plonk_prover_set_inputs has not been called" in L.plonk_last_error()
    assert L.plonk_prover_stage_inputs(bp._h, None, 1) == ERR_ARG and L.plonk_prover_stage_variables(bp._h, bytes(32), 0) == ERR_ARG
    assert L.plonk_prover_staged(bp._h, None) == ERR_ARG and L.plonk_prover_advance(bp._h, None) == ERR_ARG
    with pytest.raises(BackendError, match="advance: no batch is staged"):
        bp.advance()
    bp.set_inputs(["x0"])
    first, second, third = c.starts(0, 2), c.starts(1, 5), c.starts(2, 1)
    bp.upload_inputs(first)
    bp.stage_inputs(second)
    with pytest.raises(BackendError, match="a batch of 5 is already staged"):
        bp.stage_inputs(third)
    pinned = bp.ctx.host_alloc(32 * len(bp.variables))
    with pytest.raises(BackendError, match="a batch of 5 is already staged"):
        bp.stage_values_async(pinned, 1)
    bp.ctx.host_free(pinned)
    with pytest.raises(BackendError, match="set_inputs: a batch of 5 is staged"):
        bp.set_inputs(["x0", "x5"])
    assert bp.inputs == ("x0",)
    cells = np.ascontiguousarray(c.program.wiring_table()[1], dtype=np.uint32)
    pubs = np.zeros(1, dtype=np.uint32)
    assert L.plonk_prover_set_wiring(bp._h, cells.ctypes.data, pubs.ctypes.data, len(bp.variables)) == ERR_STATE
    assert b"set_wiring: a batch of 5 is staged" in L.plonk_last_error()
    assert bp.staged == 5
    # a plain upload between stage and advance proves its own batch, and the staged batch still advances intact
    want = references(setup, shared, c, (2, 5, 1))
    bp.upload_inputs(third)
    assert bp.staged == 5
    bp.run()
    assert proved(bp, 1) == want[2]
    assert bp.advance() == 5
    bp.run()
    assert proved(bp, 5) == want[1]
    assert_variables(bp, c.fill(second), "staged across a plain upload")
    with pytest.raises(BackendError, match="advance: no batch is staged"):
        bp.advance()
    bp.set_inputs(["x0"])  # nothing staged: a plan again, and the pipeline goes on under it
    bp.stage_inputs(first)
    assert bp.advance() == 2
    bp.run()
    assert proved(bp, 2) == want[0]


# ---- 5. sizes change under it --------------------------------------------------------------------------------------------------
def sizes_change_under_it(setup, shared, name, mode):
    """B = 5 staged behind a resident B = 1 (the staged set grows at the stage, the rounds' buffers at advance), then B = 1 behind
    the resident B = 5, then B = 5 again into the set that so far held 1; a prover destroyed with a batch staged."""
    c = circuit(shared, name)
    sizes = (1, 5, 1, 5)
    want = references(setup, shared, c, sizes)
    bp = c.prover(setup)
    keep = []
    stage = stager(bp, c, mode, keep)
    bp.upload_inputs([dict(s) for s in c.starts(0, 1)])
    for k, B in enumerate(sizes):
        bp.run()
        if k + 1 < len(sizes):
            stage(k + 1, sizes[k + 1])
        assert proved(bp, B) == want[k], (name, mode, k)
        assert_variables(bp, c.fill(c.starts(k, B)), (name, mode, k))
        if k + 1 < len(sizes):
            assert bp.advance() == sizes[k + 1]
    stage(1, 5)
    L, h = bp.ctx.L, bp._h
    bp._h = None
    assert L.plonk_prover_destroy(h) == 0  # with a batch staged and never advanced
    for buf in keep:
        bp.ctx.host_free(buf)
