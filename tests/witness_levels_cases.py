"""Bodies of the tests of the witness solver's levelised form (csrc/witness_solve.h: witness_solve_levels_kernel, one workgroup
per proof, the lanes take the rows of one dependency level at a time), shared by tests/test_emu_witness_levels.py (emulated
kernels) and tests/test_gpu_witness_levels.py (MI355X).  The checker is the oracle's fill_variable_assignments and poseidon_hash
(oracle/), never the other form of the solver — except where a case is about the two forms giving equal bytes."""
import ctypes
import re

import pytest

from helpers import R_MOD

import plonkathon_amd as pa
import witness_solve_cases as wc
from oracle.circuit import Program as OProgram
from oracle.poseidon import poseidon_hash, poseidon_program_lines
from parity_cases import chain_lines
from witness_solve_cases import CLASS_LINES, CLASS_N, CLASS_STARTS, assert_variables, oracle_fill

ERR_ARG, ERR_STATE = -1, -4
LAGRANGE_COMMITS = 1


def solve_form_option(k):
    """PLONK_PROVER_SOLVE_FORM(k) of include/plonk_hip.h."""
    return (k & 3) << 16


def braid(W, D):
    """D levels of W rows, every row reading two rows of the level before; within a level the rows stand in DESCENDING i, so that
    the order by level is not the order by row; then a check row one level deeper and `z <== 0` (level 1, empty L and R cells)."""
    lines = ["p public", "q public"]
    lines += ["c0x%d <== p * q + %d" % (i, i + 1) for i in reversed(range(W))]
    for d in range(1, D):
        lines += ["c%dx%d <== c%dx%d * c%dx%d - %d" % (d, i, d - 1, i, d - 1, (i + 7) % W, 1000 * d + i) for i in reversed(range(W))]
    lines.append("c%dx0 === c%dx0 * c%dx7 - %d" % (D - 1, D - 2, D - 2, 1000 * (D - 1)))
    lines.append("z <== 0")
    return lines


def braid_starts(B, salt=0):
    return [{"p": 3 + 1000003 * (b + salt), "q": R_MOD - 2 - 77 * b - salt} for b in range(B)]


def poseidon_multi(K):
    """K independent Poseidon hashes in one circuit: every name of copy k prefixed h{k}x, the `public` lines first."""
    public, rows = [], []
    for k in range(K):
        for line in poseidon_program_lines():
            line = re.sub(r"\b[A-Za-z][A-Za-z0-9]*\b", lambda m: m.group(0) if m.group(0) == "public" else "h%dx%s" % (k, m.group(0)), line)
            (public if line.endswith(" public") else rows).append(line)
    return public + rows


def poseidon_multi_starts(K, B):
    return [{"h%dx%s" % (k, v): 1 + 10 * b + 100 * k + (5 if v == "M0" else 0) for k in range(K) for v in ("L0", "M0")} for b in range(B)]


def braid_prover(setup, shared, W):
    """One BatchProver per braid circuit and test module, created with solve="levels"."""
    key = ("braid", W)
    if key not in shared:
        lines = braid(W, 3)
        shared[key] = (lines, OProgram(lines, 1024), pa.BatchProver(setup, pa.Program(lines, 1024), solve="levels"))
    return shared[key]


def set_form(bp, form):
    """Switch the solver's form on a live prover: it takes effect at the next input upload."""
    assert bp.ctx.L.plonk_prover_set_options(bp._h, solve_form_option(pa.BatchProver.SOLVE_FORMS[form])) == 0


def steps_of(widths, T):
    return sum(-(-w // T) for w in widths)


# ---- 1. level width against T ------------------------------------------------------------------------------------------------
def level_width_against_T(setup, shared, W):
    """braid(W, 3): with the `z <== 0` row the first level is W + 1 rows wide — exactly T for W = 255, T + 1 for W = 256 (one
    lane runs a second step), T + 45 for W = 300."""
    lines, oprog, bp = braid_prover(setup, shared, W)
    for B in (1, 3):
        starts = braid_starts(B)
        bp.upload_inputs([dict(s) for s in starts])
        plan = bp.solve_plan(B)
        assert (plan["levels"], plan["widest"], plan["threads"]) == (4, W + 1, 256)
        assert plan["steps"] == steps_of([W + 1, W, W, 1], 256)
        assert_variables(bp, oracle_fill(lines, 1024, starts, oprog), ("braid", W, B))
        assert bp.solve_failures() == [None] * B


# ---- 2. every selector class -------------------------------------------------------------------------------------------------
def every_selector_class(setup):
    """The class circuit on a FRESH prover (its first batch sizes `vars` at exactly B V elements): every variable, and z and k —
    rows with empty L and R cells — for the last proof too, whose empty cell's slot is past the buffer."""
    bp = pa.BatchProver(setup, pa.Program(CLASS_LINES, CLASS_N), solve="levels")
    bp.upload_inputs([dict(s) for s in CLASS_STARTS])
    want = oracle_fill(CLASS_LINES, CLASS_N, CLASS_STARTS)
    assert_variables(bp, want, "class, levels")
    got = bp.variable_values(["z", "k"])
    assert [g["z"] for g in got] == [0] * len(CLASS_STARTS) and [g["k"] for g in got] == [7] * len(CLASS_STARTS)
    assert bp.solve_failures() == [None] * len(CLASS_STARTS)
    plan = bp.solve_plan(len(CLASS_STARTS))
    assert plan["levels"] < plan["active_rows"] == len(CLASS_LINES) - 2 and plan["threads"] == 64


# ---- 3. width one ------------------------------------------------------------------------------------------------------------
def width_one(setup, n=32, B=5):
    lines = chain_lines(n)
    bp = pa.BatchProver(setup, pa.Program(lines, n), solve="levels")
    starts = [{"x0": 3 + 1000003 * b} for b in range(B)]
    bp.upload_inputs([dict(s) for s in starts])
    plan = bp.solve_plan(B)
    assert plan["levels"] == plan["active_rows"] == plan["steps"] == n - 1 and plan["widest"] == 1  # a barrier after every row
    assert_variables(bp, oracle_fill(lines, n, starts), ("chain, levels", n, B))
    assert bp.solve_failures() == [None] * B


# ---- 4. Poseidon at 2^10 -------------------------------------------------------------------------------------------------------
def poseidon_levels_prover(setup, shared):
    """The prover that wc.poseidon_prover hands to the Poseidon cases of witness_solve_cases: here one with forced levels."""
    if "poseidon" not in shared:
        shared["poseidon"] = pa.BatchProver(setup, wc.poseidon_program()[1], solve="levels")
    return shared["poseidon"]


def poseidon_values(setup, shared, with_hash, form="levels"):
    set_form(poseidon_levels_prover(setup, shared), form)
    wc.solved_values_poseidon(setup, shared, with_hash)


def poseidon_failing_assertion(setup, shared, form):
    """wc.failing_assertion — status bytes [0, 20, 0], solve_failures [None, row, None], proofs 0 and 2 the bytes of a clean batch —
    under the form given."""
    set_form(poseidon_levels_prover(setup, shared), form)
    wc.failing_assertion(setup, shared)


# ---- 5. the first failure in program order, not in time ------------------------------------------------------------------------
ORDER_LINES = ["a <== p * q", "b <== a * a", "c <== b * b", "e <== c * c", "f <== p + q"]


def first_failure_in_program_order(setup):
    """e and f are inputs, so rows 3 and 4 are checks: row 3 at the deepest level, row 4 at level 1, which the levelised form runs
    first.  With both wrong, both forms report row 3, as the oracle's walk does; with only f wrong, row 4."""
    p, q = 5, 11
    e, f = pow(p * q, 8, R_MOD), p + q
    oprog = OProgram(ORDER_LINES, 8)
    assert oprog.fill_variable_assignments({"p": p, "q": q, "e": e, "f": f})["c"] == pow(p * q, 4, R_MOD)
    for bad in ({"e": e + 1, "f": f + 1}, {"e": e, "f": f + 1}):
        with pytest.raises(Exception, match="Failed assertion"):
            oprog.fill_variable_assignments({"p": p, "q": q, **bad})
    for form in ("levels", "lanes"):
        bp = pa.BatchProver(setup, pa.Program(ORDER_LINES, 8), solve=form)
        bp.set_inputs(["p", "q", "e", "f"])
        plan = bp.solve_plan(1)
        assert (plan["active_rows"], plan["levels"], plan["widest"]) == (5, 4, 2)
        bp.upload_inputs([{"p": p, "q": q, "e": e + 1, "f": f + 1}, {"p": p, "q": q, "e": e, "f": f + 1}, {"p": p, "q": q, "e": e, "f": f},
                          {"p": p, "q": q, "e": e + 1, "f": f}])
        assert bp.solve_failures() == [3, 4, None, 3], form


# ---- 6. the plan query ---------------------------------------------------------------------------------------------------------
def plan_of(bp, B=1):
    plan = bp.solve_plan(B)
    return plan["active_rows"], plan["levels"], plan["widest"]


def plan_query(setup, shared):
    lines, _, bp = braid_prover(setup, shared, 300)
    bp.set_inputs(["p", "q"])
    plan = bp.solve_plan(1)
    assert plan == {"rows": len(lines), "active_rows": 902, "levels": 4, "widest": 301, "threads": 256, "steps": 7, "form": "levels"}
    # the chain: one row per level, the one-lane form for every batch
    chain = pa.BatchProver(setup, pa.Program(chain_lines(32), 32))
    L = chain.ctx.L
    out = (ctypes.c_uint32 * 7)()
    assert L.plonk_prover_solve_plan(chain._h, 1, out) == ERR_STATE  # no plan yet
    chain.set_inputs(["x0"])
    for B in (1, 64, 512):
        plan = chain.solve_plan(B)
        assert plan["levels"] == plan["active_rows"] == plan["steps"] == 31 and plan["widest"] == 1 and plan["form"] == "lanes", B
    assert L.plonk_prover_solve_plan(chain._h, 0, out) == ERR_ARG
    # a re-plan with other inputs: the numbers are the new plan's (x5 given: its row is a check beside x1's, two chains side by side)
    chain.set_inputs(["x0", "x5"])
    assert plan_of(chain) == (31, 26, 2)
    chain.set_inputs(["x0"])
    assert plan_of(chain) == (31, 31, 1)
    # Poseidon: 1 009 active rows in 448 levels, with M64 assigned or checked
    pos = wc.poseidon_prover(setup, shared)
    pos.set_inputs(["L0", "M0"])
    assert plan_of(pos) == (1009, 448, 4) and pos.solve_plan(1)["threads"] == 64
    pos.set_inputs(["L0", "M0", "M64"])
    assert plan_of(pos) == (1009, 448, 4)


def plan_query_poseidon_multi(setup, K=2):
    lines = poseidon_multi(K)
    bp = pa.BatchProver(setup, pa.Program(lines, 1024 * K))
    bp.set_inputs(list(poseidon_multi_starts(K, 1)[0]))
    assert plan_of(bp) == (1009 * K, 448, 4 * K)
    return bp, lines


# ---- 7. options ----------------------------------------------------------------------------------------------------------------
def options(setup):
    program = pa.Program(CLASS_LINES, CLASS_N)
    bp = pa.BatchProver(setup, program)
    L = bp.ctx.L
    assert L.plonk_prover_set_options(bp._h, solve_form_option(3)) == ERR_ARG
    assert L.plonk_prover_set_options(bp._h, solve_form_option(2) | LAGRANGE_COMMITS | ((1 + 1) << 8)) == 0  # with 2 segments
    assert L.plonk_prover_set_options(bp._h, 1 << 12) == ERR_ARG
    assert L.plonk_prover_set_options(bp._h, solve_form_option(2) | 2) == ERR_ARG  # bit 1
    assert L.plonk_prover_set_options(bp._h, 1 << 18) == ERR_ARG
    assert L.plonk_prover_set_options(bp._h, 0) == 0
    with pytest.raises(ValueError):
        pa.BatchProver(setup, program, solve="nonsense")
    # the form switched between two uploads on one prover: the same variables both times, the oracle's
    want = oracle_fill(CLASS_LINES, CLASS_N, CLASS_STARTS)
    for form in ("levels", "lanes", "levels", None):
        set_form(bp, form)
        bp.upload_inputs([dict(s) for s in CLASS_STARTS])
        assert_variables(bp, want, ("class", form))


# ---- GPU only ------------------------------------------------------------------------------------------------------------------
def proof_bytes(setup):
    """poseidon_multi(2) at 2^11: the 768-byte records of the two forms are equal, every status 0, the public values are the inputs
    and the two hashes, and each proof verifies with its own public values only."""
    K, n, B = 2, 2048, 2
    lines = poseidon_multi(K)
    program = pa.Program(lines, n)
    starts = poseidon_multi_starts(K, B)
    raws = {}
    for form in ("levels", "lanes"):
        bp = pa.BatchProver(setup, program, solve=form)
        proofs = bp.prove_inputs([dict(s) for s in starts])
        raws[form], st = bp.download_raw()
        assert st == bytes(B), (form, list(st))
    assert raws["levels"] == raws["lanes"] and len(raws["levels"]) == 768 * B and raws["levels"][:768] != raws["levels"][768:]
    pubs = bp.public_values()
    names = program.get_public_assignments()
    assert names == ["h%dx%s" % (k, v) for k in range(K) for v in ("L0", "M0", "M64")]
    hashes = [[poseidon_hash(s["h%dxL0" % k], s["h%dxM0" % k]) for k in range(K)] for s in starts]
    assert pubs == [[x for k in range(K) for x in (s["h%dxL0" % k], s["h%dxM0" % k], h[k])] for s, h in zip(starts, hashes)]
    vk = setup.verification_key(program.common_preprocessed_input())
    for b in range(B):
        assert vk.verify_proof(n, proofs[b], pubs[b])
        assert not vk.verify_proof(n, proofs[b], pubs[1 - b])


def two_async_batches_back_to_back(setup, shared, B=5):
    """The pattern of wc.two_async_batches_back_to_back on braid(300, 3) with forced levels: the second copy stays behind the first
    batch's read of the staging buffer, the second solve behind the first batch's gathers."""
    lines, oprog, ref = braid_prover(setup, shared, 300)
    starts = [braid_starts(B), braid_starts(B, salt=9)]
    want = []
    for s in starts:
        ref.upload_inputs([dict(d) for d in s])
        assert_variables(ref, oracle_fill(lines, 1024, s, oprog), "braid, synchronous")
        ref.run()
        raw, st = ref.download_raw()
        assert st == bytes(B)
        want.append(raw)
    assert want[0] != want[1]
    bp = pa.BatchProver(setup, ref.program, solve="levels")
    bp.set_inputs(["p", "q"])
    ctx = bp.ctx
    pinned = []
    for s in starts:
        blob = b"".join(int(d[k]).to_bytes(32, "little") for d in s for k in bp.inputs)
        buf = ctx.host_alloc(len(blob))
        buf[: len(blob)] = blob
        pinned.append(buf)
    bp.upload_input_values_async(pinned[0], B)
    bp.run()
    assert bp.download_raw() == (want[0], bytes(B))
    bp.upload_input_values_async(pinned[0], B)  # no host wait between these
    bp.run()
    bp.upload_input_values_async(pinned[1], B)
    bp.run()
    assert bp.download_raw() == (want[1], bytes(B))
    assert_variables(bp, oracle_fill(lines, 1024, starts[1], oprog), "braid, asynchronous")
    bp.upload_input_values_async(pinned[0], B)
    bp.run()
    assert bp.download_raw() == (want[0], bytes(B))
    for buf in pinned:
        ctx.host_free(buf)


def grid_geometry(setup, shared, B):
    """One workgroup per proof: B proofs with distinct inputs, every variable of the first and the last, c2x0 of every proof.  The
    inputs are this case's own (salt): values that an earlier case left in the shared prover's buffer cannot satisfy it."""
    lines, oprog, bp = braid_prover(setup, shared, 300)
    starts = braid_starts(B, salt=100 + B)
    bp.upload_inputs([dict(s) for s in starts])
    want = oracle_fill(lines, 1024, starts, oprog)
    got = bp.variable_values()
    for b in {0, B - 1}:
        for v in bp.variables:
            assert got[b][v] == want[b][v] % R_MOD, (B, b, v)
    assert [g["c2x0"] for g in got] == [w["c2x0"] % R_MOD for w in want]
    assert len({g["c2x0"] for g in got}) == B
    assert bp.solve_failures() == [None] * B


def above_2_11(setup_8192):
    """poseidon_multi(8) at 2^13, B = 2, the automatic rule: it only solves, nothing is proved."""
    K, n, B = 8, 8192, 2
    lines = poseidon_multi(K)
    bp = pa.BatchProver(setup_8192, pa.Program(lines, n))
    starts = poseidon_multi_starts(K, B)
    bp.upload_inputs([dict(s) for s in starts])
    assert plan_of(bp, B) == (8072, 448, 32)
    want = oracle_fill(lines, n, starts)
    assert len(want[0]) == 8089 and len(bp.variables) == 8088  # the oracle's fill carries the empty cell's None beside the variables
    for b in range(B):
        for k in range(K):
            assert want[b]["h%dxM64" % k] == poseidon_hash(starts[b]["h%dxL0" % k], starts[b]["h%dxM0" % k])
    assert_variables(bp, want, "poseidon x8")
    assert bp.solve_failures() == [None] * B
