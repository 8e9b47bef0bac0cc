"""Bodies of the witness solver's tests (csrc/witness_solve.h: a batch proved from the circuit's input values alone), shared by
tests/test_emu_witness_solve.py (emulated kernels) and tests/test_gpu_witness_solve.py (MI355X).  The checker is the oracle's
fill_variable_assignments (oracle/circuit.py) and the committed fixtures, never the code under test."""
import ctypes

import pytest

from helpers import R_MOD, load

import plonkathon_amd as pa
from oracle.circuit import Program as OProgram
from oracle.poseidon import poseidon_hash, poseidon_program_lines
from parity_cases import PTAU, assert_matches_fixture, chain_lines, fixture_case, flat  # noqa: F401

ERR_ARG, ERR_STATE = -1, -4

FACTORISATION = ["e public", "c <== a * b", "e <== c * d"]
# Every selector class (0, +1, -1, general) for each of QL, QR, QM and QC; a negated output (-d), two === rows, L = R rows (g, j),
# constant-only rows with empty L / R cells (k, z: z is the LAST active row), the "- 45 * x" sign rule (e, f).
CLASS_LINES = [
    "p public", "q public", "k <== 7", "a <== p * q", "b <== p + q", "c <== p - q", "-d <== a * b + 5",
    "e <== a * 3 - 45 * b * a + b", "f <== 9 - 45 * e", "g <== e * e - e - 1", "h <== -g * f - f", "a === p * q",
    "i <== h - 1 * k", "j <== 2 * i - 3 * i * h - 11", "m <== -p", "b === q + p", "z <== 0",
]
CLASS_N = 32
CLASS_STARTS = [{"p": 5, "q": R_MOD - 2}, {"p": R_MOD - 1, "q": 0}, {"p": 0x1234567890ABCDEF << 180, "q": 77}]

_poseidon = {}


def poseidon_program():
    """(lines, plonkathon_amd Program, oracle Program) of the Poseidon circuit at 2^10, once per process."""
    if not _poseidon:
        lines = poseidon_program_lines()
        _poseidon["v"] = (lines, pa.Program(lines, 1024), OProgram(lines, 1024))
    return _poseidon["v"]


def poseidon_prover(setup, shared):
    """The Poseidon circuit's BatchProver, built once per test module (`shared`: a module-scoped dict) and re-planned by every
    set_inputs: its construction is most of what a Poseidon case costs on the emulated kernels."""
    if "poseidon" not in shared:
        shared["poseidon"] = pa.BatchProver(setup, poseidon_program()[1])
    return shared["poseidon"]


def poseidon_starts(B, with_hash=False):
    starts = [{"L0": 1 + 10 * b, "M0": 2 + 7 * b} for b in range(B)]
    if with_hash:
        for s in starts:
            s["M64"] = poseidon_hash(s["L0"], s["M0"])
    return starts


def oracle_fill(lines, n, starts, oprog=None):
    oprog = oprog or OProgram(lines, n)
    return [oprog.fill_variable_assignments(dict(s)) for s in starts]


def assert_variables(bp, wants, tag):
    """variable_values() of the resident batch against the oracle's fill, on every variable of the circuit."""
    got = bp.variable_values()
    assert len(got) == len(wants)
    for b, (g, w) in enumerate(zip(got, wants)):
        assert set(g) == set(bp.variables)
        for v in bp.variables:
            assert g[v] == w[v] % R_MOD, (tag, b, v)


# ---- 1. solved values ------------------------------------------------------------------------------------------------------
def solved_values(setup, lines, n, starts, tag, oprog=None, bp=None):
    if bp is None:
        bp = pa.BatchProver(setup, pa.Program(lines, n))
    else:
        bp.set_inputs(list(starts[0]))
    bp.upload_inputs([dict(s) for s in starts])
    assert_variables(bp, oracle_fill(lines, n, starts, oprog), tag)
    return bp


def solved_values_class(setup):
    solved_values(setup, CLASS_LINES, CLASS_N, CLASS_STARTS, "class")


def solved_values_factorisation(setup):
    solved_values(setup, FACTORISATION, 8, [{"a": 3, "b": 4, "d": 5}], "factorisation")
    solved_values(setup, FACTORISATION, 8, [{"a": 3, "b": 4, "d": 5, "e": 60}], "factorisation with e")


def solved_values_chain(setup, n=32, B=5):
    solved_values(setup, chain_lines(n), n, [{"x0": 3 + 1000003 * b} for b in range(B)], ("chain", n, B))


def solved_values_poseidon(setup, shared, with_hash):
    lines, program, oprog = poseidon_program()
    bp = solved_values(setup, lines, 1024, poseidon_starts(2, with_hash), ("poseidon", with_hash), oprog, poseidon_prover(setup, shared))
    assert bp.solve_failures() == [None, None]


# ---- 2. the empty-cell rule at the end of the buffer -------------------------------------------------------------------------
def empty_cells_at_the_end_of_the_buffer(setup):
    """The class circuit's last active row, `z <== 0`, has empty L and R cells: their index is V, and for the last proof of a
    batch vars + (B - 1) V + V is the end of a buffer that a fresh prover allocates at exactly B V elements.  The rule (an empty cell
    reads as zero without a load) is checked by value here: z and k of every proof, the last one included."""
    program = pa.Program(CLASS_LINES, CLASS_N)
    assert program.wires()[-1].as_list() == [None, None, "z"] and program.wires()[2].as_list() == [None, None, "k"]
    V = len(program.wiring_table()[0])
    assert int(program.wiring_table()[1][0, len(CLASS_LINES) - 1]) == V  # the empty cell's index
    B = len(CLASS_STARTS)
    bp = pa.BatchProver(setup, program)  # fresh: its first batch sizes `vars`
    bp.upload_inputs([dict(s) for s in CLASS_STARTS])
    got = bp.variable_values(["z", "k", "m"])
    want = oracle_fill(CLASS_LINES, CLASS_N, CLASS_STARTS)
    assert [g["z"] for g in got] == [0] * B and [g["k"] for g in got] == [7] * B
    assert got[B - 1]["m"] == want[B - 1]["m"] == (-CLASS_STARTS[B - 1]["p"]) % R_MOD
    assert_variables(bp, want, "class, end of buffer")


# ---- 3. proof bytes ------------------------------------------------------------------------------------------------------
def proof_bytes_equal_filled_witnesses(setup, n=128, B=2):
    lines = chain_lines(n)
    starts = [{"x0": 3 + 4 * b} for b in range(B)]
    program = pa.Program(lines, n)
    a, b = pa.BatchProver(setup, program), pa.BatchProver(setup, program)
    a.upload([dict(w) for w in oracle_fill(lines, n, starts)])
    a.run()
    want, st = a.download_raw()
    assert st == bytes(B)
    proofs = b.prove_inputs(starts)
    got, st = b.download_raw()  # the same resident batch, as raw records with their status bytes
    assert st == bytes(B), list(st)
    assert got == want and len(got) == 768 * B and got[:768] != got[768:]
    assert [flat(p) for p in proofs] == [flat(pa.BatchProver.decode(want[768 * i:768 * (i + 1)])) for i in range(B)]


def prove_inputs_matches_fixture(setup, name):
    """prove_inputs(case["start"]) against tests/golden/oracle_proofs.json: the proof and the six challenges."""
    case, lines = fixture_case(name)
    assert "srs_tau" not in case
    bp = pa.BatchProver(setup, pa.Program(lines, case["group_order"]))
    start = {k: int(v) for k, v in case["start"].items()}
    for i, proof in enumerate(bp.prove_inputs([dict(start)])):
        assert_matches_fixture(flat(proof), case, i)
        for k, v in bp.challenges(i).items():
            assert str(v.n) == case["challenges"][k], (name, i, k)


# ---- 4. a failing assertion --------------------------------------------------------------------------------------------------
def failing_assertion(setup, shared):
    """Poseidon, three proofs from {L0, M0, M64}, proof 1 given M64 + 1: the row that assigns M64 is a check and fails there.
    Proofs 0 and 2 are the records of a clean batch of those two witnesses."""
    lines, program, oprog = poseidon_program()
    starts = poseidon_starts(3, with_hash=True)
    bp = poseidon_prover(setup, shared)
    bp.set_inputs(["L0", "M0", "M64"])
    bp.upload_inputs([dict(starts[0]), dict(starts[2])])
    bp.run()
    clean_raw, st = bp.download_raw()
    assert st == bytes(2), list(st)
    starts[1]["M64"] = (starts[1]["M64"] + 1) % R_MOD
    row = [i for i, l in enumerate(lines) if l.startswith("M64 <== ")]
    assert len(row) == 1
    row = row[0]
    with pytest.raises(Exception, match="Failed assertion"):
        oprog.fill_variable_assignments(dict(starts[1]))
    bp.upload_inputs([dict(s) for s in starts])
    bp.run()
    raw, st = bp.download_raw()
    assert list(st) == [0, 16 | 4, 0]
    assert bp.solve_failures() == [None, row, None]
    # the gate check sees the same row: with the values the solver left, the gate identity fails on `row` and nowhere else
    w = bp.variable_values()[1]
    w[None] = 0
    QL, QR, QM, QO, QC = program.gate_columns()
    pubs = [w[v] for v in program.get_public_assignments()]
    failing = []
    for i, wires in enumerate(program.wires()):
        a, b, c = (w[x] for x in wires.as_list())
        pi = -pubs[i] if i < len(pubs) else 0
        if (QL[i] * a + QR[i] * b + QM[i] * a * b + QO[i] * c + QC[i] + pi) % R_MOD:
            failing.append(i)
    assert failing == [row]
    with pytest.raises(pa.ProofError, match=r"proof 1: failed assertion at row %d \(M64 <== " % row):
        bp.download()
    assert raw[:768] == clean_raw[:768] and raw[2 * 768:] == clean_raw[768:] and clean_raw[:768] != clean_raw[768:]


# ---- 5. plan refusals ------------------------------------------------------------------------------------------------------
def plan_refusals(setup):
    program = pa.Program(FACTORISATION, 8)
    bp = pa.BatchProver(setup, program)
    L = bp.ctx.L
    # nothing to solve with yet
    assert L.plonk_prover_upload_inputs(bp._h, bytes(96), 1) == ERR_STATE
    pinned = bp.ctx.host_alloc(96)
    assert L.plonk_prover_upload_inputs_async(bp._h, ctypes.addressof(pinned), 1) == ERR_STATE
    bp.ctx.host_free(pinned)
    with pytest.raises(KeyError) as e:
        bp.set_inputs(["a", "b"])
    assert e.value.args == ("d",)
    with pytest.raises(KeyError):  # the oracle names the same variable
        OProgram(FACTORISATION, 8).fill_variable_assignments({"a": 3, "b": 4})
    assert L.plonk_prover_upload_inputs(bp._h, bytes(64), 1) == ERR_STATE  # a refused plan is no plan
    with pytest.raises(AssertionError, match="second time"):
        bp.set_inputs(["a", "b", "d", "a"])
    missing = ctypes.c_uint32(5)
    idx = (ctypes.c_uint32 * 3)(0, 1, 99)
    assert L.plonk_prover_set_inputs(bp._h, idx, 3, ctypes.byref(missing)) == ERR_ARG and missing.value == 0xFFFFFFFF
    # an unknown extra name is dropped
    bp.set_inputs(["a", "nonsense", "b", "d"])
    assert bp.inputs == ("a", "b", "d")
    bp.upload_inputs([{"a": 3, "b": 4, "d": 5, "nonsense": 1}])
    assert bp.variable_values() == [{"a": 3, "b": 4, "c": 12, "d": 5, "e": 60}]
    with pytest.raises(KeyError):
        bp.upload_inputs([{"a": 3, "b": 4, "d": 5}, {"a": 3, "b": 4}])
    # the first upload_inputs sets the inputs from the first dict's keys that are variables
    bp2 = pa.BatchProver(setup, program)
    bp2.upload_inputs([{"other": 9, "d": 5, "b": 4, "a": 3}, {"a": 1, "b": 2, "d": 3}])
    assert bp2.inputs == ("d", "b", "a")
    assert bp2.public_values() == [[60], [6]]
    # a variable that no row assigns and that is not given: y (a public row is not solved), and u (never an output)
    never = pa.BatchProver(setup, pa.Program(["y public", "c <== a * b"], 8))
    with pytest.raises(KeyError) as e:
        never.set_inputs(["a", "b"])
    assert e.value.args == ("y",)
    reads = pa.BatchProver(setup, pa.Program(["c <== a * b", "d <== c * u"], 8))
    with pytest.raises(KeyError) as e:
        reads.set_inputs(["a", "b"])
    assert e.value.args == ("u",)
    # before set_wiring: a prover created through the C ABI alone
    h = ctypes.c_void_p()
    sel = bytes(32 * 8 * 8)
    assert L.plonk_prover_create(bp.ctx.handle, bp._bases.handle, 3, sel, 0, ctypes.byref(h)) == 0
    try:
        assert L.plonk_prover_upload_inputs(h, bytes(32), 1) == ERR_STATE
        idx = (ctypes.c_uint32 * 1)(0)
        assert L.plonk_prover_set_inputs(h, idx, 1, ctypes.byref(missing)) == ERR_STATE
    finally:
        L.plonk_prover_destroy(h)


# ---- 6. non-canonical input ------------------------------------------------------------------------------------------------
def non_canonical_inputs(setup):
    program = pa.Program(CLASS_LINES, CLASS_N)
    bp = pa.BatchProver(setup, program)
    bp.set_inputs(["p", "q"])
    le = lambda vals: b"".join(int(v).to_bytes(32, "little") for v in vals)
    B, K, V = 3, 2, len(bp.variables)
    assert V > B * K  # so that a divisor left at n_vars would name proof 0
    bad = le([5, 6, 7, 8, 9, R_MOD])  # proof 2, input 1: r itself
    with pytest.raises(AssertionError, match="canonical"):
        bp.upload_input_values(bad, B)
    assert bp.ctx.L.plonk_prover_run(bp._h, B) == ERR_STATE  # no batch is resident after the refusal
    pinned = bp.ctx.host_alloc(32 * B * V)
    pinned[: len(bad)] = bad
    bp.upload_input_values_async(pinned, B)
    bp.run()
    assert list(bp.download_raw()[1]) == [0, 0, 8]
    # the existing asynchronous upload still names the proof it always did
    wits = oracle_fill(CLASS_LINES, CLASS_N, [{"p": 5, "q": 6}, {"p": 7, "q": 8}, {"p": 9, "q": 10}])
    blob = bytearray(le([w[v] for w in wits for v in bp.variables]))
    blob[32 * (V + 1):32 * (V + 2)] = R_MOD.to_bytes(32, "little")  # proof 1, variable 1
    pinned[: len(blob)] = bytes(blob)
    bp.upload_values_async(pinned, B)
    bp.run()
    st = bp.download_raw()[1]
    assert st[1] & 8 and not st[0] & 8 and not st[2] & 8, list(st)
    bp.ctx.host_free(pinned)


# ---- 7. existing uploads unchanged -------------------------------------------------------------------------------------------
def existing_uploads_unchanged(setup):
    """A prove_inputs batch with a failed check, then the K6 witness through prove_batch on the same prover: the golden proof, its
    compressed bytes, and no status bit left over."""
    k6 = load("k6_proof.json")
    assert k6["program"] == FACTORISATION
    wit = {k: int(v) for k, v in k6["witness"].items()}
    bp = pa.BatchProver(setup, pa.Program(k6["program"], k6["group_order"]))
    bp.upload_inputs([{"a": 3, "b": 4, "d": 5, "e": 61}, {"a": 3, "b": 4, "d": 5, "e": 60}])
    bp.run()
    raw, st = bp.download_raw()
    assert list(st) == [16 | 4, 0] and bp.solve_failures() == [2, None]
    with pytest.raises(pa.ProofError, match=r"proof 0: failed assertion at row 2 \(e <== c \* d\)"):
        bp.download()
    want = bytes.fromhex(load("k6_proof_bytes.json")["hex"])
    assert pa.BatchProver.decode(raw[768:]).to_bytes() == want
    bp.upload([dict(wit), dict(wit)])
    bp.run()
    raw2, st = bp.download_raw()
    assert st == bytes(2) and bp.solve_failures() == [None, None]
    assert raw2[:768] == raw[768:] and raw2[768:] == raw[768:]
    comp, st = bp.download_compressed()
    assert st == bytes(2) and comp[:480] == want and comp[480:] == want
    bp._upload_columns([dict(wit)])  # the column upload after a failed solve inherits nothing either
    bp.run()
    raw3, st = bp.download_raw()
    assert st == bytes(1) and raw3 == raw[768:]
    assert bp.ctx.L.plonk_prover_download_variables(bp._h, 1, None, 0, ctypes.create_string_buffer(32 * 5)) == ERR_STATE


# ---- 8. batch sizes and upload kinds change on one prover -------------------------------------------------------------------
def batch_sizes_change_between_uploads(setup, n=32):
    """One prover of the chain circuit: B = 2 from inputs, B = 5 from packed variable values, B = 1 from wire columns, B = 5 from
    inputs asynchronously out of a page-locked buffer.  Every buffer grows once (`vars`, `inputs`, the segments' scratch, the batch),
    a smaller batch then reuses the larger buffers, and the two staging buffers hand over to each other.  After each upload the
    proof and status bytes are those of a fresh prover given the same batch."""
    lines = chain_lines(n)
    program = pa.Program(lines, n)
    starts = [[{"x0": 3 + 11 * b} for b in range(2)], [{"x0": 500 + 7 * b} for b in range(5)], [{"x0": 90001}],
              [{"x0": 77 + 1000003 * b} for b in range(5)]]
    wits = [oracle_fill(lines, n, s) for s in starts]
    le = lambda vals: b"".join(int(v % R_MOD).to_bytes(32, "little") for v in vals)

    def proved(bp, B):
        bp.run()
        raw, st = bp.download_raw()
        assert st == bytes(B) and len(raw) == 768 * B
        return raw, st

    def fresh(upload):
        ref = pa.BatchProver(setup, program)
        B = upload(ref)
        return proved(ref, B)

    def from_inputs(s):
        return lambda q: (q.upload_inputs([dict(d) for d in s]), len(s))[1]

    def from_values(w):
        return lambda q: (q.upload_values(le([x[v] for x in w for v in q.variables]), len(w)), len(w))[1]

    def from_columns(w):
        return lambda q: (q._upload_columns([dict(x) for x in w]), len(w))[1]

    bp = pa.BatchProver(setup, program)
    seen = []
    for step, upload in enumerate([from_inputs(starts[0]), from_values(wits[1]), from_columns(wits[2])]):
        B = upload(bp)
        got = proved(bp, B)
        assert got == fresh(upload), step
        seen.append(got[0])
        if step == 2:  # wire columns: no solver verdicts, no variable values
            assert bp.solve_failures() == [None]
            assert bp.ctx.L.plonk_prover_download_variables(bp._h, 1, None, 0, ctypes.create_string_buffer(32 * len(bp.variables))) == ERR_STATE
        else:
            assert_variables(bp, wits[step], ("sizes", step))
    assert bp.inputs == ("x0",)
    blob = le([d["x0"] for d in starts[3]])
    pinned = bp.ctx.host_alloc(len(blob))
    pinned[: len(blob)] = blob
    bp.upload_input_values_async(pinned, 5)
    got = proved(bp, 5)
    assert got == fresh(from_inputs(starts[3]))
    assert_variables(bp, wits[3], ("sizes", 3))
    assert bp.solve_failures() == [None] * 5
    bp.ctx.host_free(pinned)
    seen.append(got[0])
    assert len(set(seen)) == 4 and seen[1] != seen[3]  # four different batches


# ---- GPU only ----------------------------------------------------------------------------------------------------------------
def lane_geometry(setup, B, n=32):
    """One lane per proof in 64-lane workgroups: B proofs with distinct x0, every variable of every proof."""
    solved_values_chain(setup, n, B)


def two_async_batches_back_to_back(setup, n=128, B=5):
    lines = chain_lines(n)
    program = pa.Program(lines, n)
    starts = [[{"x0": 3 + b} for b in range(B)], [{"x0": 1000 + 7 * b} for b in range(B)]]
    ref = pa.BatchProver(setup, program)
    want = []
    for s in starts:
        ref.upload_inputs(s)
        ref.run()
        raw, st = ref.download_raw()
        assert st == bytes(B)
        want.append(raw)
    assert want[0] != want[1]
    bp = pa.BatchProver(setup, program)
    bp.set_inputs(["x0"])
    ctx = bp.ctx
    pinned = []
    for s in starts:
        blob = b"".join(int(d["x0"]).to_bytes(32, "little") for d in s)
        buf = ctx.host_alloc(len(blob))
        buf[: len(blob)] = blob
        pinned.append(buf)
    bp.upload_input_values_async(pinned[0], B)
    bp.run()
    assert bp.download_raw() == (want[0], bytes(B))
    # no host wait between these: the second copy must stay behind the first batch's read of the staging buffer, and the second
    # solve behind the first batch's gathers
    bp.upload_input_values_async(pinned[0], B)
    bp.run()
    bp.upload_input_values_async(pinned[1], B)
    bp.run()
    assert bp.download_raw() == (want[1], bytes(B))
    bp.upload_input_values_async(pinned[0], B)
    bp.run()
    assert bp.download_raw() == (want[0], bytes(B))
    for buf in pinned:
        ctx.host_free(buf)


def public_values_feed_the_verifier(setup, shared):
    """The Poseidon hash M64 is a public input that the solver computes: public_values() returns it, a subset download names it,
    and the proofs verify with those public values (and not with another hash)."""
    lines, program, _ = poseidon_program()
    starts = poseidon_starts(2)
    bp = poseidon_prover(setup, shared)
    bp.set_inputs(["L0", "M0"])
    proofs = bp.prove_inputs(starts)
    pubs = bp.public_values()
    assert pubs == [[s["L0"], s["M0"], poseidon_hash(s["L0"], s["M0"])] for s in starts]
    sub = bp.variable_values(["M64", "L0", "R0"])
    assert [list(d.items()) for d in sub] == [[("M64", p[2]), ("L0", p[0]), ("R0", 0)] for p in pubs]
    vk = setup.verification_key(program.common_preprocessed_input())
    for proof, pub in zip(proofs, pubs):
        assert vk.verify_proof(1024, proof, pub)
    assert not vk.verify_proof(1024, proofs[0], pubs[1])
