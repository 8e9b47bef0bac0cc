"""`BatchProver` — many proofs of one circuit in lock-step, entirely GPU-resident.

The throughput form of /root/reference/prover.py's `Prover`: same constructor arguments
(`setup`, `program`), `prove(witness)` for one proof and `prove_batch(witnesses)` for many; returns
the same `Proof` objects.  All five rounds and the Fiat-Shamir transcript run on the device
(plonk_prover_* in include/plonk_hip.h), with one host synchronisation per batch.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check
from .backend import get_context
from .circuit import Program
from .field import Fq, R_MOD, Scalar
from .fiat_shamir import Message1, Message2, Message3, Message4, Message5
from .kzg import Setup
from .plonk import Proof
from .polynomial import _log2_exact


class ProofError(AssertionError):
    """The witness does not satisfy the circuit (the reference's in-prover asserts fail)."""


def _le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


try:  # host-side marshalling helper (csrc/pyext/pypack.c, built by __graft_entry__.build()); same bytes either way
    from ._pypack import pack_dicts_le32 as _pack_witnesses
except ImportError:  # pragma: no cover - pure-Python equivalent of the packer (not a compute fallback)
    def _pack_witnesses(witnesses, keys, modulus):
        return b"".join([(int(w[k]) % modulus).to_bytes(32, "little") for w in witnesses for k in keys])


def _selector_bytes(program):
    """QM, QL, QR, QO, QC, S1, S2, S3 of a circuit as plonk_prover_create takes them"""
    L, R, M, O, C = program.gate_columns()
    sigma = program.permutation_columns()
    return _le(M) + _le(L) + _le(R) + _le(O) + _le(C) + _le(sigma[1]) + _le(sigma[2]) + _le(sigma[3])


class _LockStepProver:
    """What the two provers share: a plonk_prover handle, its options, the blinders, the run and the forms proofs come back in."""

    SOLVE_FORMS = {None: 0, "lanes": 1, "levels": 2}  # PLONK_PROVER_SOLVE_FORM

    BLINDING = 1 << 20  # PLONK_PROVER_BLINDING

    @staticmethod
    def _check_blinding(blinding):
        if not isinstance(blinding, (bool, bytes, bytearray)) or (not isinstance(blinding, bool) and len(blinding) != 32):
            raise ValueError("blinding must be False, True or a 32-byte seed")

    def _set_options(self, lagrange_commits, segments, solve, blinding):
        """once the handle exists: the option bits, and the seed of a blinding prover"""
        flags = 1 if lagrange_commits else 0
        if segments is not None:
            if segments < 1 or segments & (segments - 1):
                raise ValueError("segments must be a power of two")
            flags |= min(segments.bit_length(), 15) << 8  # k + 1 in bits 8-11; the library checks the range
        flags |= self.SOLVE_FORMS[solve] << 16
        self.blinding = blinding is not False
        if self.blinding:
            flags |= self.BLINDING
        if flags:
            check(self.ctx.L.plonk_prover_set_options(self._h, flags))
        if self.blinding:
            check(self.ctx.L.plonk_prover_seed_blinders(self._h, os.urandom(32) if blinding is True else bytes(blinding)))

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.L.plonk_prover_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def segments_for(self, B):
        """The number of segments per proof a batch of B runs its per-proof scans in when `segments` was not given."""
        out = ctypes.c_uint(0)
        check(self.ctx.L.plonk_prover_plan_segments(self.ctx.handle, _log2_exact(self.group_order), B, ctypes.byref(out)))
        return out.value

    # ---- proving --------------------------------------------------------------------------------
    def set_blinders(self, blinders):
        """Explicit blinders for the NEXT run instead of the seed's: a list of proofs, each a list of eleven integers below r (b[0..10]
        of csrc/prover_blind.h), or the same as [B][11] 32-byte little-endian values.  The run must be of that many proofs."""
        if not isinstance(blinders, (bytes, bytearray)):
            if any(len(row) != 11 for row in blinders):
                raise ValueError("set_blinders: eleven blinders per proof")
            blinders = b"".join(int(v).to_bytes(32, "little") for row in blinders for v in row)
        if not blinders or len(blinders) % (11 * 32):
            raise ValueError("set_blinders: expected a multiple of %d bytes" % (11 * 32))
        check(self.ctx.L.plonk_prover_set_blinders(self._h, bytes(blinders), len(blinders) // (11 * 32)))

    def run(self, B=None):
        """Enqueue the five rounds for the resident witnesses (asynchronous)."""
        B = self._resident if B is None else B
        check(self.ctx.L.plonk_prover_run(self._h, B))

    def download_raw(self, B=None):
        B = self._resident if B is None else B
        out = ctypes.create_string_buffer(768 * B)
        status = ctypes.create_string_buffer(B)
        check(self.ctx.L.plonk_prover_download(self._h, B, out, status))
        return out.raw, status.raw[:B]

    def download_compressed(self, B=None):
        """The resident batch's proofs as 480-byte records (Proof.to_bytes' form: nine compressed commitments, six
        big-endian evaluations), packed on the device, + the status bytes of download_raw."""
        B = self._resident if B is None else B
        out = ctypes.create_string_buffer(480 * B)
        status = ctypes.create_string_buffer(B)
        check(self.ctx.L.plonk_prover_download_compressed(self._h, B, out, status))
        return out.raw, status.raw[:B]

    def download(self, B=None):
        raw, status = self.download_raw(B)
        proofs = []
        for b, st in enumerate(status):
            if st & 8:
                raise ProofError("proof %d: an uploaded witness value is not a canonical Fr value (>= r)" % b)
            if st & 16:
                row = self.solve_failures(len(status))[b]
                raise ProofError("proof %d: failed assertion at row %d (%s): the value given for its output is not the one "
                                 "the row computes (compiler/program.py:185-186)" % (b, row, getattr(self.program, "source", {row: "?"})[row]))
            if st & 4:
                raise ProofError("proof %d: witness does not satisfy the gate constraints "
                                 "(prover.py:108-116, checked row by row; it is what the quotient-degree assert of prover.py:205-208 detects)" % b)
            if st & 2:
                raise ProofError("proof %d: permutation accumulator does not close to 1 (prover.py:132)" % b)
            if st & 1:
                raise ProofError("proof %d: a commitment is the identity; the reference's transcript "
                                 "cannot absorb it (transcript.py:65-67)" % b)
            proofs.append(self.decode(raw[768 * b : 768 * (b + 1)]))
        return proofs

    @staticmethod
    def decode(blob):
        def pt(i):
            o = 64 * i
            return (Fq(int.from_bytes(blob[o : o + 32], "little")), Fq(int.from_bytes(blob[o + 32 : o + 64], "little")))

        def sc(i):
            o = 576 + 32 * i
            return Scalar(int.from_bytes(blob[o : o + 32], "little"))

        return Proof(
            Message1(pt(0), pt(1), pt(2)),
            Message2(pt(3)),
            Message3(pt(4), pt(5), pt(6)),
            Message4(sc(0), sc(1), sc(2), sc(3), sc(4), sc(5)),
            Message5(pt(7), pt(8)),
        )

    def challenges(self, b=0):
        out = ctypes.create_string_buffer(192)
        check(self.ctx.L.plonk_prover_challenges(self._h, b, out))
        names = ("beta", "gamma", "alpha", "fft_cofactor", "zeta", "v")
        return {k: Scalar(int.from_bytes(out.raw[32 * i : 32 * i + 32], "little")) for i, k in enumerate(names)}


class BatchProver(_LockStepProver):
    def __init__(self, setup: Setup, program: Program, ctx=None, lagrange_commits=False, segments=None, solve=None, blinding=False):
        """`ctx`: the Context (HIP stream) to run on; several BatchProvers on distinct contexts of one
        GPU overlap each other's latency-bound kernels (transcript, inversions) with MSM work.
        `lagrange_commits`: commit a_1, b_1, c_1, z_1 from Lagrange values over the Lagrange-basis SRS
        (PLONK_PROVER_LAGRANGE_COMMITS) instead of from coefficient forms; same proofs.
        `segments`: None = automatic (`segments_for`); a power of two S forces the per-proof scans of rounds 2, 4 and 5 to run
        cut into S segments per proof (PLONK_PROVER_SEGMENTS_LOG2; 1 = one workgroup per proof): tests and A/B runs, same proofs.
        `solve`: None = automatic (`solve_plan`); "lanes" / "levels" force the witness solver of `upload_inputs*` to run one lane
        per proof / one workgroup per proof over dependency levels (PLONK_PROVER_SOLVE_FORM): tests and A/B runs, same values.
        `blinding`: False = the reference's proofs, which are a deterministic function of the witness.  True or a 32-byte seed =
        zero-knowledge proofs (PLONK_PROVER_BLINDING: the PLONK paper's blinders; needs group_order >= 8 and an SRS of
        group_order + 6 powers); the same verifier accepts them.  True seeds the device's generator from os.urandom once per
        prover; a seed given here must be as secret and as unpredictable: whoever knows it can strip the blinding.
        `set_blinders` gives the next run explicit values instead."""
        self._check_blinding(blinding)
        if solve not in self.SOLVE_FORMS:
            raise ValueError('solve must be None, "lanes" or "levels"')
        self.group_order = program.group_order
        self.setup = setup
        self.program = program
        self.ctx = ctx or get_context()
        self._public_vars = program.get_public_assignments()
        self._wires = [w.as_list() for w in program.wires()]
        n = self.group_order
        # wire cell -> variable index; one extra all-zero slot serves the empty cells and the padding rows
        variables, self._cell_index = program.wiring_table()
        self._vars = list(variables)
        pos = {v: i for i, v in enumerate(self._vars)}
        sel = _selector_bytes(program)
        self._bases = setup.device_bases(self.ctx)
        self._h = ctypes.c_void_p()
        check(self.ctx.L.plonk_prover_create(self.ctx.handle, self._bases.handle, _log2_exact(n), sel,
                                             len(self._public_vars), ctypes.byref(self._h)))
        self._resident = 0
        self._staged_source = None  # the bytes of a staged batch: the library reads them until `advance`
        self._set_options(lagrange_commits, segments, solve, blinding)
        # the wiring goes to the device once; a batch is then only the variables' values (V x 32 B per proof)
        self._getter = None
        if self._vars:
            cells = np.ascontiguousarray(self._cell_index, dtype=np.uint32)
            pubs = np.ascontiguousarray([pos[v] for v in self._public_vars], dtype=np.uint32)
            check(self.ctx.L.plonk_prover_set_wiring(self._h, cells.ctypes.data, pubs.ctypes.data if len(pubs) else None,
                                                     len(self._vars)))
            self._getter = True
            self._var_keys = tuple(self._vars)
        self._pos = pos
        self._input_keys = None  # set_inputs / the first upload_inputs

    def solve_plan(self, B):
        """The witness solver's plan (after `set_inputs`) and the form a batch of B is solved in when `solve` was not given:
        rows walked, active rows, dependency levels, the widest level, the levelised kernel's workgroup size, its steps."""
        out = (ctypes.c_uint32 * 7)()
        check(self.ctx.L.plonk_prover_solve_plan(self._h, B, out))
        rows, active, levels, widest, threads, form, steps = out
        return {"rows": rows, "active_rows": active, "levels": levels, "widest": widest, "threads": threads, "steps": steps,
                "form": {1: "lanes", 2: "levels"}[form]}

    # ---- inputs ---------------------------------------------------------------------------------
    def wire_columns(self, witness):
        """A, B, C value columns of round 1 (prover.py:94-103): witness[None] = 0, zero padded."""
        n = self.group_order
        cols = [[0] * n, [0] * n, [0] * n]
        get = witness.get
        for i, (wl, wr, wo) in enumerate(self._wires):
            cols[0][i] = (get(wl, 0) if wl is not None else 0) % R_MOD
            cols[1][i] = (get(wr, 0) if wr is not None else 0) % R_MOD
            cols[2][i] = (get(wo, 0) if wo is not None else 0) % R_MOD
            if (wl is not None and wl not in witness) or (wr is not None and wr not in witness) or (
                wo is not None and wo not in witness
            ):
                raise KeyError([w for w in (wl, wr, wo) if w is not None and w not in witness][0])
        return cols

    def upload(self, witnesses):
        """Stage a batch of witnesses in HBM: each variable's value is encoded once (V x 32 bytes per proof) and
        the wire columns A, B, C + public inputs are gathered from them on the device (prover.py:94-103, 57-62).
        A KeyError names a missing variable."""
        B = len(witnesses)
        if self._getter is None:
            return self._upload_columns(witnesses)
        enc = _pack_witnesses(witnesses, self._var_keys, R_MOD)
        check(self.ctx.L.plonk_prover_upload_variables(self._h, enc, B))
        self._resident = B

    def upload_values(self, blob, B):
        """The same staging for callers that produce witnesses natively: `blob` = [B][V] canonical 32-byte little-endian
        values in the order of `self.variables` (64 KiB per proof at 2^11; no Python work per value)."""
        if len(blob) != 32 * B * len(self._vars):
            raise ValueError("upload_values: expected %d bytes" % (32 * B * len(self._vars)))
        check(self.ctx.L.plonk_prover_upload_variables(self._h, blob, B))
        self._resident = B

    def upload_values_async(self, pinned, B):
        """upload_values without a host wait: `pinned` = a Context.host_alloc buffer holding [B][V] canonical 32-byte
        values, which must stay untouched until this batch has been downloaded.  The copy runs on the context's copy
        stream and overlaps the kernels of the compute stream; a non-canonical value shows up as status bit 3."""
        if len(pinned) < 32 * B * len(self._vars):
            raise ValueError("upload_values_async: expected %d bytes" % (32 * B * len(self._vars)))
        check(self.ctx.L.plonk_prover_upload_variables_async(self._h, ctypes.addressof(pinned), B))
        self._resident = B

    # ---- inputs only: the device solves for every other variable (csrc/witness_solve.h) -----------------
    def set_inputs(self, names):
        """The circuit's inputs: the variables `upload_inputs` / `upload_input_values` give values for, in that order.
        Names that are not variables of the circuit are dropped (the reference's filler carries them along unused).  The
        device then computes every other variable as `Program.fill_variable_assignments` does.  KeyError(name): a row reads
        that variable before anything gives it a value, or nothing ever does — the filler's KeyError."""
        keys = tuple(k for k in names if k in self._pos)
        idx = np.ascontiguousarray([self._pos[k] for k in keys], dtype=np.uint32)
        missing = ctypes.c_uint32(0xFFFFFFFF)
        rc = self.ctx.L.plonk_prover_set_inputs(self._h, idx.ctypes.data if len(idx) else None, len(idx), ctypes.byref(missing))
        if rc == _lib.PLONK_ERR_ARG and missing.value != 0xFFFFFFFF:
            raise KeyError(self._vars[missing.value])
        check(rc)
        self._input_keys = keys
        self._resident = 0

    @property
    def inputs(self):
        """The input names in the column order `upload_input_values` expects (None before `set_inputs`)."""
        return self._input_keys

    def upload_inputs(self, assignments):
        """Stage a batch from the circuit's inputs alone: one dict of input values per proof (32 bytes per input and proof
        go to the device).  The first call sets the inputs from the first dict's keys that are variables of the circuit;
        a later dict that lacks one of them is a KeyError."""
        if self._input_keys is None:
            self.set_inputs(list(assignments[0]))
        B = len(assignments)
        enc = _pack_witnesses(assignments, self._input_keys, R_MOD)
        check(self.ctx.L.plonk_prover_upload_inputs(self._h, enc, B))
        self._resident = B

    def upload_input_values(self, blob, B):
        """The same staging from packed bytes: `blob` = [B][K] canonical 32-byte little-endian values in the order of
        `self.inputs`."""
        K = len(self._input_keys or ())
        if self._input_keys is not None and len(blob) != 32 * B * K:
            raise ValueError("upload_input_values: expected %d bytes" % (32 * B * K))
        check(self.ctx.L.plonk_prover_upload_inputs(self._h, blob, B))
        self._resident = B

    def upload_input_values_async(self, pinned, B):
        """upload_input_values without a host wait, as `upload_values_async`: `pinned` = a Context.host_alloc buffer that
        stays untouched until this batch has been downloaded; a non-canonical value shows up as status bit 3."""
        K = len(self._input_keys or ())
        if self._input_keys is not None and len(pinned) < 32 * B * K:
            raise ValueError("upload_input_values_async: expected %d bytes" % (32 * B * K))
        check(self.ctx.L.plonk_prover_upload_inputs_async(self._h, ctypes.addressof(pinned), B))
        self._resident = B

    # ---- two-slot intake: the next batch is staged on the copy stream while the resident one proves -----------------
    def stage_inputs(self, assignments):
        """`upload_inputs` into the prover's second intake slot: the batch is copied, solved and gathered on the context's copy
        stream, beside whatever the resident batch is doing, and becomes the resident one at `advance()`.  Nothing of the resident
        batch changes: `run`, `download`, `variable_values`, `public_values` and `solve_failures` keep meaning it."""
        if self._input_keys is None:
            self.set_inputs(list(assignments[0]))
        B = len(assignments)
        enc = _pack_witnesses(assignments, self._input_keys, R_MOD)
        check(self.ctx.L.plonk_prover_stage_inputs(self._h, enc, B))
        self._staged_source = enc

    def stage_input_values_async(self, pinned, B):
        """`stage_inputs` from packed bytes without a host wait: `pinned` = a Context.host_alloc buffer holding [B][K] canonical
        32-byte values in the order of `self.inputs`, untouched until `advance()` has returned.  A non-canonical value shows up as
        status bit 3 of the batch once it is resident."""
        K = len(self._input_keys or ())
        if self._input_keys is not None and len(pinned) < 32 * B * K:
            raise ValueError("stage_input_values_async: expected %d bytes" % (32 * B * K))
        check(self.ctx.L.plonk_prover_stage_inputs(self._h, ctypes.addressof(pinned), B))
        self._staged_source = pinned

    def stage_values_async(self, pinned, B):
        """The same for packed variables, as `upload_values_async`: `pinned` holds [B][V] canonical 32-byte values in the order of
        `self.variables`."""
        if len(pinned) < 32 * B * len(self._vars):
            raise ValueError("stage_values_async: expected %d bytes" % (32 * B * len(self._vars)))
        check(self.ctx.L.plonk_prover_stage_variables(self._h, ctypes.addressof(pinned), B))
        self._staged_source = pinned

    @property
    def staged(self):
        """The size of the batch that is staged, 0 if none is."""
        out = ctypes.c_size_t(0)
        check(self.ctx.L.plonk_prover_staged(self._h, ctypes.byref(out)))
        return out.value

    def advance(self):
        """The staged batch becomes the resident one (the compute stream waits for its staging; no host wait); returns its size.
        The batch that was resident is given up, downloaded or not."""
        out = ctypes.c_size_t(0)
        check(self.ctx.L.plonk_prover_advance(self._h, ctypes.byref(out)))
        self._resident = out.value
        self._staged_source = None
        return out.value

    def variable_values(self, names=None, B=None):
        """The resident batch's variable values, one dict name -> int per proof (all variables, or `names`): what the
        solver computed, after `upload_inputs*`; what was uploaded, after `upload` / `upload_values*`."""
        B = self._resident if B is None else B
        names = self._vars if names is None else list(names)
        idx = None if names is self._vars else np.ascontiguousarray([self._pos[k] for k in names], dtype=np.uint32)
        k = len(names)
        out = ctypes.create_string_buffer(32 * B * max(k, 1))
        check(self.ctx.L.plonk_prover_download_variables(self._h, B, None if idx is None else idx.ctypes.data, k, out))
        raw = out.raw
        return [{name: int.from_bytes(raw[32 * (b * k + j) : 32 * (b * k + j + 1)], "little") for j, name in enumerate(names)}
                for b in range(B)]

    def public_values(self, B=None):
        """The resident batch's public inputs in the order of the public rows, one list of ints per proof: what
        `VerificationKey.verify_proof` takes — a public variable the solver computed (a hash, say) among them."""
        if not self._public_vars:
            return [[] for _ in range(self._resident if B is None else B)]
        return [[w[v] for v in self._public_vars] for w in self.variable_values(self._public_vars, B)]

    def solve_failures(self, B=None):
        """Per proof of the resident batch: None, or the row whose check failed first in the solver (status bit 16)."""
        B = self._resident if B is None else B
        rows = (ctypes.c_uint32 * B)()
        check(self.ctx.L.plonk_prover_solve_failures(self._h, B, rows))
        return [r - 1 if r else None for r in rows]

    @property
    def variables(self):
        """Variable names in the column order `upload_values` expects."""
        return tuple(self._vars)

    def _upload_columns(self, witnesses):
        """The [3][B][n] column form of the same upload (circuits without variables; plonk_prover_upload_witness)."""
        B = len(witnesses)
        n, V = self.group_order, len(self._vars)
        abc = np.empty((3, B, n, 4), dtype=np.uint64)  # 32-byte little-endian elements as 4 x u64
        flat_index = self._cell_index.ravel()
        zero = bytes(32)
        for b, w in enumerate(witnesses):
            enc = b"".join([(w[v] % R_MOD).to_bytes(32, "little") for v in self._vars]) + zero
            table = np.frombuffer(enc, dtype=np.uint64).reshape(V + 1, 4)
            abc[:, b] = np.take(table, flat_index, axis=0).reshape(3, n, 4)
        abc = abc.tobytes()
        pub = b"".join(_le([w[v] % R_MOD for v in self._public_vars]) for w in witnesses)
        check(self.ctx.L.plonk_prover_upload_witness(self._h, abc, pub if self._public_vars else None, B))
        self._resident = B

    def upload_raw(self, abc_bytes, pub_bytes, B):
        check(self.ctx.L.plonk_prover_upload_witness(self._h, abc_bytes, pub_bytes, B))
        self._resident = B

    def prove_batch(self, witnesses):
        self.upload(witnesses)
        self.run()
        return self.download()

    def prove_inputs(self, assignments):
        """prove_batch from the circuit's inputs alone (`upload_inputs`)."""
        self.upload_inputs(assignments)
        self.run()
        return self.download()

    def prove_inputs_stream(self, batches):
        """`prove_inputs` over an iterable of batches, as a generator of each batch's proofs in order: batch k + 1 is packed and
        staged (`stage_inputs`) right after batch k's rounds were enqueued, so that its copy and its solve run beside them, and
        batch k is downloaded after that."""
        batches = iter(batches)
        batch = next(batches, None)
        if batch is None:
            return
        self.upload_inputs(batch)
        while batch is not None:
            self.run()
            batch = next(batches, None)
            if batch is not None:
                self.stage_inputs(batch)
            yield self.download()
            if batch is not None:
                self.advance()

    def prove(self, witness) -> Proof:  # prover.py:51-84
        return self.prove_batch([witness])[0]


class MultiBatchProver(_LockStepProver):
    """Proofs of several circuits in one lock-step batch: a table of circuits of ONE setup and ONE group order (a circuit that
    needs fewer rows is compiled at the common order: `Program(lines, n)` pads), each proof of a batch labelled with its circuit's
    position in `programs`.  The proofs are byte for byte those of a `BatchProver` of the proof's circuit.  What it does not do
    yet: the witness solver (`set_inputs`, `upload_input_values`, `solve_plan`) and the two-slot intake (`stage_values_async`,
    `advance`) raise the library's refusal, and circuits of different group orders do not share a table."""

    MAX_CIRCUITS = 64  # PLONK_PROVER_MAX_CIRCUITS

    def __init__(self, setup: Setup, programs, ctx=None, lagrange_commits=False, segments=None, blinding=False):
        """`programs`: the table; the other arguments as `BatchProver`'s."""
        self._check_blinding(blinding)
        programs = list(programs)
        K = len(programs)
        if not 1 <= K <= self.MAX_CIRCUITS:
            raise ValueError("%d circuits: a table holds 1 to %d" % (K, self.MAX_CIRCUITS))
        n = programs[0].group_order
        if any(p.group_order != n for p in programs):
            raise ValueError("the circuits of a table are of one group order: got %s" % sorted({p.group_order for p in programs}))
        self.group_order, self.setup, self.programs = n, setup, programs
        self.ctx = ctx or get_context()
        tables = [p.wiring_table() for p in programs]
        self._vars = [tuple(v) for v, _ in tables]
        self._public_vars = [list(p.get_public_assignments()) for p in programs]
        V = self._n_vars = max(1, max(len(v) for v in self._vars))  # one row width serves the table; V also marks "no variable"
        l_max = self._l_max = max(len(v) for v in self._public_vars)
        self._bases = setup.device_bases(self.ctx)
        self._h = ctypes.c_void_p()
        self._resident, self._ids = 0, []
        check(self.ctx.L.plonk_prover_create_multi(self.ctx.handle, self._bases.handle, _log2_exact(n), K, b"".join(_selector_bytes(p) for p in programs),
                                                   (ctypes.c_size_t * K)(*[len(v) for v in self._public_vars]), ctypes.byref(self._h)))
        self._set_options(lagrange_commits, segments, None, blinding)
        cells = np.empty((K, 3, n), dtype=np.uint32)
        pubs = np.full((K, max(l_max, 1)), V, dtype=np.uint32)
        for c, (variables, cell_index) in enumerate(tables):
            cells[c] = np.where(cell_index == len(variables), V, cell_index)  # the circuit's own "empty" marker -> the table's
            pos = {v: i for i, v in enumerate(variables)}
            pubs[c, : len(self._public_vars[c])] = [pos[v] for v in self._public_vars[c]]
        pubs = np.ascontiguousarray(pubs[:, :l_max])
        check(self.ctx.L.plonk_prover_set_wiring_multi(self._h, cells.ctypes.data, pubs.ctypes.data if l_max else None, V))

    # ---- inputs ---------------------------------------------------------------------------------
    def _label(self, circuit_ids):
        """The labels of the next upload -> its batch size.  A table of one circuit may give the batch size alone (no labels)."""
        if isinstance(circuit_ids, int):
            return [0] * circuit_ids
        ids = [int(c) for c in circuit_ids]
        check(self.ctx.L.plonk_prover_set_labels(self._h, (ctypes.c_uint32 * len(ids))(*ids), len(ids)))
        return ids

    def variables(self, cid):
        """Circuit `cid`'s variable names in the order its proofs' value rows hold them (the first of `n_vars` columns)."""
        return self._vars[cid]

    @property
    def n_vars(self):
        """Values per proof of `upload_values`: the most variables of any circuit of the table."""
        return self._n_vars

    @property
    def circuit_ids(self):
        """The labels of the resident batch."""
        return list(self._ids)

    def upload(self, witnesses, circuit_ids=None):
        """One witness dict per proof and the circuit of each (`circuit_ids` may be left out for a table of one circuit): each
        variable's value once, [n_vars] per proof; wire columns and public rows are gathered on the device."""
        ids = self._label(len(witnesses) if circuit_ids is None else circuit_ids)
        if len(ids) != len(witnesses):
            raise ValueError("%d witnesses, %d circuit ids" % (len(witnesses), len(ids)))
        V = self._n_vars
        enc = b"".join(_pack_witnesses([w], self._vars[c], R_MOD) + bytes(32 * (V - len(self._vars[c]))) for w, c in zip(witnesses, ids))
        check(self.ctx.L.plonk_prover_upload_variables(self._h, enc, len(ids)))
        self._resident, self._ids = len(ids), ids

    def upload_values(self, blob, circuit_ids):
        """`blob` = [B][n_vars] canonical 32-byte little-endian values, row b in the order of `variables(circuit_ids[b])`, the rest
        of the row ignored."""
        ids = self._label(circuit_ids)
        if len(blob) != 32 * len(ids) * self._n_vars:
            raise ValueError("upload_values: expected %d bytes" % (32 * len(ids) * self._n_vars))
        check(self.ctx.L.plonk_prover_upload_variables(self._h, blob, len(ids)))
        self._resident, self._ids = len(ids), ids

    def upload_values_async(self, pinned, circuit_ids):
        """upload_values without a host wait, as `BatchProver.upload_values_async`."""
        ids = self._label(circuit_ids)
        if len(pinned) < 32 * len(ids) * self._n_vars:
            raise ValueError("upload_values_async: expected %d bytes" % (32 * len(ids) * self._n_vars))
        check(self.ctx.L.plonk_prover_upload_variables_async(self._h, ctypes.addressof(pinned), len(ids)))
        self._resident, self._ids = len(ids), ids

    def upload_raw(self, abc_bytes, pub_bytes, circuit_ids):
        """Wire columns [3][B][n] and public rows [B][l_max] (l_max = the most public inputs of any circuit of the table), a row
        zero beyond its own circuit's count."""
        ids = self._label(circuit_ids)
        check(self.ctx.L.plonk_prover_upload_witness(self._h, abc_bytes, pub_bytes, len(ids)))
        self._resident, self._ids = len(ids), ids

    def public_values(self):
        """The resident batch's public inputs after a variables upload: ragged rows, each of its proof's circuit's length."""
        B, V = self._resident, self._n_vars
        out = ctypes.create_string_buffer(32 * B * V)
        check(self.ctx.L.plonk_prover_download_variables(self._h, B, None, V, out))
        rows = []
        for b, c in enumerate(self._ids):
            pos = {v: i for i, v in enumerate(self._vars[c])}
            rows.append([int.from_bytes(out.raw[32 * (b * V + pos[v]) : 32 * (b * V + pos[v] + 1)], "little") for v in self._public_vars[c]])
        return rows

    def prove_batch(self, witnesses, circuit_ids=None):
        self.upload(witnesses, circuit_ids)
        self.run()
        return self.download()

    # ---- not on a table of circuits yet: these raise what the library returns ---------------------------------
    def set_inputs(self, index):
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        check(self.ctx.L.plonk_prover_set_inputs(self._h, idx.ctypes.data, len(idx), ctypes.byref(ctypes.c_uint32(0))))

    def upload_input_values(self, blob, B):
        check(self.ctx.L.plonk_prover_upload_inputs(self._h, blob, B))

    def solve_plan(self, B):
        check(self.ctx.L.plonk_prover_solve_plan(self._h, B, (ctypes.c_uint32 * 7)()))

    def solve_failures(self, B=None):
        return [None] * (self._resident if B is None else B)

    def stage_values_async(self, pinned, B):
        check(self.ctx.L.plonk_prover_stage_variables(self._h, ctypes.addressof(pinned), B))

    def advance(self):
        check(self.ctx.L.plonk_prover_advance(self._h, ctypes.byref(ctypes.c_size_t(0))))
