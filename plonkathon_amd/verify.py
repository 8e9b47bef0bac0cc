"""`BatchVerifier` — N proofs of one circuit checked with one pairing product; `MultiBatchVerifier` — the same for a batch mixed
of the circuits of a table (one setup).

The reference verifies one proof per call (TESTING_verifier_DO_NOT_OPEN.py:39-163): e(L, [x]_2) == e(R, [1]_2) with L, R in G1.
For a batch the device computes every proof's L_i and R_i (transcript replay, field arithmetic and eleven scalar
multiplications per proof: plonk_verifier_* in include/plonk_hip.h), folds them under random 128-bit weights rho_i, and the host
asks `pairing_check` once: e(sum rho_i L_i, [x]_2) == e(sum rho_i R_i, [1]_2).  Honest batches always pass; a batch holding a bad
proof passes with probability about 2^-128.  The check is over the same [x]_2 whatever circuit a proof belongs to, so proofs of
several circuits of one setup fold together: only the eight key points a proof's fixed scalars multiply are its circuit's
(plonk_verifier_create_multi, _load_multi, _load_provers).

Naming the bad proofs of a batch that failed (`verify_each`) is by bisection over folds by default: a fold launch and a host pairing
per probe, so the cost grows with the number of bad proofs.  `device=True` replaces the bisection by ONE launch that runs every
proof's own pairing check on the device, one lane per proof (plonk_verifier_check_each, csrc/pairing_device.h): the same cost
whatever the number of bad proofs.
"""
import ctypes
import os

from ._lib import check
from .backend import get_context
from .field import Fq
from .kzg import G2, _g1_neg, pairing_check
from .plonk import Proof
from .polynomial import _log2_exact

STATUS_MALFORMED, STATUS_OFF_CURVE, STATUS_IDENTITY = 1, 2, 4
_NOT_BELOW_P = b"\xff" * 32  # stands in for a coordinate the compressed encoding could not give: status bit 0 on the device


def _point_bytes(pt):
    return bytes(64) if pt is None else int(pt[0]).to_bytes(32, "little") + int(pt[1]).to_bytes(32, "little")


def _key_bytes(vk):
    return b"".join(_point_bytes(p) for p in (vk.Qm, vk.Ql, vk.Qr, vk.Qo, vk.Qc, vk.S1, vk.S2, vk.S3))


def _public_row(row, n_public):
    row = [int(x) for x in row]
    assert len(row) == n_public, "a row of %d public inputs, the circuit has %d" % (len(row), n_public)
    assert all(0 <= x < (1 << 256) for x in row), "a public input is not a canonical Fr value"
    return b"".join(x.to_bytes(32, "little") for x in row)


class _Verifier:
    """What the two verifiers share: a plonk_verifier handle, the forms proofs come in, folds, the pairing check and bisection."""

    def __init__(self, vk, ctx):
        self.vk = vk  # its X_2 is the one the pairing check is over
        self.ctx = ctx or get_context()
        self.status, self.pairing_checks, self.device_checks = b"", 0, 0
        self._batch = 0
        self._x2_set = False  # the line tables of vk.X_2 and G2 are built at the first device check
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.L.plonk_verifier_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- inputs ---------------------------------------------------------------------------------
    def _records(self, proofs, B):
        """768-byte records (plonk_prover_download's layout) from 768-byte records, 480-byte compressed records or Proof objects."""
        if isinstance(proofs, (bytes, bytearray, memoryview)):
            proofs = bytes(proofs)
            if len(proofs) == 768 * B:
                return proofs
            assert len(proofs) == 480 * B, "proofs: %d bytes are neither %d records of 768 nor of 480 bytes" % (len(proofs), B)
            return self._decompress(proofs, B)
        proofs = list(proofs)
        assert len(proofs) == B, "%d proofs, %d rows of public inputs" % (len(proofs), B)
        out = []
        for p in proofs:
            f = p.flatten()
            out.append(b"".join(_point_bytes(f[k]) for k in Proof._POINTS) + b"".join(int(f[k]).to_bytes(32, "little") for k in Proof._SCALARS))
        return b"".join(out)

    def _decompress(self, blob, B):
        pts = b"".join(blob[480 * i : 480 * i + 288] for i in range(B))
        xy = ctypes.create_string_buffer(64 * 9 * B)
        st = ctypes.create_string_buffer(9 * B)
        check(self.ctx.L.plonk_g1_decompress(self.ctx.handle, pts, 9 * B, xy, st))
        xy, st = xy.raw, st.raw
        out = []
        for i in range(B):
            for k in range(9):
                j = 9 * i + k
                if st[j] == 1:  # malformed encoding: status bit 0
                    out.append(_NOT_BELOW_P + _NOT_BELOW_P)
                elif st[j] == 2:  # x^3 + 3 is not a square, 1 is: (x, 1) is off the curve, status bit 1
                    x = int.from_bytes(pts[32 * j : 32 * j + 32], "big") & ((1 << 254) - 1)
                    out.append(x.to_bytes(32, "little") + (1).to_bytes(32, "little"))
                else:
                    out.append(xy[64 * j : 64 * j + 64])
            out.append(b"".join(blob[480 * i + 288 + 32 * e : 480 * i + 320 + 32 * e][::-1] for e in range(6)))  # big-endian there
        return b"".join(out)

    @staticmethod
    def _seed(seed):
        seed = os.urandom(32) if seed is None else bytes(seed)
        assert len(seed) == 32, "seed: 32 bytes"
        return seed

    def _loaded(self, B):
        st = ctypes.create_string_buffer(B)
        check(self.ctx.L.plonk_verifier_status(self._h, st))
        self.status, self._batch, self.pairing_checks, self.device_checks = st.raw[:B], B, 0, 0

    # ---- folds and verdicts ---------------------------------------------------------------------
    def fold(self, lo, hi):
        """(sum rho_i L_i, sum rho_i R_i) over the well-formed proofs lo <= i < hi of the loaded batch; None = identity."""
        L, R, fl = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64), ctypes.create_string_buffer(2)
        check(self.ctx.L.plonk_verifier_fold(self._h, lo, hi, L, R, fl))

        def pt(buf, flag):
            return None if flag else (Fq(int.from_bytes(buf.raw[:32], "little")), Fq(int.from_bytes(buf.raw[32:64], "little")))

        return pt(L, fl.raw[0]), pt(R, fl.raw[1])

    def check_pairing(self, L, R) -> bool:
        """e(L, [x]_2) == e(R, [1]_2) for the two points of a fold: the one pairing product of a batch (host CPU)."""
        self.pairing_checks += 1
        return pairing_check([(L, self.vk.X_2), (_g1_neg(R), G2)])

    def _check(self, lo, hi):
        return self.check_pairing(*self.fold(lo, hi))

    def _verdict(self):
        return all(s == 0 for s in self.status) and self._check(0, self._batch)

    def check_each_device(self):
        """Every proof of the loaded batch under its OWN pairing check, on the device in one launch: [bool] per proof (False
        without a pairing where the status byte is set).  `device_checks` counts the lanes."""
        if not self._x2_set:
            x, y = self.vk.X_2
            check(self.ctx.L.plonk_verifier_set_x2(self._h, b"".join(int(c).to_bytes(32, "little") for c in x.coeffs + y.coeffs)))
            self._x2_set = True
        ok = ctypes.create_string_buffer(self._batch)
        check(self.ctx.L.plonk_verifier_check_each(self._h, ok))
        self.device_checks += self._batch
        return [b != 0 for b in ok.raw[: self._batch]]

    def _verdicts(self, device=False):
        B = self._batch
        res = [s == 0 for s in self.status]
        if self._check(0, B):
            return res
        if device:
            return self.check_each_device()

        def split(lo, hi):  # the fold over [lo, hi) is known to fail
            if hi - lo == 1:
                res[lo] = False
                return
            mid = (lo + hi) // 2
            if self._check(lo, mid):
                split(mid, hi)  # the failure is on the right: no check needed to know it
                return
            split(lo, mid)
            if not self._check(mid, hi):
                split(mid, hi)

        split(0, B)
        return res


class BatchVerifier(_Verifier):
    def __init__(self, vk, n_public: int, ctx=None):
        """`vk`: the VerificationKey of `Setup.verification_key(...)`; `n_public`: public inputs per proof."""
        super().__init__(vk, ctx)
        self.n_public = int(n_public)
        check(self.ctx.L.plonk_verifier_create(self.ctx.handle, _log2_exact(vk.group_order), _key_bytes(vk), self.n_public, ctypes.byref(self._h)))

    def _publics(self, publics):
        return b"".join(_public_row(row, self.n_public) for row in publics)

    def load(self, proofs, publics, seed=None):
        """Per-proof work on the device: status bytes, weighted scalars, scalar multiplications, L_i and R_i."""
        publics = list(publics)
        B = len(publics)
        pub = self._publics(publics)
        rec = self._records(proofs, B)
        self._batch = 0
        check(self.ctx.L.plonk_verifier_load(self._h, rec, pub if self.n_public else None, B, self._seed(seed)))
        self._loaded(B)

    def load_prover(self, batch_prover, B=None, seed=None):
        """The same for the batch resident in a BatchProver (after run()): the proofs never leave the device."""
        B = batch_prover._resident if B is None else B
        self._batch = 0
        check(self.ctx.L.plonk_verifier_load_prover(self._h, batch_prover._h, B, self._seed(seed)))
        self._loaded(B)

    def verify(self, proofs, publics, seed=None) -> bool:
        """True iff every proof is well-formed and the fold over the whole batch passes the pairing check.  `proofs`: bytes of
        768-byte records, bytes of 480-byte compressed records (BatchProver.download_compressed) or a list of Proof objects;
        `publics`: one row of public inputs per proof (at least one proof: an empty batch is the library's "bad argument").
        `seed`: 32 bytes the weights are derived from; a seed the prover can
        predict voids the soundness argument, so leave it None (os.urandom) outside tests and reproducible runs."""
        self.load(proofs, publics, seed)
        return self._verdict()

    def verify_each(self, proofs, publics, seed=None, device=False):
        """One verdict per proof.  The whole batch first; only if that fails, bisection by folds over sub-ranges (same weights,
        nothing recomputed on the device but range sums): at most 2 k ceil(log2 B) + 1 pairing checks for k bad proofs.
        `device=True`: in place of the bisection, every proof's own pairing check on the device in one launch (`pairing_checks`
        stays 1, `device_checks` = the batch size)."""
        self.load(proofs, publics, seed)
        return self._verdicts(device)

    def verify_prover(self, batch_prover, B=None, seed=None) -> bool:
        """verify() for the batch resident in `batch_prover` (after run()), without a trip through the host."""
        self.load_prover(batch_prover, B, seed)
        return self._verdict()

    def verify_each_prover(self, batch_prover, B=None, seed=None, device=False):
        self.load_prover(batch_prover, B, seed)
        return self._verdicts(device)


class MultiBatchVerifier(_Verifier):
    """A batch mixed of the circuits of a table, one pairing check.  The circuits must be of ONE setup: the argument folds checks
    over the same [x]_2, so keys of different setups are refused, not verified separately."""

    MAX_CIRCUITS = 64  # PLONK_VERIFIER_MAX_CIRCUITS

    def __init__(self, circuits, ctx=None):
        """`circuits`: a list of (vk, n_public); a proof's circuit id is its circuit's position in that list."""
        circuits = [(vk, int(l)) for vk, l in circuits]
        K = len(circuits)
        assert 1 <= K <= self.MAX_CIRCUITS, "%d circuits: a table holds 1 to %d" % (K, self.MAX_CIRCUITS)
        assert all(vk.X_2 == circuits[0][0].X_2 for vk, _ in circuits), "the verification keys are of different setups ([x]_2 differs)"
        super().__init__(circuits[0][0], ctx)
        self.vks, self.n_public = [vk for vk, _ in circuits], [l for _, l in circuits]
        log_n = (ctypes.c_uint * K)(*[_log2_exact(vk.group_order) for vk in self.vks])
        n_public = (ctypes.c_size_t * K)(*self.n_public)
        check(self.ctx.L.plonk_verifier_create_multi(self.ctx.handle, K, log_n, b"".join(_key_bytes(vk) for vk in self.vks), n_public, ctypes.byref(self._h)))

    def _ids(self, circuit_ids):
        ids = [int(c) for c in circuit_ids]
        assert all(0 <= c < len(self.vks) for c in ids), "a circuit id is outside the table of %d circuits" % len(self.vks)
        return ids

    def load(self, proofs, circuit_ids, publics, seed=None):
        """As BatchVerifier.load; `circuit_ids[i]` is the circuit of proof i and `publics[i]` a row of that circuit's length."""
        ids, publics = self._ids(circuit_ids), list(publics)
        B = len(ids)
        assert len(publics) == B, "%d circuit ids, %d rows of public inputs" % (B, len(publics))
        pub = b"".join(_public_row(row, self.n_public[c]) for row, c in zip(publics, ids))
        rec = self._records(proofs, B)
        self._batch = 0
        check(self.ctx.L.plonk_verifier_load_multi(self._h, rec, (ctypes.c_uint32 * B)(*ids), pub or None, len(pub) // 32, B, self._seed(seed)))
        self._loaded(B)

    def load_provers(self, provers, seed=None):
        """`provers`: [(circuit_id, BatchProver), ...], each after run().  The batch is their resident batches one after the other
        in list order; the proofs never leave the device."""
        provers = list(provers)
        ids = self._ids(c for c, _ in provers)
        n = len(provers)
        B = sum(bp._resident for _, bp in provers)
        self._batch = 0
        handles = (ctypes.c_void_p * n)(*[bp._h.value for _, bp in provers])
        check(self.ctx.L.plonk_verifier_load_provers(self._h, n, handles, (ctypes.c_uint32 * n)(*ids), self._seed(seed)))
        self._loaded(B)

    def load_prover(self, multi_prover, circuit_map=None, seed=None):
        """The batch resident in a MultiBatchProver (after run()), mixed as it is, without a trip through the host.
        `circuit_map[c]`: this table's id of the prover's circuit c; None = the two tables are in the same order."""
        K = len(multi_prover.programs)
        ids = self._ids(range(K) if circuit_map is None else circuit_map)
        assert len(ids) == K, "circuit_map: %d entries, the prover's table holds %d circuits" % (len(ids), K)
        self._batch = 0
        check(self.ctx.L.plonk_verifier_load_multi_prover(self._h, multi_prover._h, (ctypes.c_uint32 * K)(*ids), self._seed(seed)))
        self._loaded(multi_prover._resident)

    def verify_prover(self, multi_prover, circuit_map=None, seed=None) -> bool:
        self.load_prover(multi_prover, circuit_map, seed)
        return self._verdict()

    def verify_each_prover(self, multi_prover, circuit_map=None, seed=None, device=False):
        self.load_prover(multi_prover, circuit_map, seed)
        return self._verdicts(device)

    def verify(self, proofs, circuit_ids, publics, seed=None) -> bool:
        """BatchVerifier.verify for a mixed batch: one pairing check for all of it."""
        self.load(proofs, circuit_ids, publics, seed)
        return self._verdict()

    def verify_each(self, proofs, circuit_ids, publics, seed=None, device=False):
        """One verdict per position, by bisection over positions: the sub-ranges cut across circuits.  `device=True`: as
        BatchVerifier.verify_each, each proof against the key points of its own circuit."""
        self.load(proofs, circuit_ids, publics, seed)
        return self._verdicts(device)

    def verify_provers(self, provers, seed=None) -> bool:
        self.load_provers(provers, seed)
        return self._verdict()

    def verify_each_provers(self, provers, seed=None, device=False):
        self.load_provers(provers, seed)
        return self._verdicts(device)
