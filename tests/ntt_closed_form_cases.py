"""Transforms whose spectrum has a closed form: the bodies of tests/test_gpu_ntt_closed_form.py (2^25 .. 2^28 on an MI355X) and
tests/test_emu_ntt_closed_form.py (the same bodies at 2^9 .. 2^14 on the emulated kernels, and the checks of the references).

Above 2^24 the C oracle needs a minute per transform, so these inputs are built on the device and their transform is known
without computing one.  w = root_of_unity(n), m = the field modulus, X[k] = sum_j x[j] w^(jk); the inverse uses w^-1 and 1/n.

  1. geometric    x[j] = a c^j, c^n != 1          X[k] = a (c^n - 1) / (c w^k - 1)          inverse: / n, with w^-k
  2. deltas       x = 0 but v_t at j_t             X[k] = sum_t v_t w^(j_t k)                inverse: / n, with w^-k
  3. periodic     x[j] = b[j mod p]                X[k] = (n/p) B[k / (n/p)] where n/p | k, else 0 (B: the C oracle's p-point
                                                   transform of b);   inverse: Binv[k / (n/p)], Binv the oracle's inverse
  4. sparse poly  p(X) = sum_t a_t X^(e_t)         Lagrange values v_i = sum_t a_t (w^(e_t))^i;  on the coset: p(off mu^k), k < 4n,
                                                   mu = root_of_unity(4n);  back: a_t at e_t and zero everywhere else

Every closed form is evaluated in Python integers on the sample set S(n) (`sample_set`: both sides of every power of two, the
ends, 32 seeded indices).  For BN254 the expected vector E is also built on the device from the streaming kernels of fr_ops.hip
(powers, scalar ops, batch inversion, pointwise sums — grid-stride loops over size_t indices that test_fr_ops_launch_geometries pins
through their second grid pass), and the assertion of record has three steps, in this order (`check_output`):
  1. E equals the Python closed form on all of S(n) — this pins the reference vector itself;
  2. the transform's output equals E everywhere (plonk_fr_equal); on a mismatch the output is read on S(n), so the failure names indices;
  3. the round trip equals the input (plonk_fr_equal).
BLS12-381 has no device-side operators: it is checked on S(n) (and on every non-zero position of its sparse vectors) only.

All comparisons are exact integer equality.  Nothing is uploaded for BN254 but the delta values, the p values of b and — to place
the p non-zero bins of family 3's expected vector, which come from the C oracle — p more; a failed allocation fails the test
with the size in the message.
"""
import ctypes
import random

from oracle import c_oracle
from oracle import field as ofield

BN254_M = ofield.R_MOD
BLS_M = c_oracle.BLS12_381_FR_MODULUS


def bn254_root(n):
    return ofield.root_of_unity(n)


def bls_root(n):
    return pow(7, (BLS_M - 1) // n, BLS_M)


def sample_set(n, seed=0):
    """S(n): 0 .. 3, n - 2, n - 1; 2^b - 1, 2^b, 2^b + 1 for every bit 1 <= b < log2 n; 32 seeded random indices."""
    s = {0, 1, 2, 3, n - 2, n - 1}
    b = 1
    while (1 << b) < n:
        s |= {(1 << b) - 1, 1 << b, (1 << b) + 1}
        b += 1
    rng = random.Random(1000003 * seed + n)
    s |= {rng.randrange(n) for _ in range(32)}
    return sorted(k for k in s if 0 <= k < n)


# ---- the families: closed forms in Python integers (field given by modulus m and root w of order n) -------------------------
class Geometric:
    name = "geometric"

    def __init__(self, n, seed, m=BN254_M, root=bn254_root):
        rng = random.Random(seed)
        self.n, self.m, self.w = n, m, root(n)
        while True:
            self.a, self.c = rng.randrange(2, m), rng.randrange(2, m)
            if pow(self.c, n, m) != 1:
                break

    def host_input(self):
        return [self.a * pow(self.c, j, self.m) % self.m for j in range(self.n)]

    def numerator(self, inverse):
        num = self.a * (pow(self.c, self.n, self.m) - 1) % self.m
        return num * pow(self.n, -1, self.m) % self.m if inverse else num

    def closed(self, inverse):
        m, c = self.m, self.c
        wk, num = (pow(self.w, -1, m) if inverse else self.w), self.numerator(inverse)
        return lambda k: num * pow((c * pow(wk, k, m) - 1) % m, -1, m) % m


class Deltas:
    name = "deltas"

    def __init__(self, n, seed, m=BN254_M, root=bn254_root):
        rng = random.Random(seed)
        self.n, self.m, self.w = n, m, root(n)
        pos = []
        for j in (0, 1, n // 2 - 1, n // 2, n - 1, (3 * 2 ** 13 + 5) % n):
            if j not in pos:
                pos.append(j)
        while len(pos) < 9:
            j = rng.randrange(n)
            if j not in pos:
                pos.append(j)
        vals = [rng.randrange(1, m) for _ in pos]
        vals[3] = m - 1  # at n / 2
        self.terms = list(zip(pos, vals))

    def host_input(self):
        x = [0] * self.n
        for j, v in self.terms:
            x[j] = v
        return x

    def sequences(self, inverse):
        """the spectrum as a sum of geometric sequences: [(first, base)], value k = sum first * base^k"""
        m = self.m
        wk = pow(self.w, -1, m) if inverse else self.w
        scale = pow(self.n, -1, m) if inverse else 1
        return [(v * scale % m, pow(wk, j, m)) for j, v in self.terms]

    def closed(self, inverse):
        seq, m = self.sequences(inverse), self.m
        return lambda k: sum(f * pow(b, k, m) for f, b in seq) % m


class Periodic:
    name = "periodic"

    def __init__(self, n, seed, m=BN254_M, root=bn254_root):
        assert m == BN254_M
        rng = random.Random(seed)
        self.n, self.m, self.w = n, m, root(n)
        self.p = min(1 << 10, n // 4)
        self.b = [rng.randrange(m) for _ in range(self.p)]
        self._bins = {}

    def host_input(self):
        return [self.b[j % self.p] for j in range(self.n)]

    def bins(self, inverse):
        """the p bins that are not zero, bin i at index i n / p"""
        if inverse not in self._bins:
            B = c_oracle.fr_ntt(self.b, inverse)
            self._bins[inverse] = B if inverse else [(self.n // self.p) * v % self.m for v in B]
        return self._bins[inverse]

    def closed(self, inverse):
        q, bins = self.n // self.p, self.bins(inverse)
        return lambda k: bins[k // q] if k % q == 0 else 0


class SparsePoly:
    """family 4: p(X) = sum_t a_t X^(e_t), e = 0, 3, n - 1 and two seeded exponents"""

    def __init__(self, n, seed, m=BN254_M, root=bn254_root):
        rng = random.Random(seed)
        self.n, self.m, self.w, self.mu = n, m, root(n), root(4 * n)
        exps = [0, 3, n - 1]
        while len(exps) < 5:
            e = rng.randrange(n)
            if e not in exps:
                exps.append(e)
        self.terms = [(e, rng.randrange(1, m)) for e in exps]
        self.off = rng.randrange(2, m)

    def coeffs(self, length=None):
        c = [0] * (length or self.n)
        for e, a in self.terms:
            c[e] = a
        return c

    def lagrange(self):
        m, w, terms = self.m, self.w, self.terms
        return lambda i: sum(a * pow(w, e * i, m) for e, a in terms) % m

    def coset_sequences(self):
        m = self.m
        return [(a * pow(self.off, e, m) % m, pow(self.mu, e, m)) for e, a in self.terms]

    def on_coset(self):
        seq, m = self.coset_sequences(), self.m
        return lambda k: sum(f * pow(b, k, m) for f, b in seq) % m

    def gaps(self, length):
        """[start, stop) runs of the coefficient vector of `length` entries that must be zero"""
        out, at = [], 0
        for e in sorted(e for e, _ in self.terms):
            if e > at:
                out.append((at, e))
            at = e + 1
        if at < length:
            out.append((at, length))
        return out


FAMILIES = {"geometric": Geometric, "deltas": Deltas, "periodic": Periodic}


# ---- the comparison ------------------------------------------------------------------------------------------------------
def check_samples(what, S, closed, out_at):
    """out_at(k) == closed(k) for every k of S; the failure lists (index, got, want)."""
    bad = [(k, out_at(k), closed(k)) for k in S if out_at(k) != closed(k)]
    assert not bad, "%s: %d of %d sampled indices differ from the closed form, (index, got, want): %s" % (what, len(bad), len(S), bad[:6])


def check_output(what, S, closed, e_at, out_at, whole_equal):
    """The assertion of record, steps 1 and 2: the expected vector E (read with e_at) equals the Python closed form on S; the
    output equals E everywhere (whole_equal() — plonk_fr_equal on the device, a list compare in the checker's own tests).  On a
    mismatch the output is read on S, so that the failure names indices."""
    check_samples(what + ": the expected vector itself", S, closed, e_at)
    if not whole_equal():
        check_samples(what, S, closed, out_at)
        raise AssertionError("%s: the output differs from the expected vector at indices outside the sample set" % what)


# ---- device side (BN254): the C-ABI on an explicit context -----------------------------------------------------------------
def _le32(x):
    return int(x).to_bytes(32, "little")


class Dev:
    """The few C-ABI calls the cases need, on one context; records the least free device memory seen at its checkpoints."""

    def __init__(self, ctx):
        from plonkathon_amd._lib import OP_ADD, OP_MUL, OP_SUB, check

        self.ctx, self.L, self.H, self.check = ctx, ctx.L, ctx.handle, check
        self.OP_ADD, self.OP_SUB, self.OP_MUL = OP_ADD, OP_SUB, OP_MUL
        self.free0 = ctx.mem_info()[0]
        self.least_free = self.free0

    def mark(self):
        self.least_free = min(self.least_free, self.ctx.mem_info()[0])

    def report(self, what):
        self.mark()
        print("%s: device memory free before %.2f GiB, least free %.2f GiB, peak held %.2f GiB"
              % (what, self.free0 / 2 ** 30, self.least_free / 2 ** 30, (self.free0 - self.least_free) / 2 ** 30))

    def alloc(self, n, what):
        try:
            return self.ctx.alloc(n)
        except MemoryError as e:
            raise AssertionError("no device memory for %s: %d elements, %.2f GiB (%s)" % (what, n, 32 * n / 2 ** 30, e))

    def powers(self, first, base, n, out=None, what="a powers sequence"):
        out = self.alloc(n, what) if out is None else out
        self.check(self.L.plonk_fr_powers(self.H, _le32(first), _le32(base), n, out.ptr))
        return out

    def dup(self, buf, what="a copy"):
        c = self.alloc(buf.n, what)
        self.check(self.L.plonk_mem_d2d(self.H, c.ptr, buf.ptr, 32 * buf.n))
        return c

    def zeros(self, n, what):
        z = self.alloc(n, what)
        self.check(self.L.plonk_mem_zero(self.H, z.ptr, 32 * n))
        return z

    def put(self, buf, index, value):
        self.check(self.L.plonk_fr_upload(self.H, buf.at(index), _le32(value), 1))

    def at(self, buf):
        return lambda k: self.ctx.download_ints(buf, 1, offset=k)[0]

    def equal(self, a, b, n, a_off=0, b_off=0):
        eq = ctypes.c_int(0)
        self.check(self.L.plonk_fr_equal(self.H, a.at(a_off), b.at(b_off), n, ctypes.byref(eq)))
        return bool(eq.value)

    def ntt(self, src, dst, log_n, inverse, batch=1):
        self.check(self.L.plonk_fr_ntt(self.H, src.ptr, dst.ptr, log_n, 1 if inverse else 0, batch))

    def sum_of_sequences(self, seq, n, what):
        """[sum_t first_t * base_t^k for k < n] in two buffers: each sequence is added into the first in place"""
        acc = self.powers(seq[0][0], seq[0][1], n, what=what)
        if len(seq) > 1:
            t = self.alloc(n, what + " (one term)")
            for first, base in seq[1:]:
                self.powers(first, base, n, out=t)
                self.check(self.L.plonk_fr_pointwise(self.H, self.OP_ADD, acc.ptr, t.ptr, acc.ptr, n))
            self.mark()
        return acc

    def inverse_of_affine_powers(self, first, base, shift, n, what):
        """[1 / (first * base^k - shift) for k < n], in one buffer"""
        d = self.powers(first, base, n, what=what)
        self.check(self.L.plonk_fr_scalar_op(self.H, self.OP_SUB, d.ptr, _le32(shift), d.ptr, n, 0))
        self.check(self.L.plonk_fr_batch_inverse(self.H, d.ptr, d.ptr, n))
        return d

    # -- inputs and expected vectors of the three plain families
    def input_of(self, fam):
        n = fam.n
        if fam.name == "geometric":
            return self.powers(fam.a, fam.c, n, what="the input")
        if fam.name == "deltas":
            x = self.zeros(n, "the input")
            for j, v in fam.terms:
                self.put(x, j, v)
            return x
        x = self.alloc(n, "the input")  # periodic: b once, then doubled
        self.check(self.L.plonk_fr_upload(self.H, x.ptr, b"".join(_le32(v) for v in fam.b), fam.p))
        have = fam.p
        while have < n:
            self.check(self.L.plonk_mem_d2d(self.H, x.at(have), x.ptr, 32 * have))
            have *= 2
        return x

    def expected_of(self, fam, inverse):
        n, m = fam.n, fam.m
        what = "the expected vector"
        if fam.name == "geometric":  # num / (c wk^k - 1) = 1 / ((c / num) wk^k - 1 / num)
            wk = pow(fam.w, -1, m) if inverse else fam.w
            ninv = pow(fam.numerator(inverse), -1, m)
            return self.inverse_of_affine_powers(fam.c * ninv % m, wk, ninv, n, what)
        if fam.name == "deltas":
            return self.sum_of_sequences(fam.sequences(inverse), n, what)
        e = self.zeros(n, what)  # periodic: p bins, n / p apart
        bins = fam.bins(inverse)
        src = self.ctx.upload_bytes(b"".join(_le32(v) for v in bins))
        q = n // fam.p
        for i in range(fam.p):
            self.check(self.L.plonk_mem_d2d(self.H, e.at(i * q), src.at(i), 32))
        self.ctx.sync()  # (src is released on return)
        return e


def whole_vector_comparison_sees_one_element(ctx, n, indices, seed=0):
    """The checker on the device: plonk_fr_equal over n elements, against a second vector and against zero, turns false for one
    element off by one at each of `indices` alone (and true again once it is put back)."""
    d = Dev(ctx)
    fam = Geometric(1 << 10, 86028121 + seed)
    m = fam.m
    x = d.powers(fam.a, fam.c, n, what="a vector")
    y = d.dup(x)
    z = d.zeros(n, "a zero vector")
    zero = ctypes.c_int(0)

    def is_zero():
        d.check(d.L.plonk_fr_equal(d.H, z.ptr, None, n, ctypes.byref(zero)))
        return bool(zero.value)

    assert d.equal(x, y, n) and is_zero()
    for k in indices:
        want = fam.a * pow(fam.c, k, m) % m
        assert d.at(x)(k) == want, k
        d.put(y, k, (want + 1) % m)
        d.put(z, k, 1)
        assert not d.equal(x, y, n), "plonk_fr_equal over %d elements misses index %d" % (n, k)
        assert not is_zero(), "plonk_fr_equal against zero over %d elements misses index %d" % (n, k)
        d.put(y, k, want)
        d.check(d.L.plonk_mem_zero(d.H, z.at(k), 32))
        assert d.equal(x, y, n) and is_zero(), k


def bn254_plain(ctx, log_n, family, direction, seed=0):
    """One (size, family, direction) cell of plonk_fr_ntt on its automatic plan.  fwd: forward out of place, then back in place;
    inv: the inverse in place on a copy, then forward out of place; fwd_inplace: forward in place on a copy (above 2^26: several
    passes through the library's scratch), then back in place."""
    n = 1 << log_n
    d = Dev(ctx)
    fam = FAMILIES[family](n, 7919 * log_n + seed)
    S = sample_set(n, seed)
    what = "BN254 2^%d %s %s" % (log_n, family, direction)
    inverse = direction == "inv"
    x = d.input_of(fam)
    if direction == "fwd":
        out = d.alloc(n, "the output")
        d.ntt(x, out, log_n, False)
    else:
        out = d.dup(x, "the in-place operand")
        d.ntt(out, out, log_n, inverse)
    e = d.expected_of(fam, inverse)
    d.mark()
    check_output(what, S, fam.closed(inverse), d.at(e), d.at(out), lambda: d.equal(out, e, n))
    del e
    if direction == "inv":
        back = d.alloc(n, "the round trip")
        d.ntt(out, back, log_n, False)
    else:
        back = out
        d.ntt(back, back, log_n, True)
    d.mark()
    if not d.equal(back, x, n):  # step 3
        check_samples(what + ": round trip", S, d.at(x), d.at(back))
        raise AssertionError("%s: the round trip differs from the input outside the sample set" % what)
    d.report(what)


def bn254_forced(ctx, log_n, how, seed=0):
    """Family 1 on a forced plan — how = ("split", r1): the wave kernels as 2^r1 x 2^(log_n - r1); ("kind", 4): the generic LDS
    kernel — equal to the automatic plan's output everywhere (plonk_fr_equal) and to the closed form on S(n); back in place."""
    n = 1 << log_n
    d = Dev(ctx)
    fam = Geometric(n, 104729 * log_n + seed)
    S = sample_set(n, seed)
    what = "BN254 2^%d geometric %s %d" % (log_n, how[0], how[1])
    x = d.input_of(fam)
    auto = d.alloc(n, "the automatic plan's output")
    d.ntt(x, auto, log_n, False)
    forced = d.alloc(n, "the forced plan's output")
    try:
        if how[0] == "split":
            d.check(d.L.plonk_ntt_set_split(d.H, log_n, how[1]))
        else:
            d.check(d.L.plonk_ntt_select_kernel(d.H, how[1]))
        d.ntt(x, forced, log_n, False)
        d.mark()
        check_samples(what, S, fam.closed(False), d.at(forced))
        assert d.equal(forced, auto, n), "%s: differs from the automatic plan's output outside the sample set" % what
        del auto
        d.ntt(forced, forced, log_n, True)
        assert d.equal(forced, x, n), "%s: the round trip differs from the input" % what
    finally:
        if how[0] == "split":
            d.check(d.L.plonk_ntt_set_split(d.H, log_n, 0))
        else:
            d.check(d.L.plonk_ntt_select_kernel(d.H, 0))
    d.report(what)


def bn254_batched(ctx, log_n, batch, rows, kind=0, seed=0):
    """One call of `batch` transforms back to back, the input ONE powers sequence over the whole buffer: row b is family 1 with a
    replaced by a c^(b N).  S(N) of `rows`, then the whole buffer against E, then back in place."""
    N = 1 << log_n
    total = batch * N
    d = Dev(ctx)
    fam = Geometric(N, 15485863 * log_n + seed)
    m = fam.m
    what = "BN254 %d x 2^%d geometric, kind %d" % (batch, log_n, kind)
    x = d.powers(fam.a, fam.c, total, what="the input")
    out = d.alloc(total, "the output")
    try:
        if kind:
            d.check(d.L.plonk_ntt_select_kernel(d.H, kind))
        d.ntt(x, out, log_n, False, batch)
        # E: 1 / (c w^i - 1) over the whole buffer (w^N = 1: the same in every row), then row b times a c^(b N) (c^N - 1)
        e = d.inverse_of_affine_powers(fam.c, fam.w, 1, total, "the expected vector")
        row_factor = [fam.numerator(False) * pow(fam.c, b * N, m) % m for b in range(batch)]
        for b in range(batch):
            d.check(d.L.plonk_fr_scalar_op(d.H, d.OP_MUL, e.at(b * N), _le32(row_factor[b]), e.at(b * N), N, 0))
        d.mark()
        S = [b * N + k for b in rows for k in sample_set(N, seed + b)]
        inv_of = lambda k: pow((fam.c * pow(fam.w, k, m) - 1) % m, -1, m)
        closed = lambda i: row_factor[i // N] * inv_of(i % N) % m
        check_output(what, S, closed, d.at(e), d.at(out), lambda: d.equal(out, e, total))
        del e
        d.ntt(out, out, log_n, True, batch)
        assert d.equal(out, x, total), "%s: the round trip differs from the input" % what
    finally:
        if kind:
            d.check(d.L.plonk_ntt_select_kernel(d.H, 0))
    d.report(what)


def bn254_coset(log_n, seed=0):
    """Family 4 through Polynomial (the default context): n Lagrange values -> 4 n values on the coset -> 4 n coefficients."""
    from plonkathon_amd import Polynomial, Scalar, get_context

    n = 1 << log_n
    d = Dev(get_context())
    sp = SparsePoly(n, 32452843 * log_n + seed)
    what = "BN254 coset 2^%d -> 2^%d" % (log_n, log_n + 2)
    # the Lagrange values, built on the device and pinned on S(n)
    try:
        v = Polynomial.linear_combination([(Polynomial.powers(1, pow(sp.w, e, sp.m), n), a) for e, a in sp.terms])
    except MemoryError as err:
        raise AssertionError("no device memory for the %d sequences of 2^%d Lagrange values (%s)" % (len(sp.terms), log_n, err))
    check_samples(what + ": the Lagrange values", sample_set(n, seed), sp.lagrange(), d.at(v.device()))
    try:
        big = v.to_coset_extended_lagrange(Scalar(sp.off))
    except MemoryError as err:
        raise AssertionError("no device memory for the coset extension to 2^%d values (%s)" % (log_n + 2, err))
    e = d.sum_of_sequences(sp.coset_sequences(), 4 * n, "the expected coset values")
    d.mark()
    S4 = sample_set(4 * n, seed + 1)
    check_output(what, S4, sp.on_coset(), d.at(e), d.at(big.device()), lambda: d.equal(big.device(), e, 4 * n))
    del e
    try:
        back = big.coset_extended_lagrange_to_coeffs(Scalar(sp.off))
    except MemoryError as err:
        raise AssertionError("no device memory for the 2^%d coefficients (%s)" % (log_n + 2, err))
    d.mark()
    for t, a in sp.terms:
        assert back.value_at(t).n == a, "%s and back: coefficient %d is %d, not %d" % (what, t, back.value_at(t).n, a)
    for start, stop in sp.gaps(4 * n):
        if not back.is_zero(start, stop):
            check_samples(what + " and back", [k for k in S4 if start <= k < stop], lambda k: 0, d.at(back.device()))
            raise AssertionError("%s and back: coefficients %d .. %d are not all zero" % (what, start, stop - 1))
    d.report(what)


# ---- BLS12-381 (S(n) only: the field has no device-side operators) ---------------------------------------------------------
def _bls_sparse(n, entries, what):
    """a device vector of n elements, zero but for entries = [(index, value)]: one zeroed buffer of 32 n bytes uploaded"""
    from plonkathon_amd import bls12_381 as bls

    raw = bytearray(32 * n)
    for j, v in entries:
        raw[32 * j : 32 * j + 32] = _le32(v)
    try:
        return bls.upload(bytes(raw))
    except MemoryError as e:
        raise AssertionError("no device memory for %s: %d elements, %.2f GiB (%s)" % (what, n, 32 * n / 2 ** 30, e))


def _bls_at(buf):
    from plonkathon_amd import bls12_381 as bls

    return lambda k: int.from_bytes(bls.download(buf, 1, k), "little")


def bls_deltas(log_n, seed=0):
    """plonk_bls_fr_ntt on family 2: forward out of place on S(n); the inverse in place gives the nine values back and zero elsewhere."""
    from plonkathon_amd import bls12_381 as bls

    n = 1 << log_n
    fam = Deltas(n, 49979687 * log_n + seed, BLS_M, bls_root)
    S = sample_set(n, seed)
    what = "BLS12-381 2^%d deltas" % log_n
    x = _bls_sparse(n, fam.terms, "the input")
    try:
        out = bls.ntt(x, log_n)
    except MemoryError as e:
        raise AssertionError("no device memory for the output of 2^%d elements (%s)" % (log_n, e))
    del x
    check_samples(what + " fwd", S, fam.closed(False), _bls_at(out))
    bls.ntt(out, log_n, True, out=out)
    want = dict(fam.terms)
    check_samples(what + " and back", sorted(set(S) | set(want)), lambda k: want.get(k, 0), _bls_at(out))


def bls_coset(log_n, seed=0):
    """coset_extend / coset_to_coeffs on family 4.  The Lagrange values come from one forward transform of the sparse coefficient
    vector at 2^log_n (on the GPU 2^24: a size test_bls12_381_ntt_exact_at_microbench_sizes pins bit for bit against the C
    oracle); they are checked on S(n) here as well."""
    from plonkathon_amd import bls12_381 as bls

    n = 1 << log_n
    sp = SparsePoly(n, 67867967 * log_n + seed, BLS_M, bls_root)
    what = "BLS12-381 coset 2^%d -> 2^%d" % (log_n, log_n + 2)
    c = _bls_sparse(n, sp.terms, "the coefficients")
    v = bls.ntt(c, log_n)
    del c
    check_samples(what + ": the Lagrange values", sample_set(n, seed), sp.lagrange(), _bls_at(v))
    try:
        big = bls.coset_extend(v, log_n, sp.off)
    except MemoryError as e:
        raise AssertionError("no device memory for the coset extension to 2^%d values (%s)" % (log_n + 2, e))
    del v
    S4 = sample_set(4 * n, seed + 1)
    check_samples(what, S4, sp.on_coset(), _bls_at(big))
    try:
        back = bls.coset_to_coeffs(big, log_n + 2, sp.off)
    except MemoryError as e:
        raise AssertionError("no device memory for the 2^%d coefficients (%s)" % (log_n + 2, e))
    del big
    want = dict(sp.terms)
    check_samples(what + " and back", sorted(set(S4) | set(want)), lambda k: want.get(k, 0), _bls_at(back))
