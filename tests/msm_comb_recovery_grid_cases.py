"""Bodies of the tests of the comb MSM's RECOVERY LIST (csrc/msm_comb.h: msm_comb_finalize_kernel appends the index of every MSM to
be redone, msm_comb_slow_kernel strides over the list on a fixed grid of 16 workgroups), shared by
tests/test_emu_msm_comb_recovery_grid.py and tests/test_gpu_msm_comb_recovery_grid.py.

Bases.  n = 300 points of the known-secret SRS of tests/msm_known_secret_cases.py (tau^i G), laid out so that chosen rows of a batch
CAN be forced into recovery — on tau^0 G .. tau^299 G themselves nothing ever is: the bases are pairwise distinct and no sum of table
entries meets another.  `folded(n_total)`: [A B | B' A'], the SRS's first points followed by the same points backwards (B' = B
reversed, A' = A reversed), A padded with identity bases so that the halves fall on the kernels' own cuts: the row walk at 2 chunks
cuts the n_total scalars (the virtual scalars of a comb with top tables included) at ceil(n_total / 2), the column-lane kernel at 4
workgroups per MSM at multiples of ceil(n_total / 4).  The multiplier of base i is tau^e(i) (0 for an identity base) and the
reference of every row is (sum_i s_i tau^e(i)) G — `want`, a dot product in Python integers and one scalar multiplication of the
Python group law, never the code under test.

Rows.  A FLAGGED row has scalars folded the same way, so both halves have the same sum in every column: the first butterfly step of
msm_comb_rowsum_kernel (2 chunks) or the last of msm_comb_colsum_kernel (4 workgroups: lanes hold A, B, B', A'; the step of mask 2
leaves A + B' and B + A') adds equal points and sets MSM_COMB_REDO with an empty deferred list.  Its Montgomery residues are odd and
below 2^253, so on the comb with top tables every top code is zero and the virtual scalars add nothing to either half.  A PLAIN row
is uniform: no lane's sum of entries of distinct bases meets its next entry (negligible probability), nothing is deferred, nothing
flagged — so the counter of the recovery list (plonk_msm_recovery_count) reads exactly the number of flagged rows.
The OVERFLOW row is on a base set of its own: one base repeated 300 times with the scalars s, -s, s, -s ..: every addition of a
lane after its first meets the operand it holds or its opposite and is deferred — far more than MSM_DEFER_CAP = 256 of them, and
no flag is needed to send the MSM to recovery."""
import random

from helpers import R_MOD

import msm_known_secret_cases as ks
from oracle import g1 as og1

N = 300
COMBS = [(9, False), (11, True)]  # 29 columns plain; 23 columns + joint tables of 6 bases
R_INV = pow(1 << 261, -1, R_MOD)  # the scalars reach the digits kernel as Montgomery residues s 2^261 mod r


def comb_id(c):
    return "%d teeth%s" % (c[0], " top" if c[1] else "")


def n_total(comb):
    """Scalars the accumulation kernels see for N real ones: the virtual scalars of the top tables included (csrc/msm_comb.h)."""
    h, top = comb
    if not top:
        return N
    a = 254 // h
    g, b, entries = 0, (2 << (254 - a * h)) - 1, 1
    while entries * b <= 1 << (h - 1):
        entries *= b
        g += 1
    return N + -(-(-(-N // g)) // a)


_points = []


def srs_points(k):
    while len(_points) < k:
        _points.append(og1.multiply(og1.G1, ks.tau_powers(len(_points) + 1)[-1]))
    return _points[:k]


def folded(comb):
    """(exponent e(i) of base i or None for an identity base, the N points): [A pad | B | B' | A']."""
    quarter = -(-n_total(comb) // 4)
    assert -(-n_total(comb) // 2) == 2 * quarter  # the row walk's cut at 2 chunks is the column-lane kernel's second cut at 4
    la = N - 3 * quarter  # A' is what is left of the real scalars after three whole quarters
    assert 0 < la <= quarter
    exps = list(range(la)) + [None] * (quarter - la) + list(range(la, la + quarter))
    exps += list(range(la + quarter - 1, la - 1, -1)) + list(range(la - 1, -1, -1))
    assert len(exps) == N
    pts = srs_points(la + quarter)
    return exps, [None if e is None else pts[e] for e in exps]


_want = {}


def want(exps, row):
    key = (tuple(exps), tuple(row))
    if key not in _want:
        pw = ks.tau_powers(max(N, len(row)))
        k = sum(s * pw[e] for s, e in zip(row, exps) if e is not None) % R_MOD
        _want[key] = og1.multiply(og1.G1, k) if k else None
    return _want[key]


def flagged_row(exps, seed):
    """Scalars folded like the bases; residues odd and below 2^253 (no top code, no parity fold)."""
    rng = random.Random(seed)
    by_exp = {}
    row = []
    for i, e in enumerate(exps):
        key = e if e is not None else ("pad", i)
        if key not in by_exp:
            by_exp[key] = (rng.randrange(1 << 252) * 2 + 1) * R_INV % R_MOD
        row.append(by_exp[key])
    return row


def plain_row(seed):
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(N)]


def batch_rows(exps, M, flagged):
    return [flagged_row(exps, 1000 + k) if k in flagged else plain_row(2000 + k) for k in range(M)]


FORMS = [("rows", 2), ("lanes", 4)]  # the row walk at 2 chunks; the column-lane kernel at 4 workgroups per MSM


_loaded = {}


def run(comb, walk, groups, pts, rows):
    """-> (results, recovery counts after each call): one batched call per element of `rows` (a list of batches) on ONE context."""
    got, counts = [], []
    with ks.method("comb", comb[0], groups, {"top": comb[1], "walk": walk}) as ctx:
        key = (id(ctx), tuple(pts))  # one upload (and one table per comb) of a base set per context
        if key not in _loaded:
            _loaded[key] = (ctx, ks.load_points(pts))  # (the context is kept with it: its id stays its own)
        bases = _loaded[key][1]
        ctx.profile_reset()
        ctx.profile(True)
        try:
            for batch in rows:
                got.append(ks.run_rows(bases, batch))
                counts.append(ctx.msm_recovery_count())
        finally:
            ctx.profile(False)
        assert (ctx.profile_read("msm_comb_rowsum")[1] >= 1) == (walk == "rows")
    return got, counts


def check(exps, batch, got, tag):
    bad = [k for k, (r, g) in enumerate(zip(batch, got)) if g != want(exps, r)]
    assert not bad, (tag, bad)


def flagged_batch(comb, form, flagged=(0, 17, 39), M=40):
    """40 MSMs, rows 0, 17 and 39 flagged: an index beyond the grid of 16 workgroups, and entries 0 .. 2 of the list whichever rows
    they hold — three workgroups redo one MSM each, the others read the counter and leave.  Every row against the reference: a
    flagged row is WRONG unless it is redone (the fast addition leaves its accumulator untouched), a plain row must not be touched."""
    exps, pts = folded(comb)
    batch = batch_rows(exps, M, set(flagged))
    (got,), (count,) = run(comb, form[0], form[1], pts, [batch])
    check(exps, batch, got, (comb, form))
    assert count == len(flagged), (comb, form, count)


def nothing_flagged(comb, form, M=40):
    exps, pts = folded(comb)
    batch = batch_rows(exps, M, set())
    (got,), (count,) = run(comb, form[0], form[1], pts, [batch])
    check(exps, batch, got, (comb, form))
    assert count == 0, (comb, form, count)


def all_flagged(comb, form, M=17):
    """17 MSMs all flagged: more listed MSMs than workgroups — workgroup 0 redoes entries 0 and 16 of the list."""
    exps, pts = folded(comb)
    batch = batch_rows(exps, M, set(range(M)))
    (got,), (count,) = run(comb, form[0], form[1], pts, [batch])
    check(exps, batch, got, (comb, form))
    assert count == M, (comb, form, count)


def two_calls(comb, form, M=40):
    """Flagged rows in the first call, none in the second, on one context and one scratch: the counter must not carry over (a
    stale list would have rows 0, 17 and 39 of the second call redone — harmless — but a stale COUNT read past a fresh list)."""
    exps, pts = folded(comb)
    first, second = batch_rows(exps, M, {0, 17, 39}), batch_rows(exps, M, set())
    got, counts = run(comb, form[0], form[1], pts, [first, second])
    check(exps, first, got[0], (comb, form, "first call"))
    check(exps, second, got[1], (comb, form, "second call"))
    assert counts == [3, 0], (comb, form, counts)


def overflow(comb, walk, groups):
    """One MSM whose deferred list overflows (see the module's header): 299 deferred additions per column against a cap of 256.  The
    last scalar differs, so the result is (s + t) tau G and not the identity."""
    rng = random.Random(77 + comb[0])
    s, t = rng.randrange(1, R_MOD), rng.randrange(1, R_MOD)
    row = [s if i % 2 == 0 else R_MOD - s for i in range(N - 1)] + [t]
    exps, pts = [1] * N, [srs_points(2)[1]] * N
    (got,), (count,) = run(comb, walk, groups, pts, [[row]])
    check(exps, [row], got, (comb, walk, "overflow"))
    assert got[0] is not None and count == 1, (comb, walk, count)


# ---- the same list behind msm_slow_kernel: the bucket method and the window tables -----------------------------------------------
# Neither has a redo flag: only a deferred list past MSM_DEFER_CAP sends an MSM to recovery.  Forced with ONE base repeated 600 times
# and the scalar 1: its recoding has a single non-zero digit (window 0, digit 1), so every item that adds anything adds the same
# point.  At one workgroup per MSM (groups = 1) a lane of the window kernel takes the scalars t, t + 256, t + 512 and a lane of the
# bucket method three consecutive entries of bucket 1: every addition after a lane's first meets the point it holds — 344 deferred
# additions per MSM against the cap of 256.  The last scalar is arbitrary, so the result is (599 + t) tau G.
N_WIDE = 600
OTHER_METHODS = [("bucket", 0, 1, {}), ("windows", 11, 1, {})]
EMU_OTHER_METHODS = [("bucket", 0, 1, {}), ("windows", 4, 1, {})]


def other_methods(m, M=17):
    """17 MSMs that all overflow (more than the recovery kernel's 16 workgroups), then, on the same context, 20 uniform MSMs on the
    300 distinct points of the known-secret SRS: counts 17, then 0 — the counter does not carry over — and every result right."""
    rng = random.Random(600 + m[1])
    over = [[1] * (N_WIDE - 1) + [rng.randrange(1, R_MOD)] for _ in range(M)]
    exps = [1] * N_WIDE
    plain = [plain_row(3000 + k) for k in range(20)]
    with ks.method(*m) as ctx:
        got = ks.run_rows(ks.load_points([srs_points(2)[1]] * N_WIDE), over)
        first = ctx.msm_recovery_count()
        got_plain = ks.run_rows(ks.tau_setup(N).device_bases(), plain)
        second = ctx.msm_recovery_count()
    check(exps, over, got, (ks.method_id(m), "overflow"))
    bad = [k for k, (r, g) in enumerate(zip(plain, got_plain)) if g != ks.expected(r)]
    assert not bad, (ks.method_id(m), bad)
    assert (first, second) == (M, 0), (ks.method_id(m), first, second)
