"""Bodies of the MSM tests on an SRS whose secret is known (oracle.srs.TEST_TAU: test vectors only), shared by
tests/test_emu_msm_known_secret.py (emulated kernels, reduced sizes) and tests/test_gpu_msm_known_secret.py (MI355X).

The reference.  The bases of that SRS are tau^i G, so an MSM of the scalars s_i is (sum_i s_i tau^i mod r) G: one dot product in
Python integers and one scalar multiplication of the Python group law (`expected`) — milliseconds where a reference MSM takes the
better part of a second, which is what lets every row of every batched call below be compared, at sizes that fill workgroups.
Knowing the secret also lets a test CHOOSE the result: solving for the last scalar gives an MSM over n distinct bases whose sum is
exactly the identity, or exactly G.  For arbitrary bases the tests pick the multipliers themselves (bases k_i G, reference
(sum_i s_i k_i) G): `known_points` / `expected_on`.  Nothing here uses the code under test as its own reference.

Parts: (2) structured scalar families through every MSM method; (3) each fast-addition failure site of the comb (MSM_COMB_REDO:
the column tree, the row sum, the column sum) reached with an EMPTY deferred list; (4) the row walk where the library's rule takes
it, every MSM checked; (5) the bucket method's entry encoding at n = 32768; (6) the Lagrange view against the barycentric formula."""
import contextlib
import ctypes
import random

from helpers import R_MOD

import plonkathon_amd as pa
from plonkathon_amd import _lib
from plonkathon_amd._lib import check
from plonkathon_amd.field import Q_MOD, le32
from plonkathon_amd.kzg import _DeviceBases, _msm
from oracle import g1 as og1
from oracle.srs import TEST_TAU
from parity_cases import affine, chain_lines, product_tau_setup

TAU = int(TEST_TAU)
BUCKET_DEFAULT_BITS = 10  # MSM_DEFAULT_WINDOW_BITS of csrc/msm.hip: what msm_configure(0, ..) runs the bucket method on


# ---- 1. the reference ---------------------------------------------------------------------------
_tau_powers = [1]
_expected = {}


def tau_powers(n):
    while len(_tau_powers) < n:
        _tau_powers.append(_tau_powers[-1] * TAU % R_MOD)
    return _tau_powers[:n]


def expected(scalars, n=None):
    """(sum_{i < n} s_i tau^i mod r) G by the Python group law, None (the identity) when the sum is 0; once per input."""
    n = len(scalars) if n is None else n
    key = tuple(scalars[:n])
    if key not in _expected:
        k = sum(s * t for s, t in zip(scalars[:n], tau_powers(n))) % R_MOD
        _expected[key] = og1.multiply(og1.G1, k) if k else None
    return _expected[key]


def designed(head, target, n):
    """head + [s]: the n scalars whose MSM on the known-secret SRS is target G (target = 0: the identity), head being the first n - 1."""
    assert len(head) == n - 1
    pw = tau_powers(n)
    rest = sum(s * t for s, t in zip(head, pw)) % R_MOD
    return list(head) + [(target - rest) * pow(pw[n - 1], -1, R_MOD) % R_MOD]


_known = {}


def known_points(n, seed=4242):
    """([k_i], [k_i G]) for n distinct random multipliers (the Python group law: computed once per process)."""
    ks, pts = _known.setdefault(seed, ([], []))
    rng = random.Random(seed * 7919 + len(ks))
    while len(ks) < n:
        k = rng.randrange(1, R_MOD)
        ks.append(k)
        pts.append(og1.multiply(og1.G1, k))
    return ks[:n], pts[:n]


def expected_on(ks, scalars):
    k = sum(s * m for s, m in zip(scalars, ks)) % R_MOD
    return og1.multiply(og1.G1, k) if k else None


_setups = {}


def tau_setup(n):
    """plonkathon_amd.Setup of tau^i G, i < n (the C oracle's scalar multiplication, spot-checked against the Python group law)."""
    if n not in _setups:
        _setups[n] = product_tau_setup(TAU, n, spot_checks=4)
    return _setups[n]


def run_rows(bases, rows, n=None):
    """One batched plonk_g1_msm call — one launch of every kernel of the method — over `rows`; affine results, None = identity."""
    n = len(rows[0]) if n is None else n
    assert all(len(r) == n for r in rows)
    buf = bases.ctx.upload_ints([s % R_MOD for r in rows for s in r])
    return [affine(p) for p in _msm(bases, buf.ptr, n, len(rows), n)]


def load_points(pts):
    ctx = pa.get_context()
    xy = b"".join(le32(0) + le32(0) if p is None else le32(p[0]) + le32(p[1]) for p in pts)
    h = ctypes.c_void_p()
    check(ctx.L.plonk_srs_load_affine(ctx.handle, xy, len(pts), ctypes.byref(h)))
    return _DeviceBases(ctx, h, len(pts))


# ---- 2. scalar families -------------------------------------------------------------------------
def chain_a_column(n):
    """The A column of a chain-circuit witness (x0 = 3, x_{i+1} = x_i^2) of 2 n / 3 gates, zero padded to n as the prover pads a
    wire column to its group order: large values first, then a run of zeros."""
    from oracle.circuit import Program as OProgram

    m = max(2, 2 * n // 3)
    prog = OProgram(chain_lines(m), 1 << (m - 1).bit_length())
    wit = prog.fill_variable_assignments({"x0": 3})
    wit.setdefault(None, 0)
    col = [wit[wl] % R_MOD for wl, _, _ in prog.wires()]
    return (col + [0] * n)[:n]


def families(n, width, seed=2718):
    """[(name, n scalars)]: what real inputs look like and uniform ones do not — every entry of a window in ONE bucket, long runs
    of empty buckets, fewer entries than lanes (E < lanes) and none at all (E = 0), every comb digit the same, results that are
    exactly the identity or exactly G.  `width`: the method's window bits / teeth."""
    rng = random.Random(seed + 131 * n)
    one = rng.randrange(1, R_MOD)
    low = rng.randrange(1, 1 << width)
    pair = [(1 << 253) + (rng.randrange(1 << 252) | 1) for _ in range(n)]
    out = [
        ("all 0", [0] * n),
        ("single 1 at 0", [1] + [0] * (n - 1)),
        ("single 1 at n-1", [0] * (n - 1) + [1]),
        ("all 1", [1] * n),
        ("all r-1", [R_MOD - 1] * n),
        ("all one random value", [one] * n),
        ("bits, density 1/2", [rng.randrange(2) for _ in range(n)]),
        ("bits, density 1/64", [1 if rng.randrange(64) == 0 else 0 for _ in range(n)]),
        ("below 2^16", [rng.randrange(1 << 16) for _ in range(n)]),
        ("below 2^%d" % width, [rng.randrange(1 << width) for _ in range(n)]),
        ("2^(i mod 254)", [(1 << (i % 254)) % R_MOD for i in range(n)]),
        ("s, r-s alternating", [pair[i // 2] if i % 2 == 0 else R_MOD - pair[i // 2] for i in range(n)]),
        ("equal low %d bits" % width, [(rng.randrange(R_MOD >> width) << width) | low for _ in range(n)]),
        ("chain witness A column", chain_a_column(n)),
        ("designed identity", designed([rng.randrange(R_MOD) for _ in range(n - 1)], 0, n)),
        ("designed G", designed([rng.randrange(R_MOD) for _ in range(n - 1)], 1, n)),
        ("uniform (control)", [rng.randrange(R_MOD) for _ in range(n)]),
    ]
    assert all(len(sc) == n and all(0 <= s < R_MOD for s in sc) for _, sc in out)
    return out


# (kind, window bits / teeth, groups or chunks, flags): every MSM method of csrc/msm.hip
BUCKET = [("bucket", 0, 0, {}), ("bucket", 8, 2, {}), ("bucket", 13, 1, {})]
WINDOWS = [("windows", 11, 0, {})]
COMBS = [(9, False), (11, True)]  # 29 columns plain; 23 columns + joint tables of 6 bases (254 = 23 x 11 + 1)
LANES = [("comb", h, g, {"top": top, "walk": "lanes"}) for h, top in COMBS for g in (1, 4)]  # 4: msm_comb_colsum_kernel runs
WIDE = [("comb", h, g, {"top": top, "walk": "lanes", "wide": True}) for h, top in COMBS for g in (1, 4)]
ROWS = [("comb", h, c, {"top": top, "walk": "rows"}) for h, top in COMBS for c in (1, 2, 3)]
AUTO = [("auto", 0, 0, {})]
METHODS = BUCKET + WINDOWS + LANES + WIDE + ROWS
EMU_COMBS = [(5, False), (7, True)]  # the emulator's: 51 columns plain; 36 columns + joint tables of 2 bases


def method_id(m):
    kind, bits, groups, kw = m
    return "-".join([kind, str(bits), str(groups)] + sorted(k if v is True else str(v) for k, v in kw.items() if v))


@contextlib.contextmanager
def method(kind, bits, groups, kw):
    ctx = pa.get_context()
    try:
        if kind == "bucket":
            ctx.msm_lookup(1)
            ctx.msm_configure(bits, groups)
        elif kind == "windows":
            ctx.msm_lookup(2, bits, 0, windows=True)
            ctx.msm_configure(0, groups)
        elif kind == "comb":
            ctx.msm_lookup(2, bits, 0, **kw)
            ctx.msm_configure(0, groups)
        else:
            ctx.msm_lookup(0)
        yield ctx
    finally:
        ctx.msm_lookup(0)
        ctx.msm_configure(0, 0)


def scalar_families(m, n):
    """Every family as one row of ONE batched call on the known-secret Setup of n bases, through method m; every row against
    `expected`."""
    kind, bits, groups, kw = m
    width = bits if bits else BUCKET_DEFAULT_BITS
    fam = families(n, width)
    bases = tau_setup(n).device_bases()
    with method(*m) as ctx:
        ctx.profile_reset()
        ctx.profile(True)
        try:
            got = run_rows(bases, [sc for _, sc in fam])
        finally:
            ctx.profile(False)
        rowsums = ctx.profile_read("msm_comb_rowsum")[1]
        info = bases.lookup_info()
    if kind == "comb":
        assert (info["layout"], info["bits"], info["top_group"] != 0) == ("comb", bits, bool(kw.get("top"))), info
        assert (rowsums >= 1) == (kw.get("walk") == "rows"), (method_id(m), rowsums)
    elif kind == "windows":
        assert (info["layout"], info["bits"]) == ("windows", bits), info
    for (name, sc), g in zip(fam, got):
        assert g == expected(sc), (method_id(m), n, name)
    by_name = {name: g for (name, _), g in zip(fam, got)}
    assert by_name["all 0"] is None and by_name["designed identity"] is None and by_name["designed G"] == og1.G1


# ---- 3. each comb redo site on its own ----------------------------------------------------------
# Partition (csrc/msm_comb.h).  Row walk with G chunks: chunk c takes the scalars [c per, (c + 1) per), per = ceil(n / G); a lane is
# one (MSM, column) row and walks its chunk serially.  Column-lane kernel with G workgroups per MSM: workgroup g takes the scalars
# [g per, (g + 1) per); inside it q = 256 / a lanes per column take the scalars r, r + q, .. (nothing is left over for the other
# lanes at the sizes below: q p >= per with p = ceil(a per / 256)).  The bases of a layout are pairwise distinct inside every lane's
# share (known_points are distinct random multiples), and a lane's running sum is a sum of table entries of DIFFERENT bases — it equals
# plus or minus the next entry with negligible probability — so no addition is deferred (n_deferred stays 0: it is not readable
# through any entry point, this is the argument) and MSM_DEFER_CAP cannot force the redo: only the MSM_COMB_REDO flag of the site
# the case is built for sends the MSM to msm_comb_slow_kernel.  Without that flag the fast addition leaves its accumulator
# untouched where the operands were equal or opposite, and the result is wrong.
ROWS_COMB = (5, False)   # a = 51 columns (no divisor of 256: a workgroup of the row walk straddles the MSMs of a batch), q = 5
TREE_COMB = (2, False)   # a = 127 columns, q = 2 lanes per column: the tree of a column is ONE addition of its two lanes' pieces


def mirrored(k, negate, seed):
    """2 k bases [P_0 .. P_{k-1}, +-P_{k-1} .. +-P_0] with their multipliers, and scalars mirrored the same way: the two halves have
    equal sums (negate: opposite ones) in every column."""
    ks, pts = known_points(k)
    rng = random.Random(seed)
    half = [rng.randrange(R_MOD) for _ in range(k)]
    sign = -1 if negate else 1
    back = [(x, Q_MOD - y) for x, y in pts[::-1]] if negate else pts[::-1]
    return ks + [sign * m % R_MOD for m in ks[::-1]], pts + back, half + half[::-1]


def interleaved(k, negate, seed):
    """2 k bases [P_0, +-P_{k-1}, P_1, +-P_{k-2}, ..]: the even positions hold P_0 .. P_{k-1}, the odd ones the same points backwards,
    scalars alike — the two lanes of a column of a comb with q = 2 (scalars 0, 2, .. and 1, 3, ..) hold equal / opposite pieces."""
    ks, pts, sc = mirrored(k, negate, seed)
    mix = lambda v: [v[i // 2] if i % 2 == 0 else v[k + i // 2] for i in range(2 * k)]
    return mix(ks), mix(pts), mix(sc)


def _redo(comb, walk, groups, layout, batch):
    ks, pts, sc = layout
    n = len(pts)
    rows = [sc]
    if batch:  # row 1 of three; rows 0 and 2 uniform on the same bases: a flag raised on the wrong MSM leaves row 1 wrong
        rng = random.Random(n + groups)
        rows = [[rng.randrange(R_MOD) for _ in range(n)], sc, [rng.randrange(R_MOD) for _ in range(n)]]
    with method("comb", comb[0], groups, {"top": comb[1], "walk": walk}) as ctx:
        ctx.profile_reset()
        ctx.profile(True)
        try:
            got = run_rows(load_points(pts), rows)
        finally:
            ctx.profile(False)
        assert (ctx.profile_read("msm_comb_rowsum")[1] >= 1) == (walk == "rows")
    for k, (r, g) in enumerate(zip(rows, got)):
        assert g == expected_on(ks, r), (comb, walk, groups, "row %d of %d" % (k, len(rows)))
    return got[1 if batch else 0]


def redo_rowsum(negate, batch):
    """Site: msm_comb_rowsum_kernel (`ok &=` of its butterfly, the atomicOr on n_deferred[row / a]).  Row walk, 2 chunks of 12 scalars
    on mirrored halves: lane 0 of a row's four holds chunk 0's sum, lane 1 chunk 1's, and the first butterfly step adds two equal
    (negate: opposite) points in EVERY row.  No lane meets equal or opposite operands inside its chunk (12 distinct bases)."""
    got = _redo(ROWS_COMB, "rows", 2, mirrored(12, negate, 31), batch)
    assert (got is None) == negate


def redo_colsum(negate, batch):
    """Site: msm_comb_colsum_kernel.  Column-lane kernel, 4 workgroups of 12 scalars per MSM (48 x 51 items: the most that
    msm_groups_per_msm leaves at 4), mirrored halves [A B | B' A']: lanes 0 .. 3 of a column's wave hold the workgroups' sums, the
    step of mask 2 gives lane 0 = A + B' and lane 1 = B + A' — the same point (negate: opposite points) — and the step of mask 1
    adds them.  Inside a workgroup every column's five lanes hold sums over disjoint distinct bases: the tree meets nothing."""
    got = _redo(ROWS_COMB, "lanes", 4, mirrored(24, negate, 32), batch)
    assert (got is None) == negate


def redo_tree(negate, batch):
    """Site: the column tree of msm_comb_kernel (msm_comb.h: `if (!g1l_add_fast(v, o)) atomicOr(.., MSM_COMB_REDO)`).  One workgroup,
    16 scalars on the 2-tooth comb (q = 2, p = 8, nothing left over): lane 0 of a column sums the scalars 0, 2, .., lane 1 the
    scalars 1, 3, .., equal (negate: opposite) by the interleaved layout; the tree's single level adds them."""
    got = _redo(TREE_COMB, "lanes", 1, interleaved(8, negate, 33), batch)
    assert (got is None) == negate


def comb_column_weights(s, h, a):
    """[c_j]: column j of scalar s on the plain comb of h teeth adds c_j R^-1 P (csrc/msm_comb.h: the Montgomery residue s R mod r
    taken as an integer, made odd — r minus it, sign flipped — and written with the digits +-1 of t = (v + 2^L - 1) / 2; column j
    takes the digits j + a k with the weights 2^(a k)).  sum_j 2^j c_j = s R (mod r)."""
    v, sign = s * (1 << 261) % R_MOD, 1
    if v % 2 == 0:
        v, sign = R_MOD - v, -1
    t = (v + (1 << (a * h)) - 1) >> 1
    cs = [sign * sum((2 * ((t >> (j + a * k)) & 1) - 1) << (a * k) for k in range(h)) for j in range(a)]
    assert sum(c << j for j, c in enumerate(cs)) % R_MOD == s * (1 << 261) % R_MOD
    return cs


def redo_horner(butterfly, batch=False):
    """Site: the Horner step of msm_comb_finalize_kernel<16> (`ok &=` of the addition of a column sum; butterfly: of the first
    cross-lane step) and its atomicOr.  CONSTRUCTIBLE, but not from the recoding alone: equal column sums S_j = S_j' do not meet —
    the chain adds 2^16 S_(j+16) to S_j — and for one base the weights c_j of the S_j = c_j R^-1 P are odd and small, so
    2^16 c_16 = c_0 has no solution.  With two bases k_0 G and G and arbitrary scalars the condition is linear in k_0: on the
    8-tooth comb (32 columns, lane l of 16 takes columns l + 16 and l) k_0 is solved from 2^16 S_16 = S_0 — lane 0 adds equal
    points — or, butterfly, from T_0 = 2 T_1 for the lanes' shares T_l = 2^16 S_(16+l) + S_l.  Two scalars in two lanes of every
    column: nothing is deferred, and the tree adds entries of different bases."""
    h, a = 8, 32
    rng = random.Random(657 + butterfly)
    sc = [rng.randrange(1, R_MOD), rng.randrange(1, R_MOD)]
    c0, c1 = comb_column_weights(sc[0], h, a), comb_column_weights(sc[1], h, a)
    if butterfly:
        share = lambda c, l: (c[16 + l] << 16) + c[l]
        num, den = 2 * share(c1, 1) - share(c1, 0), share(c0, 0) - 2 * share(c0, 1)
    else:
        num, den = c1[0] - (c1[16] << 16), (c0[16] << 16) - c0[0]
    k0 = num * pow(den, -1, R_MOD) % R_MOD
    ks, pts = [k0, 1], [og1.multiply(og1.G1, k0), og1.G1]
    _redo((h, False), "lanes", 1, (ks, pts, sc), batch)


# ---- 4. the row walk where the library's rule takes it ------------------------------------------
def rule_batch(n, a):
    """The smallest M at which msm_run_comb's rule takes the row walk for M MSMs of n scalars on a comb of `a` columns (no virtual
    scalars): W = ceil(M a / 256) workgroups of rows, G = 3 slots / W chunks lowered to n / 32, taken when W G >= slots / 2,
    slots = 4 per compute unit."""
    import re

    slots = 4 * int(re.search(r"(\d+) CUs\)", pa.get_context().name()).group(1))
    for M in range(1, 513):
        W = -(-M * a // 256)
        G = max(3 * slots // W, 1)
        if G > n // 32:
            G = max(n // 32, 1)
        if W * G >= slots // 2:
            return M
    return None


def row_walk_by_the_rule(n=2048, teeth=12):
    """M MSMs of n scalars on the forced 12-tooth comb (22 columns, 268 MB at n = 2048), M the smallest batch the rule gives the row
    walk (82 on 256 compute units: W = 8 workgroups of rows x 64 chunks); uniform rows with every family dealt in at positions spread
    over the batch — rows 0 and M - 1, and the rows on both sides of the first workgroup boundary (row 256 / 22: MSM 11 straddles it).
    ALL M results against `expected`; then M = 4 in one call, which the rule leaves to the column-lane kernel."""
    a = -(-254 // teeth)
    M = rule_batch(n, a)
    walk = "rows" if M is None else None  # (no M <= 512 takes it: force the walk, the rule's chunk count, M = 512)
    M = 512 if M is None else M
    fam = families(n, teeth)
    assert M >= len(fam) + 4
    rng = random.Random(12 * n)
    rows = [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(M)]
    edge = 256 // a  # the MSM that straddles the first workgroup boundary of the row walk
    spots = [0, M - 1, edge - 1, edge, edge + 1]
    spots += [k for k in sorted(range(M), key=lambda k: (k * 37) % M) if k not in spots][:len(fam) - len(spots)]
    for k, (_, sc) in zip(spots, fam):
        rows[k] = sc
    bases = tau_setup(n).device_bases()
    with method("comb", teeth, 0, {"walk": walk}) as ctx:
        def run(rs):
            ctx.profile_reset()
            ctx.profile(True)
            try:
                got = run_rows(bases, rs)
            finally:
                ctx.profile(False)
            return got, ctx.profile_read("msm_comb_rowsum")[1], ctx.profile_read("msm_comb")[1]

        got, rowsums, combs = run(rows)
        assert rowsums >= 1 and rowsums == combs, (M, rowsums, combs)
        small, rowsums4, combs4 = run([rows[k] for k in spots[:4]])
        assert rowsums4 == 0 and combs4 >= 1, (rowsums4, combs4)
        if walk is None and M > 1:  # M is the smallest: one MSM fewer keeps the column-lane kernel
            _, rowsums_less, _ = run(rows[:M - 1])
            assert rowsums_less == 0, (M - 1, rowsums_less)
    bad = [k for k in range(M) if got[k] != expected(rows[k])]
    assert not bad, (M, bad)
    assert small == [expected(rows[k]) for k in spots[:4]]


# ---- 5. the bucket method's entry encoding ------------------------------------------------------
def bucket_entry_boundary():
    """Entries are base index in bits 0 .. 14, sign in bit 15: n = 32768 is the last size, index 32767 with a negative digit the
    entry 0xffff.  Uniform scalars; only index 32767 non-zero, with 1 and with r - 1 (= -1: a negative digit on the top index);
    n = 32769 is refused with PLONK_ERR_ARG and the context works afterwards."""
    from large_prover_cases import device_tau_setup

    n = 32768
    ctx = pa.get_context()
    try:
        ctx.msm_lookup(1)  # before the first MSM: no table is built for the 32769 bases
        bases = device_tau_setup(n + 1, TAU).device_bases()
        rng = random.Random(32768)
        rows = [[rng.randrange(R_MOD) for _ in range(n)], [0] * (n - 1) + [1], [0] * (n - 1) + [R_MOD - 1]]
        got = run_rows(bases, rows)
        for k, r in enumerate(rows):
            assert got[k] == expected(r), k
        assert got[2] == og1.neg(got[1])
        buf = ctx.upload_ints(rows[1] + [1])
        xy, flags = ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)
        assert ctx.L.plonk_g1_msm(ctx.handle, bases.handle, buf.ptr, n + 1, 1, n + 1, xy, flags) == _lib.PLONK_ERR_ARG
        assert run_rows(bases, [rows[0][:300]]) == [expected(rows[0], 300)] and run_rows(bases, rows[1:2]) == got[1:2]
    finally:
        ctx.msm_lookup(0)


# ---- 6. the Lagrange view -----------------------------------------------------------------------
def lagrange_at_tau(log_n):
    """[L_i(tau)]: (tau^n - 1) w^i / (n (tau - w^i)) in Python integers."""
    from oracle.field import root_of_unity

    n = 1 << log_n
    w = int(root_of_unity(n))
    zh = (pow(TAU, n, R_MOD) - 1) * pow(n, -1, R_MOD) % R_MOD
    out, wi = [], 1
    for _ in range(n):
        out.append(zh * wi % R_MOD * pow(TAU - wi, -1, R_MOD) % R_MOD)
        wi = wi * w % R_MOD
    assert sum(out) % R_MOD == 1
    return out


def lagrange_view(setup, log_n):
    """MSMs of Lagrange values over bases.lagrange(log_n) equal P(tau) G, P(tau) = sum_i v_i L_i(tau): the unit vectors e_0, e_1,
    e_{n-1}, one uniform vector, and all ones (the result is G).  Bucket method: the check is of the view's points."""
    n = 1 << log_n
    lag = lagrange_at_tau(log_n)
    rng = random.Random(log_n)
    unit = lambda i: [1 if j == i else 0 for j in range(n)]
    rows = [unit(0), unit(1), unit(n - 1), [rng.randrange(R_MOD) for _ in range(n)], [1] * n]
    ctx = pa.get_context()
    try:
        ctx.msm_lookup(1)
        got = run_rows(setup.device_bases().lagrange(log_n), rows)
    finally:
        ctx.msm_lookup(0)
    for k, r in enumerate(rows):
        assert got[k] == expected_on(lag, r), (log_n, k)
    assert got[4] == og1.G1
