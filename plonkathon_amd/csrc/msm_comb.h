// msm_comb.h — fixed-base MSM on COMB tables (round 5).
//
// Same job as the window tables of msm_windows.h (ec_lincomb over a reusable SRS, /root/reference/curve.py:38-111 and
// setup.py:66-72), fewer additions per base for the same memory.  With h teeth spaced a = ceil(254 / h) bits apart,
// a scalar s is cut into a columns of h bits:  s = sum_{j < a} 2^j  sum_{k < h} b_(j + a k) 2^(a k),  and
//     s P = sum_j 2^j  E_P[ bits j, j + a, j + 2a, .. ]      with ONE table per base,  E_P[idx] = sum_k (+-) 2^(a k) P.
// The a - 1 doublings of the outer sum are shared by all the bases of an MSM (they are done once per MSM on the a column sums),
// so an MSM of N bases costs N * a additions — against N * ceil(255 / c) for the window tables, whose table of the same size
// holds ceil(255 / c) windows of c bits where this one holds a single "window" of h bits:
//     2^11 bases     68.7 GB: h = 20, 13 additions per base   (windows: c = 16, 16 additions; c = 17 needs 128.8 GB for 15)
//                     8.6 GB: h = 17, 15 additions            (windows: c = 12/13, 22/20 additions)
//                     67 MB:  h = 10, 26 additions            (what the bucket method does with a sort and a bucket reduction)
// Signed digits without a zero digit: the scalar is made odd (s even: r - s, and the base's sign flips; r is odd), then written
// with all digits +-1:  s = sum_j b_j 2^j, b_j = 2 t_j - 1, t = (s + 2^L - 1) / 2, L = a h.  A column whose top tooth is -1 is
// the negated entry of the complemented lower teeth, so the table has 2^(h-1) entries per base,
//     E_P[idx] = 2^(a (h-1)) P + sum_{k < h-1} (idx_k ? + : -) 2^(a k) P,
// and EVERY (scalar, column) item is exactly one mixed addition: no zero digits, no branches in the loop.
// The table is built over P'_i = R^-1 P_i (R = 2^261, the Montgomery radix of Fr): the scalars reach the MSM as Montgomery residues
// s R mod r, and (s R) (R^-1 P) = s P — the digit kernel takes the residue as it is, sparing a conversion (a quarter of its work).
//
// With TOP TABLES (round 6, below: "combs with top tables") the comb has floor(254 / h) columns and the one or two bits they leave over
// go through joint tables of g bases each: 21 teeth, 12 columns, g = 7 — 12.15 additions per base of 2^11 from 157.6 GB.
//
// Kernels (one launch each per batch of MSMs):
//   msm_comb_digits_kernel<H, TOP>  one lane per scalar: the residue as stored, parity fold, t, and the a column indices (sign in bit 31)
//                               written column-major (digits[m][j][i], 4 B per item) — read back coalesced by the next kernel;
//                               TOP: a workgroup takes whole groups of g scalars and adds the digits of the virtual scalars
//   msm_comb_kernel             one workgroup per (MSM, scalar sub-range).  Lanes are bound to COLUMNS (a lane's accumulator can
//                               only hold one column's sum): q = 256 / a lanes per column walk scalars r, r + q, .. — the whole
//                               chip reads the tables of q consecutive bases at a time (address translation: msm_windows.h,
//                               msm_lookup_kernel) — for p = ceil(a n / 256) steps, and the 256 - a q lanes left over take the
//                               scalars the columns' lanes did not reach, column after column, leaving one partial sum
//                               ("piece") in LDS per column they touch.  Every lane performs p additions (+-0): 104 for 2^11
//                               scalars in 13 columns.  The pieces are tree-reduced per column through LDS; the workgroup
//                               stores a column sums.
//   msm_comb_rows_kernel        the accumulation of a BATCH (the row walk; msm_run_comb's rule chooses): lanes bound to (MSM, column)
//                               rows, a workgroup = 256 consecutive rows x one chunk of the scalars, the whole chip on one base's
//                               block per step; digits item-major; no LDS, no tree.  msm_comb_rowsum_kernel adds a row's chunks.
//   msm_comb_colsum_kernel      (only when an MSM is cut into >= 4 workgroups) a wave per (MSM, column) sums the workgroups' sums
//   msm_comb_finalize_kernel    sum_j 2^j S_j by Horner over groups of LPM lanes per MSM, deferred additions, unique affine form; an
//                               addition of OPPOSITE operands gives the identity here (an MSM whose result is the identity — all
//                               scalars zero — cancels in these last additions, not before)
//   msm_comb_slow_kernel        the recovery path of MSM_DEFER_CAP / MSM_COMB_REDO (general formulas throughout): 16 workgroups over the
//                               list of MSMs that msm_comb_finalize_kernel found in need of it — empty in a prover's calls
// Table build: msm_comb_scale_kernel gives P'_i; msm_table_kernel G_k = 2^(a k) P'_i; msm_comb_fill_kernel walks each run of 2^8 consecutive indices in
// Gray-code order (one mixed addition of +-2 G_k per entry); g1_batch_to_affine_kernel converts a chunk of bases at a time;
// msm_comb_top_base_kernel / msm_comb_top_fill_kernel: the joint tables, one block of 2^(h-1) entries per group behind the bases' blocks.
#pragma once
#include <utility>

#include "msm_common.h"

#define MSM_COMB_MAX_TEETH 24
#define MSM_COMB_SEG_BITS 8
#define MSM_COMB_SCALAR_BITS 254   // r < 2^254
// n_deferred[m]: the number of deferred additions of MSM m in the low bits (the list holds the first MSM_DEFER_CAP of them), and this
// flag when a tree / Horner addition met equal or opposite operands.  Either way past the cap: msm_comb_slow_kernel redoes the MSM.
#define MSM_COMB_REDO 0x80000000u
PLONK_HD bool msm_comb_needs_redo(uint32_t v) { return (v & MSM_COMB_REDO) != 0 || v > MSM_DEFER_CAP; }
// The MSMs to be redone go to the call's recovery list (msm_common.h): msm_comb_finalize_kernel appends, msm_comb_slow_kernel redoes.

// A digit of this value stands for an item whose table entry is the identity — an identity base, the all-zero code of a group of
// the top tables, a group past the last scalar — and every kernel that reads digits passes it over without a load.  No real item
// has it: a real scalar's digit is an index below 2^(h-1) <= 2^23 beside bit 31, and a virtual scalar's digit has bit 31 clear and
// stays below (virtual (a - 1) + 1) << (h-1), which msm_comb_top_reach_ok keeps below 2^31 - ((a - 1) << (h-1)).
#define MSM_COMB_SKIP 0xffffffffu
struct alignas(16) MsmCombDigit4 { uint32_t d[4]; };  // four digits of consecutive rows: one 16-byte store (item-major layout)

PLONK_HD unsigned msm_comb_columns(unsigned h) { return (MSM_COMB_SCALAR_BITS + h - 1) / h; }

// ---- combs with TOP TABLES (round 6) -----------------------------------------------------------
// ceil(254 / h) rounds up: 20 teeth need 13 columns (260 positions for 254 bits), and the next count of columns, 12, needs 22
// teeth — 275 GB for 2^11 bases.  21 teeth x 12 columns cover 252 bits; the two bits left over are worth one addition per base
// if they get a column of their own, but only 1 / g of one when g bases share a joint table for them:
//     s' = v + 2^L u,  L = a h,  v = s' mod 2^L (odd: all digits +-1 as before),  u = s' >> L in [0, 2^R),  R = 254 - L  (1 or 2)
//     sum_i s'_i P_i = (the comb over the v_i)  +  sum_groups  T_grp[ codes of its g bases ],
//     T_grp[idx] = sum_pos code_pos 2^(L - j) P'_(g grp + pos),   code = +-u in [-(2^R - 1), 2^R - 1]  (B = 2^(R+1) - 1 values),
//     idx = sum_pos (code_pos + (B - 1) / 2) B^pos  <  B^g <= 2^(h-1).
// Group grp is dealt to column j = grp mod a (hence the 2^(L - j): the Horner step multiplies column j's sum by 2^j), as the
// "virtual scalar" n + grp / a of that column: msm_comb_kernel sees an MSM of n + ceil(ceil(n / g) / a) scalars and runs
// unchanged — its table simply has one more 2^(h-1)-entry block per group behind the blocks of the N bases (block N + grp), and
// a virtual scalar's digit carries the block offset (v (a - 1) + j) beside idx: scalar n + v starts from block N + v (the kernels add
// top_delta = N - n to the index of a virtual scalar, msm_comb_block_of), and N + v + v (a - 1) + j = N + grp.  2^11 bases, h = 21: 12 columns of 2 073
// (virtual) scalars = 12.15 additions per base from 137.4 + 20.1 GB, against 13 from 68.7 GB.
struct MsmCombShape {
    unsigned h, a;                // teeth, columns
    unsigned top_bits, top_g;     // R and g (0, 0: no top tables — a = ceil(254 / h))
    unsigned top_b;               // B = 2^(R+1) - 1
    uint32_t top_entries;         // B^g
};
PLONK_HD constexpr MsmCombShape msm_comb_shape(unsigned h, bool top) {
    MsmCombShape s{h, (MSM_COMB_SCALAR_BITS + h - 1) / h, 0, 0, 0, 0};
    if (!top) return s;
    s.a = MSM_COMB_SCALAR_BITS / h;
    s.top_bits = MSM_COMB_SCALAR_BITS - s.a * h;
    s.top_b = (2u << s.top_bits) - 1;
    s.top_entries = 1;
    while (s.top_bits && (uint64_t)s.top_entries * s.top_b <= ((uint64_t)1 << (h - 1))) {
        s.top_entries *= s.top_b;
        s.top_g++;
    }
    return s;
}
// a comb of h teeth can take top tables: one or two bits left over, and a block holds the joint table of at least one base
PLONK_HD constexpr bool msm_comb_top_ok(unsigned h) {
    const MsmCombShape s = msm_comb_shape(h, true);
    return h >= 2 && s.a >= 1 && s.top_bits >= 1 && s.top_bits <= 2 && s.top_g >= 1;
}
PLONK_HD size_t msm_comb_top_groups(size_t n, unsigned g) { return g ? (n + g - 1) / g : 0; }
// virtual scalars per column of an MSM of n scalars (= virtual blocks per column of a table of n bases)
PLONK_HD size_t msm_comb_virtual(size_t n, const MsmCombShape& s) { return s.top_g ? (msm_comb_top_groups(n, s.top_g) + s.a - 1) / s.a : 0; }
// blocks of 2^(h-1) entries in the table of n bases
PLONK_HD size_t msm_comb_blocks(size_t n, const MsmCombShape& s) { return n + msm_comb_virtual(n, s) * s.a; }
// a virtual scalar's digit carries its block offset (v (a - 1) + j) beside the index: 31 bits in all
PLONK_HD bool msm_comb_top_reach_ok(size_t n, const MsmCombShape& s) {
    return !s.top_g || ((uint64_t)(msm_comb_virtual(n, s) * (s.a - 1) + s.a) << (s.h - 1)) < ((uint64_t)1 << 31);
}
// block of the table an item of scalar i (real: i < n_real; virtual: the others) starts from
PLONK_HD size_t msm_comb_block_of(size_t i, size_t n_real, size_t top_delta) { return i + (i >= n_real ? top_delta : 0); }

// c P by double-and-add over the bits of a wave-uniform constant (c = R^-1 mod r, 254 bits): one-off, per base
struct MsmCombScale { uint32_t c[8]; };
PLONK_DEV G1Xyzz msm_comb_scaled_base(const G1Affine& P, const MsmCombScale& k) {
    G1Xyzz acc = g1_xyzz_identity();
#pragma unroll 1
    for (int bit = 255; bit >= 0; bit--) {
        g1_dbl(acc);
        if ((k.c[bit >> 5] >> (bit & 31)) & 1u) g1_madd<true>(acc, P);
    }
    return acc;
}
__global__ void __launch_bounds__(64) msm_comb_scale_kernel(const G1Affine* bases, size_t n, MsmCombScale k, G1Xyzz* out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        G1Affine b;
        b.x = fp_load(&bases[i].x);
        b.y = fp_load(&bases[i].y);
        out[i] = msm_comb_scaled_base(b, k);
    }
}

// E_P[idx] by the definition (signed Horner from the top tooth): used by the verification of a shared table only
PLONK_DEV G1Xyzz msm_comb_entry_slow(const G1Affine& P, unsigned a, unsigned h, uint32_t idx) {
    G1Xyzz acc = g1_xyzz_from_affine(P);
    const G1Affine N = g1_affine_is_identity(P) ? P : g1_affine_neg(P);
#pragma unroll 1
    for (int k = (int)h - 2; k >= 0; k--) {
#pragma unroll 1
        for (unsigned d = 0; d < a; d++) g1_dbl(acc);
        g1_madd<true>(acc, ((idx >> k) & 1) ? P : N);
    }
    return acc;
}

// out[k * n + i] = 2 * cb[k * n + i]  (the Gray-code steps of the fill), XYZZ
__global__ void msm_comb_delta_kernel(const G1Affine* cb, size_t count, G1Xyzz* out) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (size_t)gridDim.x * blockDim.x) {
        G1Affine b;
        b.x = fp_load(&cb[t].x);
        b.y = fp_load(&cb[t].y);
        out[t] = g1_affine_is_identity(b) ? g1_xyzz_identity() : g1_dbl_affine(b);
    }
}

// tmp[(i - i0) << (h-1) | idx] = E_{P_i}[idx] for the bases i0 .. i0 + nb - 1, XYZZ.  cb[k n + i] = 2^(a k) P_i (k < h),
// cd[k n + i] = 2^(a k + 1) P_i (k < sb), both affine.  A lane fills a run of 2^sb consecutive indices: the first entry from the
// h tooth points, the others in Gray-code order, each one mixed addition of +-2 G_k away from the previous one.
__global__ void __launch_bounds__(64) msm_comb_fill_kernel(const G1Affine* cb, const G1Affine* cd, size_t n, size_t i0, size_t nb, unsigned h,
                                                           unsigned sb, G1Xyzz* tmp) {
    const size_t nseg = (size_t)1 << (h - 1 - sb), seg_len = (size_t)1 << sb;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < nb * nseg; id += (size_t)gridDim.x * blockDim.x) {
        const size_t bi = id / nseg, i = i0 + bi, idx0 = (id % nseg) << sb;
        G1Affine t;
        t.x = fp_load(&cb[(size_t)(h - 1) * n + i].x);
        t.y = fp_load(&cb[(size_t)(h - 1) * n + i].y);
        G1Xyzz acc = g1_xyzz_from_affine(t);
#pragma unroll 1
        for (unsigned k = 0; k + 1 < h; k++) {
            t.x = fp_load(&cb[(size_t)k * n + i].x);
            t.y = fp_load(&cb[(size_t)k * n + i].y);
            if (!((idx0 >> k) & 1)) t.y = fp_neg(t.y);
            g1_madd<true>(acc, t);
        }
        G1Xyzz* out = tmp + (bi << (h - 1)) + idx0;
        out[0] = acc;
#pragma unroll 1
        for (uint32_t s = 1; s < seg_len; s++) {
            const unsigned b = (unsigned)__builtin_ctz(s);
            const uint32_t gray = s ^ (s >> 1);
            t.x = fp_load(&cd[(size_t)b * n + i].x);
            t.y = fp_load(&cd[(size_t)b * n + i].y);
            if (!((gray >> b) & 1)) t.y = fp_neg(t.y);
            g1_madd<true>(acc, t);
            out[gray] = acc;
        }
    }
}

// ---- top tables: build ----
// out[i] = 2^(L - j) P'_i, j = (i / g) mod a: the tooth point of base i in the joint table of its group (XYZZ)
__global__ void __launch_bounds__(64) msm_comb_top_base_kernel(const G1Affine* pb, size_t n, unsigned L, unsigned a, unsigned g, G1Xyzz* out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        G1Affine b;
        b.x = fp_load(&pb[i].x);
        b.y = fp_load(&pb[i].y);
        G1Xyzz p = g1_xyzz_from_affine(b);
        const unsigned j = (unsigned)((i / g) % a);
#pragma unroll 1
        for (unsigned k = 0; k < L - j; k++) g1_dbl(p);
        out[i] = p;
    }
}
PLONK_DEV G1Affine msm_comb_top_point(const G1Affine* tq, size_t n, size_t i, bool neg) {
    G1Affine q = g1_affine_identity();
    if (i < n) {
        q.x = fp_load(&tq[i].x);
        q.y = fp_load(&tq[i].y);
        if (neg && !g1_affine_is_identity(q)) q.y = fp_neg(q.y);
    }
    return q;
}
// tmp[(grp - g0) << hb | idx] = T_grp[idx], idx < B^g, for the groups g0 .. g0 + ng - 1 (XYZZ; the caller zeroes tmp: the entries
// from B^g up stay the identity).  tq: the n tooth points, affine.  A lane fills a run of B^2 consecutive indices (B when a
// group is one base): the higher digits' share first, then the two low digits from (-c, -c) upwards in boustrophedon order, so that
// every entry is one mixed addition of +-Q away from the one before.
__global__ void __launch_bounds__(64) msm_comb_top_fill_kernel(const G1Affine* tq, size_t n, size_t g0, size_t ng, unsigned hb, unsigned g, unsigned B,
                                                               uint32_t entries, G1Xyzz* tmp) {
    const unsigned low = g >= 2 ? 2u : 1u, run = low == 2 ? B * B : B, c = (B - 1) / 2;
    const size_t runs = entries / run;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < ng * runs; id += (size_t)gridDim.x * blockDim.x) {
        const size_t bi = id / runs, grp = g0 + bi, i0 = grp * g;
        uint32_t t = (uint32_t)(id - bi * runs);
        G1Xyzz* out = tmp + (bi << hb) + (size_t)t * run;
        G1Xyzz acc = g1_xyzz_identity();
#pragma unroll 1
        for (unsigned pos = low; pos < g; pos++) {
            const int code = (int)(t % B) - (int)c;
            t /= B;
            const G1Affine q = msm_comb_top_point(tq, n, i0 + pos, code < 0);
#pragma unroll 1
            for (int k = 0; k < (code < 0 ? -code : code); k++) g1_madd<true>(acc, q);
        }
        const G1Affine q0 = msm_comb_top_point(tq, n, i0, false), m0 = msm_comb_top_point(tq, n, i0, true);
        const G1Affine q1 = msm_comb_top_point(tq, n, low == 2 ? i0 + 1 : n, false), m1 = msm_comb_top_point(tq, n, low == 2 ? i0 + 1 : n, true);
#pragma unroll 1
        for (unsigned k = 0; k < c; k++) {
            g1_madd<true>(acc, m0);
            g1_madd<true>(acc, m1);
        }
#pragma unroll 1
        for (unsigned d1 = 0; d1 < (low == 2 ? B : 1u); d1++) {
            const bool down = (d1 & 1u) != 0;
#pragma unroll 1
            for (unsigned st = 0; st < B; st++) {
                out[d1 * B + (down ? B - 1 - st : st)] = acc;
                if (st + 1 < B) g1_madd<true>(acc, down ? m0 : q0);
            }
            if (d1 + 1 < B) g1_madd<true>(acc, q1);
        }
    }
}

// skip[i] = 1 where base i is the identity (MsmLookupTable::base_skip): every entry of its block is the identity.  No other entry of
// a base's block is: E_P[idx] = c R^-1 P with c odd and |c| < 2^(a (h-1) + 1) < r.
__global__ void msm_comb_base_skip_kernel(const G1Affine* bases, size_t n, uint8_t* skip) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        G1Affine b;
        b.x = fp_load(&bases[i].x);
        b.y = fp_load(&bases[i].y);
        skip[i] = g1_affine_is_identity(b) ? 1 : 0;
    }
}

// digits[(m * A + j) * nd + i] = column j of scalar i of MSM m: the index of its table entry in bits 0 .. H-2, bit 31 set when the
// entry is to be subtracted.  Scalar vector of MSM m: msm_scalar_row.  nd = n without top
// tables.  TOP (see msm_comb_shape): a workgroup takes PER = g floor(256 / g) scalars — whole groups — and, after the columns,
// lane t < PER / g folds the top codes of its group into the digit of virtual scalar n + grp / A of column grp % A
// (nd = n + ceil(ceil(n / g) / A); a group past the last scalar gets the all-zero code: the identity entry of its block).
// Items whose entry is the identity get MSM_COMB_SKIP: every column of an identity base (base_skip), and a group whose codes are all
// zero — an identity base's code counts as zero, its share of every joint entry being the identity.  The kernel also zeroes
// n_deferred[m] and the counter of the recovery list (redo[0]): it runs before the kernels that count.
// Layout: the digit of (row = m A + j, item i) is digits[row * rs + i * is].  Column-major (rs, is) = (nd, 1) is what msm_comb_kernel
// reads; item-major (1, R), R = M A rows, is the row walk's (msm_comb_rows_kernel): there a lane's A digits lie next to each other
// and, where A is a multiple of four (every row then starts on 16 bytes), leave as 16-byte stores.
// tsh: a workgroup takes 2^tsh MSMs (up to m_end) and 256 >> tsh scalars of each (whole groups), the MSM in the low bits of the lane
// number.  0 for the column-major layout (a grid row per MSM); 2 for the item-major one, where the digits of one scalar in four
// consecutive MSMs are 4 A consecutive words: lanes that wrote A words each, 4 R bytes apart, left every line partly written
// (the kernel took twice its time).
template <unsigned H, bool TOP> __global__ void __launch_bounds__(256) msm_comb_digits_kernel(const Fr* scalars, size_t n, size_t stride, size_t inner,
                                                                                              size_t outer_stride, size_t m0, size_t m_end, unsigned tsh,
                                                                                              uint32_t* digits, size_t nd, size_t rs, size_t is,
                                                                                              const uint8_t* base_skip, uint32_t* n_deferred, uint32_t* redo) {
    PLONK_SHORT_KERNEL();
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) redo[0] = 0;  // the recovery list's counter (its own part of the scratch: msm_redo_words)
    constexpr MsmCombShape SH = msm_comb_shape(H, TOP);
    constexpr unsigned A = SH.a, L = A * H;
    static_assert(L <= 9 * 32 && H <= MSM_COMB_MAX_TEETH, "the recoded scalar is kept in nine words");
    constexpr unsigned GRP = TOP && SH.top_g ? SH.top_g : 1;
    const unsigned span = 256u >> tsh, per = (span / GRP) * GRP;  // scalars per MSM of the workgroup: whole groups
    const unsigned ml = threadIdx.x & ((1u << tsh) - 1u), il = threadIdx.x >> tsh;
    const size_t m = m0 + ((size_t)blockIdx.y << tsh) + ml, i = (size_t)blockIdx.x * per + il;  // (no division per lane)
    const bool live = il < per && i < n && m < m_end;
    if (blockIdx.x == 0 && il == 0 && m < m_end) n_deferred[m] = 0;
    int code = 0;
    if (live) {
        const bool skip = base_skip[i] != 0;
        const Fr* sc = msm_scalar_row(scalars, m, stride, inner, outer_stride);
        const Fr s = fp_load(sc + i);  // the Montgomery residue s R mod r, taken as the integer it is: the table holds multiples of R^-1 P
        // odd representative: s, or r - s with the sign of the base flipped (r is odd; s = 0 becomes r, and r P = O comes out of the sums)
        const bool even = !(s.v[0] & 1u);
        uint32_t sp[8], br = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t d = fp_sbb(FrParams::mod(k), s.v[k], br);
            sp[k] = even ? d : s.v[k];
        }
        // t = (v + 2^L - 1) / 2 = (v >> 1) + 2^(L-1), v = s' (mod 2^L when the top tables take the rest): bit p of t is 1 where the
        // digit of 2^p is +1
        uint32_t w[9];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = (sp[k] >> 1) | (k < 7 ? sp[k + 1] << 31 : 0u);
        w[8] = 0;
        if constexpr (TOP) {
            constexpr unsigned hi = L >> 5, sh = L & 31;  // u = bits L .. 253 of s'
            uint32_t u = sp[hi] >> sh;
            if constexpr (sh + SH.top_bits > 32 && hi + 1 < 8) u |= sp[hi + 1] << (32 - sh);
            code = (int)(u & ((1u << SH.top_bits) - 1u));
            if (even) code = -code;
            if (skip) code = 0;
#pragma unroll
            for (unsigned k = 0; k < 9; k++) {  // v >> 1 keeps bits 0 .. L-2
                if (k > ((L - 1) >> 5)) w[k] = 0;
                else if (k == ((L - 1) >> 5)) w[k] &= (1u << ((L - 1) & 31)) - 1u;
            }
        }
        w[(L - 1) >> 5] |= 1u << ((L - 1) & 31);
        uint32_t* out = digits + (m * A) * rs + i * is;
        constexpr bool VEC = A % 4 == 0 && A <= 32;  // (more columns than that: a toy comb, word stores)
        const bool vec = VEC && tsh != 0;  // (the launcher gives tsh != 0 to the item-major layout alone)
        uint32_t dv[VEC ? A : 1];
        // Column j's index is the bits j + A k of t.  Shifted right by (A - 1) k + c0, tooth k's bits of the C columns from c0 on sit at
        // k + (j - c0): one shift per tooth and chunk of columns, and the teeth k, k + C, .. land in disjoint windows [k, k + C) that
        // are merged before the columns take their bits — diag[j - c0] = idx_j << (j - c0), from one AND-OR per column and C teeth.
        // C: as many columns as keep the H + C - 1 bits of a diagonal inside a word.  (Below six teeth a column has too few bits for
        // the shared shifts to pay: those combs gather bit by bit.)
        const auto emit = [&](unsigned j, uint32_t idx) PLONK_LAMBDA_INLINE {
            const uint32_t top = idx >> (H - 1), mask = (1u << (H - 1)) - 1u;
            const uint32_t low = top ? (idx & mask) : (~idx & mask);  // top tooth -1: minus the entry of the complemented teeth
            const uint32_t neg = (top ? 0u : 1u) ^ (even ? 1u : 0u);
            const uint32_t d = low | (neg << 31);
            if constexpr (VEC) {
                if (vec) {
                    dv[j] = skip ? MSM_COMB_SKIP : d;
                    return;
                }
            }
            out[(size_t)j * rs] = d;
        };
        if constexpr (H < 6) {
#pragma unroll
            for (unsigned j = 0; j < A; j++) {
                uint32_t idx = 0;
#pragma unroll
                for (unsigned k = 0; k < H; k++) {
                    const unsigned p = j + A * k;
                    idx |= ((w[p >> 5] >> (p & 31)) & 1u) << k;
                }
                emit(j, idx);
            }
        } else {
            constexpr unsigned C = A < 33 - H ? A : 33 - H;
#pragma unroll
            for (unsigned c0 = 0; c0 < A; c0 += C) {
                uint32_t diag[C] = {};
#pragma unroll
                for (unsigned k0 = 0; k0 < C && k0 < H; k0++) {
                    uint32_t v = 0, teeth = 0;
#pragma unroll
                    for (unsigned k = k0; k < H; k += C) {
                        const unsigned s = (A - 1) * k + c0, q = s >> 5, sh = s & 31;
                        const uint32_t win = sh ? (w[q] >> sh) | (q + 1 < 9 ? w[q + 1] << (32 - sh) : 0u) : w[q];
                        v |= win & (((1u << C) - 1u) << k);
                        teeth |= 1u << k;
                    }
#pragma unroll
                    for (unsigned j = 0; j < C; j++) diag[j] |= v & (teeth << j);
                }
#pragma unroll
                for (unsigned j = c0; j < c0 + C && j < A; j++) emit(j, diag[j - c0] >> (j - c0));
            }
        }
        if constexpr (VEC) {
            if (vec) {
#pragma unroll
                for (unsigned j = 0; j < A; j += 4) *reinterpret_cast<MsmCombDigit4*>(out + j) = MsmCombDigit4{{dv[j], dv[j + 1], dv[j + 2], dv[j + 3]}};
            }
        }
        if (skip && !vec) {  // (written over afterwards, by the lanes concerned alone: nothing per column for the others)
#pragma unroll 1
            for (unsigned j = 0; j < A; j++) out[(size_t)j * rs] = MSM_COMB_SKIP;
        }
    }
    if constexpr (TOP) {
        constexpr unsigned G = SH.top_g, B = SH.top_b;
        __shared__ int codes[256];
        codes[ml * span + il] = code;  // (the codes of one MSM side by side)
        __syncthreads();
        const size_t grp = (size_t)blockIdx.x * (per / G) + il, nv = msm_comb_virtual(n, SH);
        if (il < per / G && grp < nv * A && m < m_end) {
            uint32_t idx = 0, pw = 1;
#pragma unroll
            for (unsigned pos = 0; pos < G; pos++) {
                idx += (uint32_t)(codes[ml * span + il * G + pos] + (int)((B - 1) / 2)) * pw;
                pw *= B;
            }
            const size_t v = grp / A, j = grp - v * A;
            digits[(m * A + j) * rs + (n + v) * is] = idx == (SH.top_entries - 1) / 2 ? MSM_COMB_SKIP : (uint32_t)((v * (A - 1) + j) << (H - 1)) + idx;  // (B^g - 1) / 2: every code zero
        }
    }
}

// Partition of a workgroup's nsub scalars x a columns over its MSM_BLOCK lanes (see the header): q lanes per column take p scalars
// each out of the first n_main; the other lanes share the a * n_left items left, in column-major order.
struct MsmCombPlan {
    uint32_t q, p, n_main, n_left;
};
PLONK_HD MsmCombPlan msm_comb_plan(uint32_t nsub, uint32_t a) {
    MsmCombPlan pl;
    pl.q = MSM_BLOCK / a;
    pl.p = (a * nsub + MSM_BLOCK - 1) / MSM_BLOCK;
    const uint32_t reach = pl.q * pl.p;
    pl.n_main = reach < nsub ? reach : nsub;
    pl.n_left = nsub - pl.n_main;
    return pl;
}
// pieces of column j left by the left-over lanes: lanes ulo .. ulo + x - 1
PLONK_HD void msm_comb_left_pieces(const MsmCombPlan& pl, uint32_t j, uint32_t& ulo, uint32_t& x) {
    if (!pl.n_left) {
        ulo = 0;
        x = 0;
        return;
    }
    ulo = (j * pl.n_left) / pl.p;
    x = ((j + 1) * pl.n_left - 1) / pl.p - ulo + 1;
}
// LDS slot of piece r of column j: the q column lanes first, then the left-over lanes' pieces (lane u, column j: slot a q + u + j —
// lanes and the columns they touch are both monotone, so the slot is unique)
PLONK_HD uint32_t msm_comb_slot(const MsmCombPlan& pl, uint32_t a, uint32_t j, uint32_t r, uint32_t ulo) {
    return r < pl.q ? j * pl.q + r : a * pl.q + ulo + j + (r - pl.q);
}

// NARROW: the table has at most 2^32 entries (decided per launch on the host), so an entry's index is formed in one 32-bit register
// and scaled once; the wide form is for larger tables.
template <bool NARROW>
__global__ void __launch_bounds__(MSM_BLOCK, MSM_ACC_WAVES) msm_comb_kernel(const G1Affine* lookup, unsigned hb, unsigned a,
                                                                             const uint32_t* digits, size_t n, unsigned G,
                                                                             G1Xyzz* partial, MsmDeferred* deferred, size_t deferred_stride,
                                                                             uint32_t* n_deferred, unsigned n_real, unsigned top_delta) {
    // (n counts the virtual scalars of a comb with top tables, n_real the real ones: block of scalar i = msm_comb_block_of)
    PLONK_DYN_SMEM(smem);  // (MSM_BLOCK + a) pieces of 128 B
    G1Xyzz* red = reinterpret_cast<G1Xyzz*>(smem);
    const unsigned m = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
    const uint32_t per_g = (uint32_t)((n + G - 1) / G);
    const uint32_t s0 = g * per_g < n ? g * per_g : (uint32_t)n, s1 = s0 + per_g < n ? s0 + per_g : (uint32_t)n, nsub = s1 - s0;
    const MsmCombPlan pl = msm_comb_plan(nsub, a);
    const uint32_t* dg = digits + (size_t)m * a * n + s0;  // dg[j * n + i], i relative to s0
    const G1Affine* tab = lookup + ((size_t)s0 << hb);
    const uint32_t nr_rel = n_real > s0 ? n_real - s0 : 0u;  // first virtual scalar, relative to s0
    uint32_t j, i, step, count, slot;
    const bool column_lane = tid < a * pl.q;
    if (column_lane) {
        j = tid / pl.q;
        i = tid - j * pl.q;
        step = pl.q;
        count = i < pl.n_main ? (pl.n_main - 1 - i) / pl.q + 1 : 0;
        slot = tid;
    } else {
        const uint32_t u = tid - a * pl.q, items = a * pl.n_left;
        const uint32_t lo = u * pl.p < items ? u * pl.p : items, hi = lo + pl.p < items ? lo + pl.p : items;
        count = hi - lo;
        j = pl.n_left ? lo / pl.n_left : 0;
        i = pl.n_main + (lo - j * pl.n_left);
        step = 1;
        slot = a * pl.q + u + j;
    }
    G1XyzzL run = g1l_identity();
    auto flush = [&]() { red[slot] = g1l_to_piece(run); };  // [0, 4m) words: what g1l_from_piece takes
    const uint32_t* col = dg + (size_t)j * n;  // the digits of the lane's column
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t d = col[i];
        if (d != MSM_COMB_SKIP) {  // (an identity entry is known by its digit: no test of the entry itself)
            const bool is_virtual = i >= nr_rel;
            const uint32_t blk = i + (is_virtual ? top_delta : 0u), e = d & 0x7fffffffu;
            const G1Affine* src;
            if constexpr (NARROW) src = tab + ((blk << hb) + e);
            else src = tab + (((size_t)blk << hb) + e);
            const Fq x = fp_load(&src->x), y = fp_load(&src->y);
            // a JOINT entry can still be the identity under non-zero codes when the group's bases are related (a duplicated base with
            // opposite codes): the virtual scalars, one item in a g + 1, keep the test of the entry
            bool add = true;
            if (is_virtual) add = !(fp_is_zero(x) && fp_is_zero(y));
            if (add && !g1l_madd_signed(run, x, y, (uint32_t)((int32_t)d >> 31))) {  // equal or opposite: see msm_accumulate_kernel
                const uint32_t sl = atomicAdd(n_deferred + m, 1u);
                if (sl < MSM_DEFER_CAP) deferred[(size_t)m * deferred_stride + sl] = MsmDeferred{(uint32_t)(j * n + s0 + i), d};
            }
        }
        i += step;
        if (i >= nsub && k + 1 < count) {  // a left-over lane moves on to the next column
            flush();
            run = g1l_identity();
            slot++;
            j++;
            col += n;
            i = pl.n_main;
        }
    }
    if (column_lane || count) flush();
    __syncthreads();
    // Per-column tree over the pieces: level by level the upper half of every column's list is added onto its lower half.
    // Lists differ in length by at most the left-over pieces (<= 2 + 1); `cur` walks the longest one.
    uint32_t cur = pl.q + (pl.n_left ? (pl.n_left + pl.p - 1) / pl.p + 1 : 0);
    while (cur > 1) {
        const uint32_t half = (cur + 1) / 2, cnt = cur - half;
        for (uint32_t w = tid; w < a * cnt; w += MSM_BLOCK) {
            const uint32_t jj = w / cnt, r = w - jj * cnt;
            uint32_t ulo, x;
            msm_comb_left_pieces(pl, jj, ulo, x);
            if (r + half < pl.q + x) {
                const uint32_t sa = msm_comb_slot(pl, a, jj, r, ulo), sb = msm_comb_slot(pl, a, jj, r + half, ulo);
                const G1XyzzL o = g1l_from_piece(&red[sb]);
                if (!o.inf) {
                    G1XyzzL v = g1l_from_piece(&red[sa]);
                    if (!g1l_add_fast(v, o)) atomicOr(n_deferred + m, MSM_COMB_REDO);  // equal or opposite sums: msm_comb_slow_kernel
                    red[sa] = g1l_to_piece_wide(v);
                }
            }
        }
        __syncthreads();
        cur = half;
    }
    if (tid < a) partial[((size_t)m * G + g) * a + tid] = red[tid * pl.q];
}

// The ROW WALK: the same accumulation with lanes bound to ROWS — row = m a + j, one (MSM, column) pair, R = M a of them in a
// launch — where msm_comb_kernel binds q lanes to a column of ONE MSM.  A workgroup takes MSM_BLOCK consecutive rows (they need not
// be whole MSMs; rows from R up do nothing) and one chunk [i0, i1) of the n scalars, chunk c = blockIdx.x / W of G chunks of
// ceil(n / G) scalars (the last ones may be short or empty), W = ceil(R / MSM_BLOCK).  At step i every lane adds its row's entry of
// scalar i: the block msm_comb_block_of(i) and is_virtual are wave-uniform, so all lanes of a workgroup — and all workgroups of a
// chunk — read ONE base's block of 2^(h-1) entries per step (G blocks on the chip at a time, against q per workgroup and phase of
// msm_comb_kernel: address-translation reach).  digits: item-major, digits[i R + row] — a wave's load is 256 contiguous bytes.
// A lane's sum IS its row's share of the chunk: no LDS, no barrier, no tree, no left-over lanes; it is stored chunk-major,
// partial[c R + row], and msm_comb_rowsum_kernel adds the G chunks of a row.
template <bool NARROW>
__global__ void __launch_bounds__(MSM_BLOCK, MSM_ACC_WAVES) msm_comb_rows_kernel(const G1Affine* lookup, unsigned hb, unsigned a, const uint32_t* digits,
                                                                                  unsigned n, unsigned R, unsigned W, unsigned G, G1Xyzz* partial,
                                                                                  MsmDeferred* deferred, size_t deferred_stride, uint32_t* n_deferred,
                                                                                  unsigned n_real, unsigned top_delta) {
    const unsigned c = blockIdx.x / W, row = (blockIdx.x - c * W) * MSM_BLOCK + threadIdx.x;
    if (row >= R) return;
    const unsigned per = (n + G - 1) / G;
    const unsigned i0 = c * per < n ? c * per : n, i1 = i0 + per < n ? i0 + per : n;
    const unsigned m = row / a, j = row - m * a;
    const uint32_t* dg = digits + row;
    G1XyzzL run = g1l_identity();
    if (i0 < i1) {
        // Two steps deep: the entry of step i + 1 and the digit of step i + 2 are requested before the addition of step i, so both
        // latencies pass under its ~2 100 instructions.  (The workgroups of a round of the chip's slots start together and run in lock
        // step: without this the four waves of a SIMD wait for their entries together — VALU busy 0.86 with no translation miss
        // left.  The kernel has the registers for it: 86 without the second entry.)  A skipped item requests entry 0 of its block
        // and the steps past the chunk's end request the last item again: valid addresses, no branch around the loads.
        const unsigned last = i1 - 1;
        const auto entry = [&](unsigned i, uint32_t d) PLONK_LAMBDA_INLINE {
            const uint32_t blk = i + (i >= n_real ? top_delta : 0u), e = d == MSM_COMB_SKIP ? 0u : d & 0x7fffffffu;
            if constexpr (NARROW) return lookup + ((blk << hb) + e);
            else return lookup + (((size_t)blk << hb) + e);
        };
        uint32_t d = dg[(size_t)i0 * R], dn = dg[(size_t)(i0 < last ? i0 + 1 : last) * R];
        const G1Affine* src = entry(i0, d);
        Fq x = fp_load(&src->x), y = fp_load(&src->y);
        for (unsigned i = i0; i < i1; i++) {
            const unsigned in = i < last ? i + 1 : last, in2 = i + 2 < last ? i + 2 : last;
            const uint32_t dn2 = dg[(size_t)in2 * R];
            const G1Affine* sn = entry(in, dn);
            const Fq xn = fp_load(&sn->x), yn = fp_load(&sn->y);
            if (d != MSM_COMB_SKIP) {  // (an identity entry is known by its digit: no test of the entry itself)
                bool add = true;  // (a joint entry can be the identity under non-zero codes: msm_comb_kernel)
                if (i >= n_real) add = !(fp_is_zero(x) && fp_is_zero(y));
                if (add && !g1l_madd_signed(run, x, y, (uint32_t)((int32_t)d >> 31))) {  // equal or opposite: see msm_accumulate_kernel
                    const uint32_t sl = atomicAdd(n_deferred + m, 1u);
                    if (sl < MSM_DEFER_CAP) deferred[(size_t)m * deferred_stride + sl] = MsmDeferred{(uint32_t)(j * n + i), d};
                }
            }
            d = dn;
            dn = dn2;
            x = xn;
            y = yn;
        }
    }
    partial[(size_t)c * R + row] = g1l_to_piece(run);
}

// colsum[row] = sum_c partial[c R + row], the G chunks of the row walk.  MSM_ROWSUM_LANES = 4 lanes per row take the chunks c = l
// (mod 4) serially and two butterfly steps join them: 4 (ceil(G / 4) + 2) general additions per row where a wave per row
// (msm_comb_colsum_kernel) spends 64 x 7 — 3.9 % of the accumulation's VALU instructions at the rule's G = 42 and 64 (1.8 % at G = 14),
// against a quarter.  ONE lane per row would be the least work (G additions), but its chain of G serial additions in R / 64 waves took
// 157 us per launch of 1 152 MSMs at G = 14 and a twelfth of the chip's issue slots, on a queue whose next kernel waits for it.  The layout is what msm_comb_finalize_kernel
// reads with G = 1.
#define MSM_ROWSUM_LANES 4
__global__ void PLONK_BESIDE_ACC(64, 2) msm_comb_rowsum_kernel(const G1Xyzz* partial, unsigned G, unsigned R, unsigned a, G1Xyzz* colsum, uint32_t* n_deferred) {
    PLONK_SHORT_KERNEL();
    const unsigned lane = threadIdx.x, row = blockIdx.x * (64 / MSM_ROWSUM_LANES) + lane / MSM_ROWSUM_LANES, l = lane % MSM_ROWSUM_LANES;
    G1XyzzL acc = g1l_identity();  // (a lane past the last row keeps the identity: every lane takes part in the exchanges)
    bool ok = true;
    if (row < R) {
#pragma unroll 1
        for (unsigned c = l; c < G; c += MSM_ROWSUM_LANES) ok &= g1l_add_fast(acc, g1l_from_piece(&partial[(size_t)c * R + row]));
    }
    ok &= g1l_wave_reduce_step<1>(acc, lane);
    ok &= g1l_wave_reduce_step<2>(acc, lane);
    if (!ok && row < R) atomicOr(n_deferred + row / a, MSM_COMB_REDO);  // equal or opposite operands somewhere: msm_comb_slow_kernel
    if (l == 0 && row < R) colsum[row] = g1l_to_piece_wide(acc);
}

// colsum[m * a + j] = sum_g partial[(m * G + g) * a + j]: a wave per (MSM, column), lane g (G <= 64)
__global__ void __launch_bounds__(64) msm_comb_colsum_kernel(const G1Xyzz* partial, unsigned G, unsigned a, G1Xyzz* colsum, uint32_t* n_deferred) {
    PLONK_SHORT_KERNEL();
    const size_t m = blockIdx.x / a, j = blockIdx.x % a;
    const unsigned lane = threadIdx.x;
    G1XyzzL acc = g1l_identity();
    bool ok = true;
    for (unsigned g = lane; g < G; g += 64) ok &= g1l_add_fast(acc, g1l_from_piece(&partial[(m * G + g) * a + j]));
    ok &= g1l_wave_reduce_step<32>(acc, lane);
    ok &= g1l_wave_reduce_step<16>(acc, lane);
    ok &= g1l_wave_reduce_step<8>(acc, lane);
    ok &= g1l_wave_reduce_step<4>(acc, lane);
    ok &= g1l_wave_reduce_step<2>(acc, lane);
    ok &= g1l_wave_reduce_step<1>(acc, lane);
    if (!ok) atomicOr(n_deferred + m, MSM_COMB_REDO);  // equal or opposite operands somewhere: msm_comb_slow_kernel
    if (lane == 0) colsum[m * a + j] = g1l_to_piece_wide(acc);
}

// sum_j 2^j S_j for MSM m, S_j = sum_g sums[(m G + g) a + j] + the deferred additions of column j.  LPM lanes per MSM: lane l
// takes the columns j = l (mod LPM) by Horner from the top (LPM doublings between two of them), doubles its share l more times,
// and the LPM shares are summed by the cross-lane butterfly.  LPM = 1 is the plain Horner chain, one MSM per lane (least work:
// a batch); larger groups shorten the chain of a - 1 serial doublings at the price of idle lanes (few MSMs: latency).
template <unsigned LPM> __global__ void PLONK_BESIDE_ACC(64, 1) msm_comb_finalize_kernel(const G1Xyzz* sums, size_t M, unsigned G, unsigned a,
                                                                                       const G1Affine* lookup, unsigned hb, size_t n,
                                                                                       const MsmDeferred* deferred, size_t deferred_stride,
                                                                                       uint32_t* n_deferred, uint32_t* redo, Fq* out_xy, uint8_t* flags,
                                                                                       unsigned n_real, unsigned top_delta) {
    PLONK_SHORT_KERNEL();
    const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x, m = gid / LPM;
    const unsigned l = (unsigned)(gid % LPM), lane = threadIdx.x;
    G1XyzzL acc = g1l_identity();
    bool ok = true;  // false: an addition met equal or opposite operands — the MSM goes to msm_comb_slow_kernel
    bool listed = false;  // lane 0 of the MSM: the kernels before this one left it to be redone
    if (m < M && l < a) {
        const uint32_t seen = n_deferred[m];
        listed = l == 0 && msm_comb_needs_redo(seen);
        const uint32_t nd = msm_comb_needs_redo(seen) ? 0u : seen;  // (an MSM to be redone: its list may have holes, its sum is overwritten)
        const unsigned jtop = l + ((a - 1 - l) / LPM) * LPM;
#pragma unroll 1
        for (int j = (int)jtop; j >= 0; j -= (int)LPM) {
            if (j != (int)jtop)
#pragma unroll 1
                for (unsigned d = 0; d < LPM; d++) g1l_dbl(acc);
#pragma unroll 1
            for (unsigned g = 0; g < G; g++) ok &= g1l_add_fast<true>(acc, g1l_from_piece(&sums[(m * G + g) * a + j]));  // (<true>: opposite operands give the identity)
#pragma unroll 1
            for (uint32_t k = 0; k < nd; k++) {
                const MsmDeferred e = deferred[m * deferred_stride + k];  // `bucket` carries the item j * n + i here
                if (e.bucket / n != (uint32_t)j || e.entry == MSM_COMB_SKIP) continue;  // (the comb kernel defers no skipped item)
                const size_t i = e.bucket - (size_t)j * n;
                const G1Affine* src = lookup + ((msm_comb_block_of(i, n_real, top_delta) << hb) + (e.entry & 0x7fffffffu));
                // deferred for being exceptional against its LANE's sum at the time; against the column's sum it normally is not
                const Fq x = fp_load(&src->x), y = fp_load(&src->y);
                if (!(fp_is_zero(x) && fp_is_zero(y))) ok &= g1l_madd_fast(acc, x, y, (e.entry >> 31) != 0);
            }
        }
#pragma unroll 1
        for (unsigned d = 0; d < l; d++) g1l_dbl(acc);
    }
    if constexpr (LPM >= 2) ok &= g1l_wave_reduce_step<1, true>(acc, lane);
    if constexpr (LPM >= 4) ok &= g1l_wave_reduce_step<2, true>(acc, lane);
    if constexpr (LPM >= 8) ok &= g1l_wave_reduce_step<4, true>(acc, lane);
    if constexpr (LPM >= 16) ok &= g1l_wave_reduce_step<8, true>(acc, lane);
    if constexpr (LPM >= 32) ok &= g1l_wave_reduce_step<16, true>(acc, lane);
    if constexpr (LPM >= 64) ok &= g1l_wave_reduce_step<32, true>(acc, lane);
    // The recovery list takes every MSM to be redone ONCE.  One flagged before this kernel (the accumulation's count past the cap, the
    // tree's or the row sum's flag): its lane 0, and every atomicOr below then returns a value that already says "redo".  One whose
    // first failed addition is here: the lane whose atomicOr returns a value that does not — the flag is never cleared, so one lane.
    if (m < M && !ok && !msm_comb_needs_redo(atomicOr(n_deferred + m, MSM_COMB_REDO))) listed = true;
    if (listed) msm_redo_append(redo, (uint32_t)m, (uint32_t)M);
    if (m < M && l == 0) msm_store_result(g1l_to_xyzz(acc), m, out_xy, flags);
}

// Recovery path (MSM_DEFER_CAP, MSM_COMB_REDO): every MSM of the recovery list recomputed from its digits with the general formulas.
// A fixed grid of at most MSM_SLOW_GRID workgroups strides over the list, a workgroup per listed MSM at a time; with an empty
// list — the normal case — every workgroup reads the counter and returns.  Lane t: Horner over the columns of the scalars t, t + 256, ..
// (rs, is): the digits' row and item strides (msm_comb_digits_kernel).  M bounds the list (the counter cannot pass it: an MSM is
// appended once).
__global__ void PLONK_BESIDE_ACC(256, 32) msm_comb_slow_kernel(const G1Affine* lookup, unsigned hb, unsigned a, const uint32_t* digits, size_t n, size_t rs,
                                                            size_t is, const uint32_t* redo, unsigned M, Fq* out_xy, uint8_t* flags, unsigned n_real,
                                                            unsigned top_delta) {
    PLONK_SHORT_KERNEL();
    __shared__ G1Xyzz red[256];
    const unsigned tid = threadIdx.x, count = redo[0] < M ? redo[0] : M;
#pragma unroll 1
    for (unsigned k = blockIdx.x; k < count; k += gridDim.x) {  // (count is the same in every lane: the barriers below are reached by all)
        const unsigned m = redo[1 + k];
        if (m >= M) continue;  // (never: finalize appends indices below M; the same in every lane)
        const uint32_t* dg = digits + (size_t)m * a * rs;
        G1Xyzz acc = g1_xyzz_identity();
#pragma unroll 1
        for (int j = (int)a - 1; j >= 0; j--) {
            g1_dbl(acc);
#pragma unroll 1
            for (size_t i = tid; i < n; i += 256) {
                const uint32_t d = dg[(size_t)j * rs + i * is];
                if (d == MSM_COMB_SKIP) continue;
                const G1Affine* src = lookup + ((msm_comb_block_of(i, n_real, top_delta) << hb) + (d & 0x7fffffffu));
                G1Affine pt;
                pt.x = fp_load(&src->x);
                pt.y = fp_load(&src->y);
                if (d >> 31) pt.y = fp_neg(pt.y);
                g1_madd<false>(acc, pt);  // the rare branch inline: the out-of-line g1_madd_equal_x alone holds 97 VGPRs, one more than fit
            }
        }
        msm_fold_store(red, acc, tid, 256, m, out_xy, flags);
        __syncthreads();  // red is written again for the workgroup's next MSM
    }
}

// Verification of a comb table found in the registry by its 64-bit key (msm_tables.h, lut_verified), against THIS SRS's bases:
//   every base: the all-ones entry = (sum_k 2^(a k)) R^-1 P_i, recomputed by doublings and additions from the base;
//   LUT_VERIFY_SAMPLES bases: entry 0 (every lower tooth -1) and the entry of the alternating index 0101.. as well.
// A table of another tooth count / spacing, or of other bases, filed under the same key fails here.
PLONK_DEV bool msm_comb_entry_matches(const G1Affine& P0, const MsmCombScale& k, unsigned a, unsigned h, uint32_t idx, const G1Affine* e) {
    const G1Affine P = g1_to_affine(msm_comb_scaled_base(P0, k));
    const G1Xyzz v = msm_comb_entry_slow(P, a, h, idx);
    const Fq ex = fp_load(&e->x), ey = fp_load(&e->y);
    if (g1_is_identity(v)) return fp_is_zero(ex) && fp_is_zero(ey);
    return fp_eq(fp_mul(ex, v.zz), v.x) && fp_eq(fp_mul(ey, v.zzz), v.y);
}
__global__ void __launch_bounds__(64) msm_comb_verify_kernel(const G1Affine* bases, const G1Affine* lookup, size_t n, unsigned a, unsigned h,
                                                             unsigned samples, MsmCombScale k, unsigned* mismatches) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n + 2 * (size_t)samples) return;
    const uint32_t mask = (1u << (h - 1)) - 1u;
    size_t i;
    uint32_t idx;
    if (t < n) {
        i = t;
        idx = mask;
    } else {
        const unsigned s = (unsigned)(t - n) >> 1;
        i = n <= samples ? (s < n ? s : n - 1) : (size_t)s * (n - 1) / (samples - 1);
        idx = ((t - n) & 1) ? (0x55555555u & mask) : 0u;
    }
    G1Affine b;
    b.x = fp_load(&bases[i].x);
    b.y = fp_load(&bases[i].y);
    if (!msm_comb_entry_matches(b, k, a, h, idx, lookup + ((i << (h - 1)) + idx))) atomicAdd(mismatches, 1u);
}

// ... and of its top tables: for every group the entry whose codes are all +1 = sum_pos 2^(L - j) R^-1 P_(g grp + pos), recomputed
// from this SRS's bases (a table of another tooth count, group size or base set fails here)
__global__ void __launch_bounds__(64) msm_comb_verify_top_kernel(const G1Affine* bases, const G1Affine* lookup, size_t n, unsigned a, unsigned h, unsigned g,
                                                                 unsigned B, MsmCombScale k, unsigned* mismatches) {
    const size_t grp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (grp >= msm_comb_top_groups(n, g)) return;
    const unsigned L = a * h, j = (unsigned)(grp % a);
    G1Xyzz sum = g1_xyzz_identity();
    uint32_t idx = 0, pw = 1;
#pragma unroll 1
    for (unsigned pos = 0; pos < g; pos++, pw *= B) {
        const size_t i = grp * g + pos;
        idx += ((B - 1) / 2 + (i < n ? 1u : 0u)) * pw;
        if (i >= n) continue;
        G1Affine b;
        b.x = fp_load(&bases[i].x);
        b.y = fp_load(&bases[i].y);
        G1Xyzz p = msm_comb_scaled_base(b, k);
#pragma unroll 1
        for (unsigned d = 0; d < L - j; d++) g1_dbl(p);
        g1_add(sum, p);
    }
    const G1Affine* e = lookup + (((n + grp) << (h - 1)) + idx);
    const Fq ex = fp_load(&e->x), ey = fp_load(&e->y);
    const bool ok = g1_is_identity(sum) ? (fp_is_zero(ex) && fp_is_zero(ey)) : (fp_eq(fp_mul(ex, sum.zz), sum.x) && fp_eq(fp_mul(ey, sum.zzz), sum.y));
    if (!ok) atomicAdd(mismatches, 1u);
}

// ---- host side ---------------------------------------------------------------------------------
// XYZZ staging of the build: an eighth of the table's entries at a time (whole bases), at most 2^27 of them (17 GB)
static size_t msm_comb_stage_entries(size_t n, unsigned h) {
    const size_t half = (size_t)1 << (h - 1);
    size_t bases = n / 8 ? n / 8 : 1;
    while (bases > 1 && bases * half > ((size_t)1 << 27)) bases /= 2;
    return bases * half;
}
static size_t msm_comb_bytes(size_t n, unsigned h, bool top) {  // table + staging
    return (msm_comb_blocks(n, msm_comb_shape(h, top)) << (h - 1)) * sizeof(G1Affine) + msm_comb_stage_entries(n, h) * sizeof(G1Xyzz);
}
static double msm_comb_additions(unsigned h, bool top) {
    const MsmCombShape sh = msm_comb_shape(h, top);
    return (double)sh.a + (top ? 1.0 / sh.top_g : 0.0);
}
bool msm_comb_takes_top(unsigned teeth) { return teeth >= 2 && teeth <= MSM_COMB_MAX_TEETH && msm_comb_top_ok(teeth); }
static bool msm_comb_takes_top_for(size_t n, unsigned h) { return msm_comb_top_ok(h) && msm_comb_top_reach_ok(n, msm_comb_shape(h, true)); }
static bool msm_comb_well_formed(const MsmLookupTable* t) {
    if (t->bits < 2 || t->bits > MSM_COMB_MAX_TEETH) return false;
    const bool top = t->top_g != 0;
    if (top && !msm_comb_top_ok(t->bits)) return false;
    const MsmCombShape sh = msm_comb_shape(t->bits, top);
    return t->base_skip && t->windows == sh.a && t->top_bits == sh.top_bits && t->top_g == sh.top_g &&
           t->bytes == (msm_comb_blocks(t->n_points, sh) << (t->bits - 1)) * sizeof(G1Affine);
}

// R^-1 mod r as a plain integer (R = 2^261, Fr's Montgomery radix): the comb tables hold multiples of R^-1 P_i
static MsmCombScale msm_comb_scale_constant() {
    Fr one_plain = fp_zero<FrParams>();
    one_plain.v[0] = 1;
    const Fr c = fp_from_mont(one_plain);  // fp_from_mont multiplies the integer it is given by R^-1 mod r: here the integer 1
    MsmCombScale k;
    for (int i = 0; i < 8; i++) k.c[i] = c.v[i];
    return k;
}

// Builds the comb table of h teeth; top: with top tables (floor(254 / h) columns, a joint table per group of bases for the bits left over)
static int msm_comb_build(plonk_ctx* ctx, const plonk_srs* srs, unsigned h, bool top, MsmLookupTable* t) {
    if (top && !msm_comb_top_ok(h)) {
        plonk_set_error("a comb of %u teeth takes no top tables (254 mod teeth must be 1 or 2)", h);
        return PLONK_ERR_ARG;
    }
    const MsmCombShape sh = msm_comb_shape(h, top);
    if (!msm_comb_top_reach_ok(srs->n_points, sh)) {
        plonk_set_error("%zu bases are too many for the top tables of a %u-tooth comb (a virtual scalar's block offset must fit 31 bits)", srs->n_points, h);
        return PLONK_ERR_ARG;
    }
    const unsigned a = sh.a, sb = h - 1 < MSM_COMB_SEG_BITS ? h - 1 : MSM_COMB_SEG_BITS;
    const size_t n = srs->n_points, half = (size_t)1 << (h - 1), stage = msm_comb_stage_entries(n, h), chunk_bases = stage / half;
    const size_t blocks = msm_comb_blocks(n, sh);
    void *gx = nullptr, *gb = nullptr, *dx = nullptr, *db = nullptr, *tmp = nullptr, *tab = nullptr, *pb = nullptr, *skip = nullptr;
    auto fail = [&]() {
        for (void* q : {gx, gb, dx, db, tmp, tab, pb, skip})
            if (q) hipFree(q);
        (void)hipGetLastError();
        plonk_set_error("the %u-tooth comb table (%zu MiB) does not fit in device memory", h, msm_comb_bytes(n, h, top) >> 20);
        return PLONK_ERR_NOMEM;
    };
    if (!plonk_dev_malloc(&tab, blocks * half * sizeof(G1Affine))) return fail();
    if (!plonk_dev_malloc(&tmp, stage * sizeof(G1Xyzz))) return fail();
    if (!plonk_dev_malloc(&gx, n * h * sizeof(G1Xyzz))) return fail();
    if (!plonk_dev_malloc(&gb, n * h * sizeof(G1Affine))) return fail();
    if (!plonk_dev_malloc(&dx, n * (sb ? sb : 1) * sizeof(G1Xyzz))) return fail();
    if (!plonk_dev_malloc(&db, n * (sb ? sb : 1) * sizeof(G1Affine))) return fail();
    if (!plonk_dev_malloc(&pb, n * sizeof(G1Affine))) return fail();
    if (!plonk_dev_malloc(&skip, n)) return fail();
    PLONK_LAUNCH(msm_comb_base_skip_kernel, grid1(n), dim3(256), 0, ctx->stream, (const G1Affine*)srs->bases, n, (uint8_t*)skip);
    // P'_i = R^-1 P_i (the scalars arrive as Montgomery residues), through the staging buffers of the next step
    PLONK_LAUNCH(msm_comb_scale_kernel, grid1(n, 64, 2048), dim3(64), 0, ctx->stream, (const G1Affine*)srs->bases, n, msm_comb_scale_constant(), (G1Xyzz*)gx);
    g1_batch_to_affine(ctx, (const G1Xyzz*)gx, (G1Affine*)pb, n);
    // tooth points G_k = 2^(a k) P'_i (k < h) and the Gray-code steps 2 G_k (k < sb), affine
    msm_window_bases(ctx, (const G1Affine*)pb, n, a, h, (G1Xyzz*)gx);
    g1_batch_to_affine(ctx, (const G1Xyzz*)gx, (G1Affine*)gb, n * h);
    if (sb) {
        PLONK_LAUNCH(msm_comb_delta_kernel, grid1(n * sb), dim3(256), 0, ctx->stream, (const G1Affine*)gb, n * sb, (G1Xyzz*)dx);
        g1_batch_to_affine(ctx, (const G1Xyzz*)dx, (G1Affine*)db, n * sb);
    }
    for (size_t i0 = 0; i0 < n; i0 += chunk_bases) {
        const size_t nb = n - i0 < chunk_bases ? n - i0 : chunk_bases, lanes = nb << (h - 1 - sb);
        PLONK_LAUNCH(msm_comb_fill_kernel, grid1(lanes, 64, 65536), dim3(64), 0, ctx->stream, (const G1Affine*)gb, (const G1Affine*)db, n, i0, nb, h, sb,
                     (G1Xyzz*)tmp);
        g1_batch_to_affine(ctx, (const G1Xyzz*)tmp, (G1Affine*)tab + i0 * half, nb * half);
    }
    if (top) {
        // tooth points of the top tables 2^(L - j) P'_i (through gx / gb, free by now), then the joint tables a chunk of groups at a
        // time; a block past the last group (the columns are padded to equal lengths) stays all identity
        PLONK_LAUNCH(msm_comb_top_base_kernel, grid1(n, 64, 2048), dim3(64), 0, ctx->stream, (const G1Affine*)pb, n, a * h, a, sh.top_g, (G1Xyzz*)gx);
        g1_batch_to_affine(ctx, (const G1Xyzz*)gx, (G1Affine*)gb, n);
        const size_t groups = msm_comb_top_groups(n, sh.top_g), vblocks = blocks - n, run = sh.top_g >= 2 ? (size_t)sh.top_b * sh.top_b : sh.top_b;
        for (size_t g0 = 0; g0 < vblocks; g0 += chunk_bases) {
            const size_t nb = vblocks - g0 < chunk_bases ? vblocks - g0 : chunk_bases;
            const size_t ng = g0 >= groups ? 0 : (groups - g0 < nb ? groups - g0 : nb);
            if (hipMemsetAsync(tmp, 0, nb * half * sizeof(G1Xyzz), ctx->stream) != hipSuccess) return fail();
            if (ng)
                PLONK_LAUNCH(msm_comb_top_fill_kernel, grid1(ng * (sh.top_entries / run), 64, 65536), dim3(64), 0, ctx->stream, (const G1Affine*)gb, n, g0, ng,
                             h - 1, sh.top_g, sh.top_b, sh.top_entries, (G1Xyzz*)tmp);
            g1_batch_to_affine(ctx, (const G1Xyzz*)tmp, (G1Affine*)tab + (n + g0) * half, nb * half);
        }
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return fail();
    for (void* q : {gx, gb, dx, db, tmp, pb}) hipFree(q);
    t->kind = MSM_TABLE_COMB;
    t->bits = h;
    t->windows = a;
    t->top_bits = sh.top_bits;
    t->top_g = sh.top_g;
    t->data = (G1Affine*)tab;
    t->base_skip = (uint8_t*)skip;
    t->bytes = blocks * half * sizeof(G1Affine);
    return PLONK_OK;
}

static void msm_comb_verify(plonk_ctx* ctx, const plonk_srs* srs, const MsmLookupTable* t, unsigned* d_mismatches) {
    const size_t lanes = srs->n_points + 2 * LUT_VERIFY_SAMPLES;
    PLONK_LAUNCH(msm_comb_verify_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, ctx->stream, (const G1Affine*)srs->bases,
                 (const G1Affine*)t->data, srs->n_points, t->windows, t->bits, (unsigned)LUT_VERIFY_SAMPLES, msm_comb_scale_constant(), d_mismatches);
    if (t->top_g) {
        const size_t groups = msm_comb_top_groups(srs->n_points, t->top_g);
        PLONK_LAUNCH(msm_comb_verify_top_kernel, dim3((unsigned)((groups + 63) / 64)), dim3(64), 0, ctx->stream, (const G1Affine*)srs->bases,
                     (const G1Affine*)t->data, srs->n_points, t->windows, t->bits, t->top_g, (2u << t->top_bits) - 1u, msm_comb_scale_constant(),
                     d_mismatches);
    }
}

// digits kernel of the comb with h teeth (one instantiation per tooth count: the bit gather is unrolled at compile time); TOP: the
// comb with top tables, whose workgroups take whole groups of scalars and add the virtual scalars' digits (nd = n + their number)
template <unsigned H, bool TOP> static void msm_comb_launch_digits(plonk_ctx* ctx, const Fr* d_scalars, size_t n, size_t stride, size_t inner,
                                                                   size_t outer_stride, size_t M, uint32_t* digits, size_t nd, bool item_major,
                                                                   const uint8_t* base_skip, uint32_t* n_deferred, uint32_t* redo) {
    if constexpr (!TOP || msm_comb_top_ok(H)) {
        constexpr MsmCombShape SH = msm_comb_shape(H, TOP);
        constexpr unsigned G = TOP ? SH.top_g : 1;
        const size_t rs = item_major ? 1 : nd, is = item_major ? M * SH.a : 1;  // column-major digits[row][i] / item-major digits[i][row]
        const unsigned tsh = item_major ? 2 : 0, PER = ((256u >> tsh) / G) * G;  // item-major: four MSMs per workgroup (the kernel's header)
        size_t gx = (n + PER - 1) / PER;
        if (TOP) {  // every virtual scalar's digit is written, also those of the groups past the last scalar
            const size_t gv = ((nd - n) * SH.a + PER / G - 1) / (PER / G);
            gx = gx > gv ? gx : gv;
        }
        void (*kern)(const Fr*, size_t, size_t, size_t, size_t, size_t, size_t, unsigned, uint32_t*, size_t, size_t, size_t, const uint8_t*, uint32_t*, uint32_t*) = msm_comb_digits_kernel<H, TOP>;  // (a template-id's comma would split the macro's arguments)
        for (size_t m0 = 0; m0 < M; m0 += (size_t)32768 << tsh) {  // (a grid's second dimension ends at 65 535)
            const size_t rows = M - m0 < ((size_t)32768 << tsh) ? M - m0 : (size_t)32768 << tsh;
            PLONK_LAUNCH(kern, dim3((unsigned)gx, (unsigned)((rows + (1u << tsh) - 1) >> tsh)), dim3(256), 0, ctx->stream, d_scalars, n, stride, inner,
                         outer_stride, m0, M, tsh, digits, nd, rs, is, base_skip, n_deferred, redo);
        }
    }
}
typedef void (*msm_comb_digits_fn)(plonk_ctx*, const Fr*, size_t, size_t, size_t, size_t, size_t, uint32_t*, size_t, bool, const uint8_t*, uint32_t*, uint32_t*);
template <bool TOP, unsigned... H> static msm_comb_digits_fn msm_comb_digits_for(unsigned h, std::integer_sequence<unsigned, H...>) {
    msm_comb_digits_fn fn = nullptr;
    ((h == H + 2 && (!TOP || msm_comb_top_ok(H + 2)) ? (void)(fn = &msm_comb_launch_digits<H + 2, TOP>) : (void)0), ...);
    return fn;
}

static int msm_run_comb(plonk_ctx* ctx, const plonk_srs* srs, const Fr* d_scalars, size_t n_real, size_t M, size_t stride, Fq* d_out_xy, uint8_t* d_flags,
                        size_t inner, size_t outer_stride) {
    const G1Affine* table = srs->shared->data;
    const unsigned h = srs->shared->bits, a = srs->shared->windows, hb = h - 1;
    // top tables: the kernels see n = n_real + nv scalars, the last nv of each column being its share of the groups
    const bool top = srs->shared->top_g != 0;
    const MsmCombShape sh = msm_comb_shape(h, top);
    const size_t nv = msm_comb_virtual(n_real, sh), n = n_real + nv;
    const unsigned top_delta = (unsigned)(srs->n_points - n_real);  // block of virtual scalar n_real + v = n_points + v (+ the digit's offset)
    PLONK_REQUIRE((uint64_t)n * a < ((uint64_t)1 << 32), PLONK_ERR_ARG, "MSM size %zu too large for the lookup path", n_real);
    PLONK_REQUIRE(msm_comb_top_reach_ok(n_real, sh), PLONK_ERR_ARG, "MSM size %zu too large for the top tables of %u teeth", n_real, h);
    PLONK_REQUIRE(M < ((size_t)1 << 31), PLONK_ERR_ARG, "%zu MSMs are too many for one call", M);  // (an MSM's index is a 32-bit word of the recovery list)
    // Which accumulation kernel.  The row walk (msm_comb_rows_kernel) launches W = ceil(R / 256) workgroups of rows times G chunks of
    // scalars, TWO rounds of the chip's workgroup slots: G = 2 slots / W, lowered until a chunk holds 32 scalars (a chunk's flush
    // and its addition in the row sum cost about 1.3 additions).  One round — every slot filled exactly once — is the least overhead
    // and the slowest step: the launch holds the whole chip for its length, and the other streams' kernels cannot fill in beside it;
    // more rounds buy less than their flushes cost since the short kernels take issue slots by priority (measured one to three
    // rounds, twice: docs/HISTORY.md).  It is taken when W G fills half the
    // slots; fewer MSMs — the latency paths — keep msm_comb_kernel, whose workgroups split ONE MSM.  ctx->msm_groups has no say here: it means workgroups
    // per MSM, for msm_comb_kernel alone.  Test flags (plonk_msm_lookup_configure mode | 128, | 256) force either form; with the row
    // walk forced a non-zero msm_groups is the chunk count, which makes several chunks reachable at toy sizes.
    const size_t R = M * a, W = (R + MSM_BLOCK - 1) / MSM_BLOCK, slots = 4 * (size_t)device_cus(ctx->device);
    size_t Gr = 2 * slots / W ? 2 * slots / W : 1;
    if (Gr > n / 32) Gr = n / 32 ? n / 32 : 1;
    bool rows = ctx->msm_comb_walk == 1 || (ctx->msm_comb_walk == 0 && W * Gr >= slots / 2);
    if (ctx->msm_comb_walk == 1 && ctx->msm_groups) Gr = ctx->msm_groups < n ? ctx->msm_groups : n;
    if (R > ((size_t)1 << 31) || W * Gr > ((size_t)1 << 31)) {
        PLONK_REQUIRE(ctx->msm_comb_walk != 1, PLONK_ERR_ARG, "%zu MSMs are too many for the row walk", M);
        rows = false;
    }
    // msm_comb_kernel: enough waves to occupy 1024 SIMDs three to four deep, in as few workgroups per MSM as that takes; at least two additions per lane
    unsigned G = rows ? (unsigned)Gr : msm_groups_per_msm(ctx, M, 64, 3072 / (MSM_BLOCK / 64), 0.035, n * a, 2);
    while (!rows && G > 1 && (size_t)G > n) G /= 2;
    MsmScratch s;
    const size_t part_off = s.take(M * G * a * sizeof(G1Xyzz)), col_off = s.take(rows || G >= 4 ? M * a * sizeof(G1Xyzz) : 0), cnt_off = s.take(M * 4);
    const size_t dfr_off = s.take(M * MSM_DEFER_CAP * sizeof(MsmDeferred)), dig_off = s.take(M * a * n * 4);
    const size_t redo_off = s.take(msm_redo_words(M) * sizeof(uint32_t));  // the recovery list: a part of its own, a counter and M indices
    PLONK_TRY(ctx_scratch(ctx, 1, s.total, (void**)&s.base));
    G1Xyzz *partial = s.at<G1Xyzz>(part_off), *colsum = s.at<G1Xyzz>(col_off);
    uint32_t *n_deferred = s.at<uint32_t>(cnt_off), *digits = s.at<uint32_t>(dig_off), *redo = s.at<uint32_t>(redo_off);
    MsmDeferred* deferred = s.at<MsmDeferred>(dfr_off);
    const auto teeth = std::make_integer_sequence<unsigned, MSM_COMB_MAX_TEETH - 1>();
    const msm_comb_digits_fn digits_fn = top ? msm_comb_digits_for<true>(h, teeth) : msm_comb_digits_for<false>(h, teeth);
    PLONK_REQUIRE(digits_fn, PLONK_ERR_ARG, "no comb of %u teeth", h);
    PLONK_TRY(prof_begin(ctx, "msm_digits", (double)M * (double)n * (32.0 + 4.0 * a)));
    // digits: column-major digits[row][i] for msm_comb_kernel, item-major digits[i][row] for the row walk
    const size_t dig_rs = rows ? 1 : n, dig_is = rows ? R : 1;
    digits_fn(ctx, d_scalars, n_real, stride, inner, outer_stride, M, digits, n, rows, srs->shared->base_skip, n_deferred, redo);  // (also zeroes n_deferred and the recovery list's counter)
    PLONK_TRY(prof_end(ctx));
    const size_t lds = (size_t)(MSM_BLOCK + a) * sizeof(G1Xyzz);
    PLONK_TRY(prof_begin(ctx, "msm_comb", (double)M * (96.0 * (double)n_real + 64.0)));  // (the accumulation, whichever kernel runs it)
    // every entry index fits 32 bits (and no test asked for the wide form: plonk_msm_lookup_configure mode | 64)
    const bool narrow = !ctx->msm_comb_wide && srs->shared->bytes / sizeof(G1Affine) <= ((uint64_t)1 << 32);
    const auto comb_kernel = narrow ? msm_comb_kernel<true> : msm_comb_kernel<false>;
    const auto rows_kernel = narrow ? msm_comb_rows_kernel<true> : msm_comb_rows_kernel<false>;
    if (rows)
        PLONK_LAUNCH(rows_kernel, dim3((unsigned)(W * G)), dim3(MSM_BLOCK), 0, ctx->stream, table, hb, a, (const uint32_t*)digits, (unsigned)n, (unsigned)R,
                     (unsigned)W, G, partial, deferred, (size_t)MSM_DEFER_CAP, n_deferred, (unsigned)n_real, top_delta);
    else
        PLONK_LAUNCH(comb_kernel, dim3((unsigned)(M * G)), dim3(MSM_BLOCK), lds, ctx->stream, table, hb, a,
                     (const uint32_t*)digits, n, G, partial, deferred, (size_t)MSM_DEFER_CAP, n_deferred, (unsigned)n_real, top_delta);
    PLONK_TRY(prof_end(ctx));
    const G1Xyzz* sums = partial;
    unsigned Gf = G;
    if (rows) {  // four lanes per row sum its G chunks ("msm_comb_rowsum" is recorded by the row walk alone: how a test tells the forms apart)
        PLONK_TRY(prof_begin(ctx, "msm_comb_rowsum", (double)R * (double)(G + 1) * sizeof(G1Xyzz)));
        PLONK_LAUNCH(msm_comb_rowsum_kernel, dim3((unsigned)((R + 64 / MSM_ROWSUM_LANES - 1) / (64 / MSM_ROWSUM_LANES))), dim3(64), 0, ctx->stream, (const G1Xyzz*)partial, G, (unsigned)R, a, colsum,
                     n_deferred);
        PLONK_TRY(prof_end(ctx));
        sums = colsum;
        Gf = 1;
    } else if (G >= 4) {  // few MSMs in many pieces: a wave per (MSM, column) sums the pieces in parallel
        PLONK_LAUNCH(msm_comb_colsum_kernel, dim3((unsigned)(M * a)), dim3(64), 0, ctx->stream, (const G1Xyzz*)partial, G, a, colsum, n_deferred);
        sums = colsum;
        Gf = 1;
    }
    // lanes per MSM in the Horner step (chain of a - 1 doublings and the additions between them, on lazy limbs): four for a batch
    // (12 doublings + 6 additions per lane, 16 MSMs per wave), sixteen when the MSMs are few (12 + 4: the shortest chain);
    // one lane per MSM would be the least work and the longest chain (12 + 12).
#define PLONK_COMB_FINALIZE(L)                                                                                                                      \
    PLONK_LAUNCH(msm_comb_finalize_kernel<L>, dim3((unsigned)((M * L + 63) / 64)), dim3(64), 0, ctx->stream, sums, M, Gf, a, table, hb, n,            \
                 (const MsmDeferred*)deferred, (size_t)MSM_DEFER_CAP, n_deferred, redo, d_out_xy, d_flags, (unsigned)n_real, top_delta)
    if (M >= 64) PLONK_COMB_FINALIZE(4);
    else PLONK_COMB_FINALIZE(16);
#undef PLONK_COMB_FINALIZE
    // the recovery kernel: a fixed small grid over the list finalize left (empty in every call of a prover: 16 workgroups read one word)
    PLONK_LAUNCH(msm_comb_slow_kernel, dim3(msm_slow_grid(M)), dim3(256), 0, ctx->stream, table, hb, a, (const uint32_t*)digits, n, dig_rs, dig_is,
                 (const uint32_t*)redo, (unsigned)M, d_out_xy, d_flags, (unsigned)n_real, top_delta);
    PLONK_CHECK_HIP(hipGetLastError());
    ctx->msm_redo = redo;  // (every kernel that writes the list is enqueued: plonk_msm_recovery_count)
    return PLONK_OK;
}

static const MsmTableLayout msm_comb_layout = {22,
                                               msm_comb_takes_top_for,
                                               msm_comb_additions,
                                               msm_comb_bytes,
                                               msm_comb_well_formed,
                                               msm_comb_build,
                                               msm_comb_verify,
                                               msm_run_comb};
