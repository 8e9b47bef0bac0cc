// msm_common.h — what the three MSM methods of msm.hip share: the signed-digit recoding of a scalar, the deferred-addition
// record, the result epilogue and the recovery kernel on the device; launch-shape helpers and the description of a table
// layout on the host.
#pragma once
#include <string.h>

#include "plonk_internal.h"
#include "wave.h"

#ifndef MSM_BLOCK
#define MSM_BLOCK 256
#endif
#ifndef MSM_ACC_WAVES
#define MSM_ACC_WAVES 4  // waves per SIMD the accumulate kernel is compiled for (register budget 512 / waves)
#endif
// Additions the fast formulas cannot take (accumulator == +-addend: duplicate bases, or the 2^-25 false positive
// of the cheap filter) are deferred to a per-MSM list of this many slots.  An MSM that overflows it (pathological
// input: many equal bases) is recomputed from scratch with the general formulas by msm_*_slow_kernel.
#define MSM_DEFER_CAP 256
#define LUT_VERIFY_SAMPLES 8  // bases a registered table is compared on entry by entry before it is shared (msm_tables.h)

struct MsmRecode { uint32_t k[9]; };
struct alignas(8) MsmDeferred { uint32_t bucket, entry; };  // an addition left to the method's last kernel

// Scalar vector of MSM m: scalars + (m % inner) * stride + (m / inner) * outer_stride  (lets one call commit
// several slices of each row of a [batch][4n] array, e.g. the three quotient parts).
PLONK_DEV const Fr* msm_scalar_row(const Fr* scalars, size_t m, size_t stride, size_t inner, size_t outer_stride) {
    return scalars + (m % inner) * stride + (m / inner) * outer_stride;
}

PLONK_DEV void msm_recode(const Fr* scalars, size_t idx, const MsmRecode& rc, uint32_t limb[10]) {
    Fr s = fp_from_mont(fp_load(scalars + idx));
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        carry += (uint64_t)(j < 8 ? s.v[j] : 0) + rc.k[j];
        limb[j] = (uint32_t)carry;
        carry >>= 32;
    }
    limb[9] = 0;
}

// Calls emit(w, d) for the W signed c-bit digits d of the recoded scalar, low window first.  The limbs are
// consumed through a 64-bit bit buffer with compile-time limb indices (a dynamically indexed register
// array would live in scratch memory).
template <class F> PLONK_DEV void msm_for_each_digit(const uint32_t limb[10], unsigned c, unsigned W, F emit) {
    const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
    uint64_t buf = 0;
    unsigned nb = 0, w = 0;
#pragma unroll
    for (int j = 0; j < 10; j++) {
        buf |= (uint64_t)limb[j] << nb;
        nb += 32;
        while (nb >= c && w < W) {
            emit(w, (int)((uint32_t)buf & mask) - (int)half);
            buf >>= c;
            nb -= c;
            w++;
        }
    }
}

// Result of MSM m: the unique affine representative, canonical x||y; the identity is reported out of band.
PLONK_DEV void msm_store_result(G1Xyzz sum, size_t m, Fq* out_xy, uint8_t* flags) {
    G1Affine a = g1_to_affine(sum);
    flags[m] = g1_affine_is_identity(a) ? 1 : 0;
    fp_store(out_xy + 2 * m, fp_from_mont(a.x));
    fp_store(out_xy + 2 * m + 1, fp_from_mont(a.y));
}

// Sum of the nl lanes' shares (nl = 64, 128 or 256; red: nl slots of LDS): across waves through LDS, then the last six
// levels inside wave 0 by cross-lane moves (wave.h); lane 0 stores the result.
PLONK_DEV void msm_fold_store(G1Xyzz* red, const G1Xyzz& share, unsigned tid, unsigned nl, size_t m, Fq* out_xy, uint8_t* flags) {
    red[tid] = share;
    __syncthreads();
    for (unsigned s = nl / 2; s >= 64; s >>= 1) {
        if (tid < s) {
            G1Xyzz x = red[tid];
            g1_add(x, red[tid + s]);
            red[tid] = x;
        }
        __syncthreads();
    }
    if (tid >= 64) return;
    G1Xyzz total = red[tid];
    g1_wave_reduce(total, tid);
    if (tid == 0) msm_store_result(total, m, out_xy, flags);
}

// The RECOVERY LIST of a call of M MSMs, a part of the call's scratch of its own (msm_run_comb / msm_run_windows / msm_run_bucket):
// redo[0] counts the MSMs that need the method's recovery kernel and redo[1 .. 1 + count) holds their indices, each once, in no
// particular order (count <= M: the part has 1 + M words).  The counter is zeroed where n_deferred is (the comb's digit kernel, the
// bucket method's sort kernel, the window tables' memset); the method's LAST kernel before the recovery kernel — the one place
// that sees an MSM's final count — appends; the recovery kernel strides over the list on a small fixed grid.  A call that needs no
// recovery — every call of a prover — pays a launch of MSM_SLOW_GRID workgroups that read one word, where one workgroup per MSM read
// one flag each.
#define MSM_SLOW_GRID 16
PLONK_HD size_t msm_redo_words(size_t M) { return M + 1; }
// (the slot is the atomic's return: appends from any lanes of any workgroups land in distinct words; the caller sees to it that an MSM
// is appended once, so the slot is below M: the comparison only keeps a counter that was never zeroed from writing outside the part)
PLONK_DEV void msm_redo_append(uint32_t* redo, uint32_t m, uint32_t M) {
    const uint32_t slot = atomicAdd(redo, 1u);
    if (slot < M) redo[1 + slot] = m;
}
static unsigned msm_slow_grid(size_t M) { return M < MSM_SLOW_GRID ? (unsigned)M : MSM_SLOW_GRID; }

// Recovery path (see MSM_DEFER_CAP): every MSM of the recovery list is recomputed with the general addition formulas, which handle
// every exceptional case (identity, P == Q, P == -Q), and its output overwritten.  At most MSM_SLOW_GRID workgroups stride over
// the list, a workgroup per listed MSM at a time; with an empty list — the normal case — every workgroup reads the counter and
// returns.  M bounds the list.
// kind 0: window tables (entry |d| of item (i, w));  kind 1: the bucket method's T[w][i] (|d| * T by double-and-add).
__global__ void __launch_bounds__(256) msm_slow_kernel(int kind, const G1Affine* tab, size_t table_n, unsigned c, unsigned W,
                                                       const Fr* scalars, size_t n, size_t stride, size_t inner,
                                                       size_t outer_stride, MsmRecode rc, const uint32_t* redo, unsigned M,
                                                       Fq* out_xy, uint8_t* flags) {
    PLONK_SHORT_KERNEL();
    __shared__ G1Xyzz red[256];
    const unsigned tid = threadIdx.x, count = redo[0] < M ? redo[0] : M;
#pragma unroll 1
    for (unsigned k = blockIdx.x; k < count; k += gridDim.x) {  // (count is the same in every lane: the barriers below are reached by all)
        const unsigned m = redo[1 + k];
        if (m >= M) continue;  // (never: only indices below M are appended; the same in every lane)
        const Fr* sc = msm_scalar_row(scalars, m, stride, inner, outer_stride);
        G1Xyzz acc = g1_xyzz_identity();
        for (size_t i = tid; i < n; i += 256) {
            uint32_t limb[10];
            msm_recode(sc, i, rc, limb);
            msm_for_each_digit(limb, c, W, [&](unsigned w, int d) {
                if (!d) return;
                const uint32_t ad = d < 0 ? (uint32_t)-d : (uint32_t)d;
                const G1Affine* src = kind == 0 ? tab + ((((size_t)w * table_n + i) << (c - 1)) + (ad - 1)) : tab + (size_t)w * table_n + i;
                G1Affine pt;
                pt.x = fp_load(&src->x);
                pt.y = fp_load(&src->y);
                if (d < 0) pt.y = fp_neg(pt.y);
                if (kind == 0) {
                    g1_madd<true>(acc, pt);
                } else {
                    G1Xyzz t = g1_xyzz_identity();
                    for (int bit = (int)c - 1; bit >= 0; bit--) {
                        g1_dbl(t);
                        if ((ad >> bit) & 1) g1_madd<true>(t, pt);
                    }
                    g1_add(acc, t);
                }
            });
        }
        msm_fold_store(red, acc, tid, 256, m, out_xy, flags);
        __syncthreads();  // red is written again for the workgroup's next MSM
    }
}

// ---- host side ---------------------------------------------------------------------------------
static unsigned msm_windows_for(unsigned c) {
    // Smallest W with  s + sum_w 2^(c w + c - 1) < 2^(c W)  for every canonical scalar s < r: the recoding
    // constant is < 2^(cW-1) / (1 - 2^-c), and r < 0.76 * 2^254, so c W >= 255 is enough once c >= 3
    // (17-bit windows need 15 of them, not 16).
    return c >= 3 ? (255 + c - 1) / c : (256 + c - 1) / c;
}

static void msm_recode_constant(unsigned c, unsigned W, MsmRecode* rc) {
    memset(rc, 0, sizeof *rc);
    for (unsigned w = 0; w < W; w++) {
        unsigned bit = c * w + c - 1;
        rc->k[bit >> 5] |= 1u << (bit & 31);
    }
}

// `g0` workgroups per MSM fill the chip; a launch, however, runs in ROUNDS of (CUs x 4) resident 256-thread
// workgroups, and a last round that is half empty leaves half the SIMD slots without a wave for the time of a whole round
// (M = 1536 MSMs at one workgroup each: 1.5 rounds on 1024 slots — two of the four MSM launches of a lock-step batch of 512 proofs).
// Cutting every MSM into twice the workgroups halves the length of a round for `overhead` more work per workgroup (its tree
// reduction / its extra pieces): taken when the model  rounds x (1 / G + overhead)  says it pays by more than 3 %.
// Measured (profiles/r05_f_msm_rounds_stagger_ab.json, r05_d_msm_sweep.jsonl): 1152 MSMs on the
// bucket method 5.59 -> 5.14 ms per call; the prover's own launch shapes gain under 1 % on either method.
static unsigned msm_round_aware_groups(int device, size_t M, unsigned g0, unsigned g_max, double overhead) {
    if (g0 >= g_max) return g0;
    const double slots = 4.0 * (double)device_cus(device);
    auto cost = [&](unsigned G) {
        const double wgs = (double)M * G;
        double rounds = wgs / slots;
        rounds = rounds <= 1.0 ? 1.0 : (double)(size_t)(rounds + 0.999999);
        return rounds * (1.0 / G + overhead);
    };
    return cost(2 * g0) < 0.97 * cost(g0) ? 2 * g0 : g0;
}

// Workgroups per MSM: the caller's (plonk_msm_configure), else the power of two <= cap that brings the launch to `fill`
// workgroups, doubled where the rounds say so; either way no more than leave every lane `min_per_lane` of the MSM's items.
static unsigned msm_groups_per_msm(const plonk_ctx* ctx, size_t M, unsigned cap, size_t fill, double overhead, size_t items, unsigned min_per_lane) {
    unsigned G = ctx->msm_groups;
    if (!G) {
        G = 1;
        while (G < cap && M * G < fill) G *= 2;
        G = msm_round_aware_groups(ctx->device, M, G, cap, overhead);
    }
    while (G > 1 && (size_t)G * MSM_BLOCK * min_per_lane > items) G /= 2;
    return G;
}

// Carves one scratch allocation into 256-byte aligned parts: take() every part, allocate `total`, then at().
struct MsmScratch {
    size_t total = 0;
    uint8_t* base = nullptr;
    size_t take(size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    }
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

// What the registry and the policy (msm_tables.h) know of a table layout; the instances are msm_windows_layout and msm_comb_layout.
// bits: window bits c / teeth h;  top: the comb's variant with top tables (window tables have none).
struct MsmTableLayout {
    unsigned auto_max_bits;                                            // the widest table the automatic choice considers
    bool (*takes_top)(size_t n, unsigned bits);                        // the `top` variant exists for n bases
    double (*additions)(unsigned bits, bool top);                      // mixed additions per base and MSM
    size_t (*bytes)(size_t n, unsigned bits, bool top);                // the table plus the staging of its build
    bool (*well_formed)(const MsmLookupTable* t);                      // t's windows / top tables / bytes are what build() gives for its bits
    // fills t (kind, bits, windows, top_*, data, bytes); PLONK_ERR_NOMEM (nothing allocated) if it does not fit
    int (*build)(plonk_ctx* ctx, const plonk_srs* srs, unsigned bits, bool top, MsmLookupTable* t);
    void (*verify)(plonk_ctx* ctx, const plonk_srs* srs, const MsmLookupTable* t, unsigned* d_mismatches);  // enqueues the comparison with srs->bases
    int (*run)(plonk_ctx* ctx, const plonk_srs* srs, const Fr* d_scalars, size_t n, size_t M, size_t stride, Fq* d_out_xy, uint8_t* d_flags, size_t inner,
               size_t outer_stride);                                   // on srs->shared
};
