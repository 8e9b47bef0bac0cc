// msm.hip — batched fixed-base multi-scalar multiplication on BN254 G1.
//
// Reference behaviour replaced: ec_lincomb -> lincomb -> multisubset
// (/root/reference/curve.py:38-111), i.e. everything Setup.commit does after its ifft
// (setup.py:66-72).  The reference bit-slices the scalars into 255 subsets and adds affine points
// with one Fq inversion per addition (~109k additions for N = 2^11); the result is a group element,
// so any correct schedule yields the same affine point.  The schedules:
//
// A. TABLE MSM — for a reusable SRS (plonk_srs_load_ptau), within the HBM budget the caller grants (1/16 of the device's memory by
//    default; bench.py opts into 180 GB).  ONE table per (device, base set, layout, bits), shared by every context.
//    A1. comb tables (msm_comb.h, the default): 2^(h-1) entries per base, N * ceil(254 / h) mixed additions per MSM — 13 per base
//        from 68.7 GB, 15 from 8.6 GB for 2^11 points — and ceil(254 / h) - 1 doublings per MSM; with TOP TABLES (round 6: floor(254 / h)
//        columns + a joint table per g bases for the bits left over) 12.15 per base from 157.6 GB (h = 21, g = 7).
//    A2. window tables (rounds 2 - 5; plonk_msm_lookup_configure mode | 16): every multiple L[w][i][d] = d * 2^(c w) * P_i a signed
//        c-bit digit can select (128.8 GB at c = 17 for 2^11 points), N * ceil(255 / c) mixed additions of looked-up points:
//      msm_lookup_kernel           lanes walk flat ranges of (scalar, window) items, 64 random bytes per item
//      msm_lookup_finalize_kernel  sum of the workgroup partials + deferred additions -> canonical affine
//    See msm_windows.h.  The registry of tables and the choice of one for a budget: msm_tables.h.
//
// B. BUCKET METHOD (Pippenger, msm_bucket.h) — arbitrary bases (plonk_srs_load_affine), or when no table fits.
//    A window table T[w][i] = 2^(c*w) * P_i is built once per base set; every window of every scalar then lands
//    in ONE shared bucket set and no doublings remain in the per-MSM work:
//   1. msm_sort_kernel        (one workgroup per MSM) scalar -> canonical -> + sum_w 2^(cw+c-1), signed
//                             digits d_w in [-2^(c-1), 2^(c-1)); LDS counting sort (LDS atomics) of all
//                             W*N (point, window) entries by bucket |d|; the sorted entry list and the
//                             bucket boundaries go to HBM (~210 KiB per MSM).
//   2. msm_accumulate_kernel  (G workgroups per MSM) the sorted list is cut into EQUAL flat ranges, one per
//                             lane, so every lane performs the same number of mixed additions whatever the
//                             bucket sizes.  A lane sums its range top-down and stores one partial sum
//                             ("piece") per bucket it touches: a bucket boundary costs a 128-byte store,
//                             never a group operation, so the wave does not serialise on boundaries that
//                             its lanes cross at different steps.  >= 80 % of this method's time.
//   3. msm_bucket_reduce_kernel (two waves per MSM) lane l owns K/128 consecutive buckets: walking them top-down,
//                             run += pieces of bucket k, tot += run; its share is tot + (first bucket - 1) * run, the
//                             second term from a cross-lane suffix scan of the runs (round 4);
//                             shares are summed across waves through LDS and then inside wave 0 by a cross-lane
//                             butterfly (wave.h: DPP / ds_swizzle / v_permlane32_swap — the "wave-reduced bucket
//                             sum"); lane 0 converts the result to the unique affine representative, canonical x||y.
//                             Buckets never exist in memory.
//    Window-table reads hit L2 / Infinity Cache (3.4 MiB at c = 10).
//
// Both inner loops keep the accumulator as 9 x 29-bit limbs with lazy reductions (fpl.h, g1l_madd_fast) and run
// at the rate of a bare mixed-addition loop (13.4 G additions/s chip-wide): the kernels are integer-ALU bound.
// Steps the fast formulas cannot take are deferred to a 256-slot list per MSM; an MSM that overflows it is redone by
// msm_slow_kernel (msm_common.h).  msm_lagrange_srs builds the Lagrange-basis view of an SRS out of the same kernels.
// This file: the kernels every table build uses, the Lagrange-basis SRS, and msm_run_device, which picks the method.
#include <stdlib.h>
#include <string.h>

#include "msm_bucket.h"
#include "msm_tables.h"

#define MSM_DEFAULT_WINDOW_BITS 10  // of the bucket method

// ------------------------------------------------------------------------------------------------
// Window table: table[w*n + i] = 2^(c*w) * bases[i], affine.
__global__ void msm_table_kernel(const G1Affine* bases, size_t n, unsigned c, unsigned W, G1Xyzz* tmp) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        G1Affine b;
        b.x = fp_load(&bases[i].x);
        b.y = fp_load(&bases[i].y);
        G1Xyzz p = g1_xyzz_from_affine(b);
        for (unsigned w = 0; w < W; w++) {
            tmp[(size_t)w * n + i] = p;
            if (w + 1 < W)
                for (unsigned k = 0; k < c; k++) g1_dbl(p);
        }
    }
}

void msm_window_bases(plonk_ctx* ctx, const G1Affine* bases, size_t n, unsigned c, unsigned W, G1Xyzz* out) {
    PLONK_LAUNCH(msm_table_kernel, grid1(n, 64, 2048), dim3(64), 0, ctx->stream, bases, n, c, W, out);
}

// XYZZ -> affine for a whole array, Montgomery's trick over chunks of 8 (identity -> (0,0)).
#define AFF_CHUNK 8
__global__ void __launch_bounds__(64) g1_batch_to_affine_kernel(const G1Xyzz* in, G1Affine* out, size_t n) {
    size_t nchunks = (n + AFF_CHUNK - 1) / AFF_CHUNK;
    for (size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x; ch < nchunks; ch += (size_t)gridDim.x * blockDim.x) {
        size_t base = ch * AFF_CHUNK;
        Fq pre[AFF_CHUNK];  // prefix products in registers (compile-time indices); zz zzz is formed again on the way back
        Fq acc = fp_one<FqParams>();
        wave_for<AFF_CHUNK>([&](auto K) {
            constexpr unsigned k = decltype(K)::value;
            Fq den = fp_zero<FqParams>();
            if (base + k < n) den = fp_mul(fp_load(&in[base + k].zz), fp_load(&in[base + k].zzz));  // zero <=> identity
            pre[k] = acc;
            if (!fp_is_zero(den)) acc = fp_mul(acc, den);
        });
        acc = fp_inv(acc);
        wave_for_down<AFF_CHUNK>([&](auto K) {
            constexpr unsigned k = decltype(K)::value;
            if (base + k < n) {
                const G1Xyzz& p = in[base + k];
                const Fq zz = fp_load(&p.zz), zzz = fp_load(&p.zzz), den = fp_mul(zz, zzz);
                G1Affine r = g1_affine_identity();
                if (!fp_is_zero(den)) {
                    const Fq t = fp_mul(acc, pre[k]);  // 1 / (zz * zzz)
                    acc = fp_mul(acc, den);
                    r.x = fp_mul(fp_load(&p.x), fp_mul(t, zzz));
                    r.y = fp_mul(fp_load(&p.y), fp_mul(t, zz));
                }
                fp_store(&out[base + k].x, r.x);
                fp_store(&out[base + k].y, r.y);
            }
        });
    }
}

void g1_batch_to_affine(plonk_ctx* ctx, const G1Xyzz* in, G1Affine* out, size_t n, size_t max_groups) {
    if (!n) return;
    PLONK_LAUNCH(g1_batch_to_affine_kernel, grid1((n + AFF_CHUNK - 1) / AFF_CHUNK, 64, max_groups), dim3(64), 0, ctx->stream, in, out, n);
}

// ------------------------------------------------------------------------------------------------
// Lagrange-basis SRS (setup.py:66-72 says commit = ifft + lincomb with powers_of_x): the points
//     [L_i(tau)]_1 = sum_j (w^(-ij) / n) [tau^j]_1,      i < n = 2^log_n,
// i.e. the inverse DFT of the SRS over the group, computed once per (SRS, n) — as n batched MSMs over the
// monomial bases whose scalar rows are the inverse NTT of the identity matrix (row i = coefficients of L_i), so the
// "EC-iNTT" reuses the NTT and MSM kernels as they are (2^11 rows: a few milliseconds on the lookup table).
// commit(values) = sum_i values_i [L_i(tau)]_1 is then one MSM with no inverse NTT in front of it.
__global__ void fr_identity_rows_kernel(Fr* out, size_t n, size_t row0, size_t rows) {
    const size_t total = rows * n;
    const Fr one = fp_one<FrParams>(), zero = fp_zero<FrParams>();
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t r = gI / n, j = gI - r * n;
        fp_store(out + gI, j == row0 + r ? one : zero);
    }
}
__global__ void fq_to_mont_kernel(const Fq* in, Fq* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fp_store(out + i, fp_to_mont(fp_load(in + i)));
}

// the view of `srs` on the 2^log_n Lagrange-basis points `bases` (device; owned by the view), filed under srs->lagrange
static plonk_srs* msm_lagrange_child(plonk_srs* srs, unsigned log_n, G1Affine* bases) {
    plonk_srs* child = new plonk_srs();
    child->device = srs->device;
    child->n_points = (size_t)1 << log_n;
    child->bases = bases;
    child->fixed = srs->fixed;
    child->parent = srs;
    const uint64_t tag[2] = {srs->content_key, 0x4c61677200000000ull | log_n};  // "Lagr" | log_n
    child->content_key = plonk_fnv1a64(tag, sizeof tag);
    srs->lagrange[log_n] = child;
    return child;
}

int msm_lagrange_srs(plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, plonk_srs** out) {
    auto it = srs->lagrange.find(log_n);
    if (it != srs->lagrange.end()) {
        *out = it->second;
        return PLONK_OK;
    }
    const size_t n = (size_t)1 << log_n;
    PLONK_REQUIRE(n <= srs->n_points, PLONK_ERR_ARG, "Lagrange basis of size %zu needs %zu powers, the SRS has %zu", n, n, srs->n_points);
    PLONK_REQUIRE(log_n <= PLONK_FR_TWO_ADICITY, PLONK_ERR_ARG, "size 2^%u exceeds the 2-adicity of Fr", log_n);
    // Two routes to the same points (bit-identical: both end in the unique affine representative).  Up to 2^12: n MSMs over the
    // monomial bases (below) — a few milliseconds once the lookup table exists, but quadratic.  Above: the inverse DFT over the
    // group (g1_ntt.hip), n log n group operations.  PLONK_LAGRANGE_SRS = msm / ntt forces one (tests, A/B).
    {
        const char* e = getenv("PLONK_LAGRANGE_SRS");
        const bool by_ntt = e ? !strcmp(e, "ntt") : log_n > 12;
        if (by_ntt) {
            G1Affine* nb = nullptr;
            if (!plonk_dev_malloc(&nb, n * sizeof(G1Affine))) {
                plonk_set_error("hipMalloc failed while building the Lagrange-basis SRS of size %zu", n);
                return PLONK_ERR_NOMEM;
            }
            const int rcn = g1_lagrange_by_ntt(ctx, srs, log_n, nb);
            if (rcn != PLONK_OK) {
                hipFree(nb);
                return rcn;
            }
            *out = msm_lagrange_child(srs, log_n, nb);
            return PLONK_OK;
        }
    }
    const size_t rows = n < 1024 ? n : 1024;  // rows per round: bounds the scalar matrix at 1024 * n elements
    void *mat = nullptr, *res = nullptr, *bases = nullptr;
    auto cleanup = [&]() {
        if (mat) hipFree(mat);
        if (res) hipFree(res);
    };
    if (!plonk_dev_malloc(&mat, rows * n * sizeof(Fr)) || !plonk_dev_malloc(&res, rows * (2 * sizeof(Fq) + 1) + 64) ||
        !plonk_dev_malloc(&bases, n * sizeof(G1Affine))) {
        cleanup();
        if (bases) hipFree(bases);
        plonk_set_error("hipMalloc failed while building the Lagrange-basis SRS of size %zu", n);
        return PLONK_ERR_NOMEM;
    }
    Fq* d_xy = (Fq*)res;
    uint8_t* d_fl = (uint8_t*)res + rows * 2 * sizeof(Fq);
    int rc = PLONK_OK;
    for (size_t row0 = 0; row0 < n && rc == PLONK_OK; row0 += rows) {
        PLONK_LAUNCH(fr_identity_rows_kernel, grid1(rows * n), dim3(256), 0, ctx->stream, (Fr*)mat, n, row0, rows);
        rc = ntt_run(ctx, ntt_inverse((const Fr*)mat, (Fr*)mat, log_n, rows));
        if (rc == PLONK_OK) rc = msm_run_device(ctx, srs, (const Fr*)mat, n, rows, n, d_xy, d_fl);
        if (rc == PLONK_OK) {  // canonical x||y -> Montgomery bases; the identity stays (0, 0)
            unsigned g2 = (unsigned)((2 * rows + 255) / 256);
            PLONK_LAUNCH(fq_to_mont_kernel, dim3(g2), dim3(256), 0, ctx->stream, (const Fq*)d_xy, (Fq*)((G1Affine*)bases + row0), 2 * rows);
        }
    }
    if (rc == PLONK_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)) {
        plonk_set_error("building the Lagrange-basis SRS failed on the device");
        rc = PLONK_ERR_HIP;
    }
    cleanup();
    if (rc != PLONK_OK) {
        hipFree(bases);
        return rc;
    }
    *out = msm_lagrange_child(srs, log_n, (G1Affine*)bases);
    return PLONK_OK;
}

// Enqueue a batch of M MSMs; results land in device buffers (d_out_xy: 2*M Fq canonical, d_flags: M bytes).
int msm_run_device(plonk_ctx* ctx, plonk_srs* srs, const Fr* d_scalars, size_t n, size_t M, size_t stride,
                   Fq* d_out_xy, uint8_t* d_flags, size_t inner, size_t outer_stride) {
    if (!inner) inner = M ? M : 1;
    PLONK_REQUIRE(n >= 1 && n <= srs->n_points, PLONK_ERR_ARG, "MSM size %zu exceeds the %zu loaded bases", n, srs->n_points);
    if (!M) return PLONK_OK;
    ctx->msm_redo = nullptr;  // (scratch slot 1 may move below: the method's run sets it again once its kernels are enqueued)
    if (msm_table_prepare(ctx, srs)) return msm_layout(srs->shared->kind).run(ctx, srs, d_scalars, n, M, stride, d_out_xy, d_flags, inner, outer_stride);
    const unsigned c = ctx->msm_window_bits ? ctx->msm_window_bits : MSM_DEFAULT_WINDOW_BITS;
    return msm_run_bucket(ctx, srs, c, d_scalars, n, M, stride, d_out_xy, d_flags, inner, outer_stride);
}
