// msm_windows.h — fixed-base MSM on WINDOW tables (rounds 2 - 5; plonk_msm_lookup_configure mode | 16).  MI355X has 288 GB of HBM; a reusable SRS of 2^11 points affords the table of EVERY multiple
//     L[w][i][d] = d * 2^(c w) * P_i,   d = 1 .. 2^(c-1)      (128.8 GB at c = 17, 68.7 GB at c = 16)
// so that an MSM is just N * ceil(255 / c) mixed additions of looked-up points (30 720 at c = 17 against
// 53 248 sorted bucket additions plus the bucket reduction): 64 random bytes from HBM per addition — the chip
// sustains 20 G such reads/s (tools/ubench/gather.hip) against the 16-19 G additions/s its ALUs can do.
// Signed digits as in the bucket method; a lane walks a flat range of (scalar, window) items.
#pragma once
#include "msm_common.h"

// tmp[i * half + d - 1] = d * wbase[w * n + i] for one window w, XYZZ (converted by g1_batch_to_affine_kernel)
__global__ void __launch_bounds__(64) msm_lookup_fill_kernel(const G1Affine* wbase, size_t n, unsigned c, unsigned w, G1Xyzz* tmp) {
    const size_t half = (size_t)1 << (c - 1);
    const size_t seg_len = half < 256 ? half : 256, nseg = half / seg_len;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n * nseg; id += (size_t)gridDim.x * blockDim.x) {
        const size_t i = id / nseg, k = (id % nseg) * seg_len;  // this lane fills multiples k+1 .. k+seg_len
        G1Affine b;
        b.x = fp_load(&wbase[(size_t)w * n + i].x);
        b.y = fp_load(&wbase[(size_t)w * n + i].y);
        G1Xyzz acc = g1_xyzz_identity();
#pragma unroll 1
        for (int bit = (int)c - 1; bit >= 0; bit--) {  // acc = k * b
            g1_dbl(acc);
            if ((k >> bit) & 1) g1_madd<true>(acc, b);
        }
        G1Xyzz* out = tmp + i * half + k;
#pragma unroll 1
        for (size_t j = 0; j < seg_len; j++) {
            g1_madd<true>(acc, b);
            out[j] = acc;
        }
    }
}

// item = i * W + w.  Which items a lane adds (`strided`, chosen by the host):
//   strided (n >= lanes: every batch of the prover)  lane t of the MSM's 256 * G lanes takes the scalars i = t, t + lanes, ..,
//       all W windows of one scalar before the next.  At any moment the lanes of a workgroup — and, because every workgroup
//       of a launch walks the same sequence at the same pace, the lanes of the whole chip — read the table slabs of ONE
//       window and `lanes` CONSECUTIVE bases: a contiguous 1 - 2 GB of the 128.8 GB table.  The table look-ups are random
//       64-byte reads; what they cost is address translation, not bandwidth (round 5, profiles/r05_valu_summary.json: random
//       64-byte reads run at 40 G/s over a span of <= 2 GiB and at 20 G/s from 8 GiB up, where 88 - 94 % of the UTCL1 requests
//       miss and the UTCL2 is busy 99.5 % of the time; this kernel with round 4's order — each lane 8 consecutive scalars, the
//       chip spread over the whole table — had 92.5 % UTCL1 misses and the UTCL2 busy 92.6 % of its duration).
//   flat (a lone MSM cut into more lanes than it has scalars)  lane t adds items [t * per, (t + 1) * per).
__global__ void __launch_bounds__(MSM_BLOCK, MSM_ACC_WAVES) msm_lookup_kernel(
    const G1Affine* lookup, size_t table_n, unsigned c, unsigned W, const Fr* scalars, size_t n, size_t stride, size_t inner,
    size_t outer_stride, MsmRecode rc, unsigned G, G1Xyzz* partial, MsmDeferred* deferred, size_t deferred_stride,
    uint32_t* n_deferred, unsigned strided) {
    PLONK_DYN_SMEM(smem);  // MSM_BLOCK x 128 B: first each lane's recoded scalar (10 words), then the tree reduction
    const unsigned m = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
    uint32_t* row = reinterpret_cast<uint32_t*>(smem) + tid * 10;
    G1Xyzz* red = reinterpret_cast<G1Xyzz*>(smem);
    const Fr* sc = msm_scalar_row(scalars, m, stride, inner, outer_stride);
    const uint32_t items = (uint32_t)(n * W), lanes = G * MSM_BLOCK, t = g * MSM_BLOCK + tid;
    const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
    uint32_t i, w, count, step;
    if (strided) {
        i = t;
        w = 0;
        count = t < n ? (((uint32_t)n - 1 - t) / lanes + 1) * W : 0;
        step = lanes;
    } else {
        const uint32_t per = (items + lanes - 1) / lanes;
        const uint64_t lo64 = (uint64_t)t * per;
        const uint32_t lo = lo64 < items ? (uint32_t)lo64 : items;
        const uint32_t hi = lo64 + per < items ? (uint32_t)(lo64 + per) : items;
        i = lo / W;
        w = lo - i * W;
        count = hi - lo;
        step = 1;
    }

    G1XyzzL run = g1l_identity();
    bool fresh = true;
    for (uint32_t k = 0; k < count; k++) {
        if (fresh) {  // new scalar: canonical value + recoding constant, parked in this lane's LDS row
            uint32_t limb[10];
            msm_recode(sc, i, rc, limb);
#pragma unroll
            for (int j = 0; j < 10; j++) row[j] = limb[j];
            fresh = false;
        }
        const unsigned bit = c * w, j = bit >> 5, sh = bit & 31;
        const uint64_t two = (uint64_t)row[j] | ((uint64_t)row[j + 1] << 32);
        const int d = (int)((uint32_t)(two >> sh) & mask) - (int)half;
        if (d) {
            const uint32_t ad = d < 0 ? (uint32_t)-d : (uint32_t)d;
            const G1Affine* src = lookup + ((((size_t)w * table_n + i) << (c - 1)) + (ad - 1));
            const Fq x = fp_load(&src->x), y = fp_load(&src->y);
            if (!g1l_madd_fast(run, x, y, d < 0) && !(fp_is_zero(x) && fp_is_zero(y))) {  // see msm_accumulate_kernel
                const uint32_t slot = atomicAdd(n_deferred + m, 1u);
                if (slot < MSM_DEFER_CAP) deferred[(size_t)m * deferred_stride + slot] = MsmDeferred{i * W + w, (uint32_t)d};
            }
        }
        if (++w == W) {
            w = 0;
            i += step;
            fresh = true;
        }
    }
    __syncthreads();  // the scalar rows are dead: the same LDS now carries the reduction
    red[tid] = g1l_to_piece(run);
    red[tid] = g1_piece_load(&red[tid]);
    __syncthreads();
    // Tree reduction through LDS.  (A wave-level butterfly for the last six levels — wave.h, as in the bucket reduction
    // below — was measured here and is 1.7 % slower end to end: inlined it costs the 128-VGPR loop 51 spilled registers,
    // out of line the accumulator travels through scratch; profiles/r02_g_msm_reduce_ab.txt.)
    for (unsigned s = MSM_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            G1Xyzz x = red[tid];
            g1_add(x, red[tid + s]);
            red[tid] = x;
        }
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)m * G + g] = red[0];
}

// acc += the deferred additions of MSM m
PLONK_DEV void msm_windows_add_deferred(G1Xyzz& acc, size_t m, const G1Affine* lookup, size_t table_n, unsigned c, unsigned W,
                                        const MsmDeferred* deferred, size_t deferred_stride, const uint32_t* n_deferred, uint32_t* redo,
                                        size_t M) {
    const uint32_t nd = n_deferred[m] < MSM_DEFER_CAP ? n_deferred[m] : MSM_DEFER_CAP;  // past the cap: msm_slow_kernel
    if (n_deferred[m] > MSM_DEFER_CAP) msm_redo_append(redo, (uint32_t)m, (uint32_t)M);  // (called by one lane per MSM, after the accumulation)
    for (uint32_t k = 0; k < nd; k++) {
        const MsmDeferred e = deferred[m * deferred_stride + k];
        const uint32_t i = e.bucket / W, w = e.bucket - i * W;  // `bucket` carries the item index here
        const int d = (int)e.entry;
        const uint32_t ad = d < 0 ? (uint32_t)-d : (uint32_t)d;
        const G1Affine* src = lookup + ((((size_t)w * table_n + i) << (c - 1)) + (ad - 1));
        G1Affine pt;
        pt.x = fp_load(&src->x);
        pt.y = fp_load(&src->y);
        if (d < 0) pt.y = fp_neg(pt.y);
        g1_madd(acc, pt);
    }
}

// out_xy[m] = canonical affine of sum_g partial[m][g] + the deferred additions; flags[m] = 1 for the identity
__global__ void __launch_bounds__(64) msm_lookup_finalize_kernel(const G1Xyzz* partial, size_t M, unsigned G, const G1Affine* lookup,
                                                                 size_t table_n, unsigned c, unsigned W, const MsmDeferred* deferred,
                                                                 size_t deferred_stride, const uint32_t* n_deferred, uint32_t* redo,
                                                                 Fq* out_xy, uint8_t* flags) {
    for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (size_t)gridDim.x * blockDim.x) {
        G1Xyzz acc = partial[m * G];
        for (unsigned g = 1; g < G; g++) g1_add(acc, partial[m * G + g]);
        msm_windows_add_deferred(acc, m, lookup, table_n, c, W, deferred, deferred_stride, n_deferred, redo, M);
        msm_store_result(acc, m, out_xy, flags);
    }
}

// The same for few MSMs cut into many workgroups (a lone commitment: G = 64): one WAVE per MSM, lane g takes partial g and
// the 64 of them are summed by the cross-lane butterfly of wave.h (six general additions instead of 63 in a row — the
// serial form made a lone 2^11 commitment 0.75 ms, most of the reference-shaped Prover's latency); lane 0 finishes.
__global__ void __launch_bounds__(64) msm_lookup_finalize_wave_kernel(const G1Xyzz* partial, size_t M, unsigned G, const G1Affine* lookup,
                                                                      size_t table_n, unsigned c, unsigned W, const MsmDeferred* deferred,
                                                                      size_t deferred_stride, const uint32_t* n_deferred, uint32_t* redo,
                                                                      Fq* out_xy, uint8_t* flags) {
    const size_t m = blockIdx.x;
    const unsigned lane = threadIdx.x;
    G1Xyzz acc = g1_xyzz_identity();
    for (unsigned g = lane; g < G; g += 64) {  // G <= 64 in practice: at most one partial per lane
        if (g == lane) acc = partial[m * G + g];
        else g1_add(acc, partial[m * G + g]);
    }
    g1_wave_reduce(acc, lane);
    if (lane) return;
    msm_windows_add_deferred(acc, m, lookup, table_n, c, W, deferred, deferred_stride, n_deferred, redo, M);
    msm_store_result(acc, m, out_xy, flags);
}

// Comparison of a registered window table with THIS SRS's bases (msm_tables.h, lut_verified):
//   1. its d = 1 entries of window 0 — the bases themselves — ALL equal this SRS's bases (lut_verify_kernel);
//   2. for LUT_VERIFY_SAMPLES bases spread over the set and EVERY window w, its d = 1 entry equals 2^(c w) P_i and its last
//      entry (d = 2^(c-1)) equals 2^(c w + c - 1) P_i, both recomputed here by doublings from this SRS's own base
//      (lut_verify_windows_kernel) — a table of another window size or window count filed under the same key, or one whose
//      higher windows belong to other bases, fails here.
__global__ void lut_verify_kernel(const G1Affine* bases, const G1Affine* lookup, size_t n, unsigned c, unsigned* mismatches) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine* e = lookup + (i << (c - 1));
    if (!fp_eq(fp_load(&bases[i].x), fp_load(&e->x)) || !fp_eq(fp_load(&bases[i].y), fp_load(&e->y))) atomicAdd(mismatches, 1u);
}
// lane = (sample s, window w): P = 2^(c w) bases[i_s] by doublings; compare with entries d = 1 and d = 2^(c-1) of (w, i_s)
__global__ void __launch_bounds__(64) lut_verify_windows_kernel(const G1Affine* bases, const G1Affine* lookup, size_t n, unsigned c, unsigned W,
                                                                unsigned* mismatches) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= LUT_VERIFY_SAMPLES * W) return;
    const unsigned s = t / W, w = t - s * W;
    const size_t i = n <= LUT_VERIFY_SAMPLES ? (s < n ? s : n - 1) : (size_t)s * (n - 1) / (LUT_VERIFY_SAMPLES - 1);
    G1Affine b;
    b.x = fp_load(&bases[i].x);
    b.y = fp_load(&bases[i].y);
    if (g1_affine_is_identity(b)) return;  // (0, 0) stays (0, 0) in every window: covered by check 1
    G1Xyzz p = g1_xyzz_from_affine(b);
#pragma unroll 1
    for (unsigned k = 0; k < c * w; k++) g1_dbl(p);
    const G1Affine* e = lookup + ((((size_t)w * n + i) << (c - 1)));
    G1Affine a = g1_to_affine(p);
    bool ok = fp_eq(a.x, fp_load(&e[0].x)) && fp_eq(a.y, fp_load(&e[0].y));
#pragma unroll 1
    for (unsigned k = 0; k + 1 < c; k++) g1_dbl(p);
    a = g1_to_affine(p);
    const size_t last = ((size_t)1 << (c - 1)) - 1;
    ok = ok && fp_eq(a.x, fp_load(&e[last].x)) && fp_eq(a.y, fp_load(&e[last].y));
    if (!ok) atomicAdd(mismatches, 1u);
}

// ---- host side ---------------------------------------------------------------------------------
static size_t msm_windows_bytes(size_t n, unsigned c, bool) {  // table + the XYZZ staging buffer of one window
    const size_t half = (size_t)1 << (c - 1);
    return n * msm_windows_for(c) * half * sizeof(G1Affine) + n * half * sizeof(G1Xyzz);
}
static bool msm_windows_well_formed(const MsmLookupTable* t) {
    return t->windows == msm_windows_for(t->bits) && t->bytes == t->n_points * t->windows * ((size_t)1 << (t->bits - 1)) * sizeof(G1Affine);
}

static int msm_windows_build(plonk_ctx* ctx, const plonk_srs* srs, unsigned c, bool, MsmLookupTable* t) {
    const unsigned W = msm_windows_for(c);
    const size_t n = srs->n_points, half = (size_t)1 << (c - 1);
    void *wx = nullptr, *wb = nullptr, *tmp = nullptr, *tab = nullptr;
    auto fail = [&]() {
        for (void* q : {wx, wb, tmp, tab})
            if (q) hipFree(q);
        (void)hipGetLastError();
        plonk_set_error("the %u-bit lookup table (%zu MiB) does not fit in device memory", c, msm_windows_bytes(n, c, false) >> 20);
        return PLONK_ERR_NOMEM;
    };
    if (!plonk_dev_malloc(&tab, n * W * half * sizeof(G1Affine))) return fail();
    if (!plonk_dev_malloc(&tmp, n * half * sizeof(G1Xyzz))) return fail();
    if (!plonk_dev_malloc(&wx, n * W * sizeof(G1Xyzz))) return fail();
    if (!plonk_dev_malloc(&wb, n * W * sizeof(G1Affine))) return fail();
    // window bases 2^(c w) P_i, affine
    msm_window_bases(ctx, srs->bases, n, c, W, (G1Xyzz*)wx);
    g1_batch_to_affine(ctx, (const G1Xyzz*)wx, (G1Affine*)wb, n * W, 4096);
    const size_t seg_len = half < 256 ? half : 256, fill_lanes = n * (half / seg_len);
    for (unsigned w = 0; w < W; w++) {
        PLONK_LAUNCH(msm_lookup_fill_kernel, grid1(fill_lanes, 64, 65536), dim3(64), 0, ctx->stream, (const G1Affine*)wb, n, c, w, (G1Xyzz*)tmp);
        g1_batch_to_affine(ctx, (const G1Xyzz*)tmp, (G1Affine*)tab + (size_t)w * n * half, n * half);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return fail();
    for (void* q : {wx, wb, tmp}) hipFree(q);
    t->kind = MSM_TABLE_WINDOWS;
    t->bits = c;
    t->windows = W;
    t->data = (G1Affine*)tab;
    t->bytes = n * W * half * sizeof(G1Affine);
    return PLONK_OK;
}

static void msm_windows_verify(plonk_ctx* ctx, const plonk_srs* srs, const MsmLookupTable* t, unsigned* d_mismatches) {
    PLONK_LAUNCH(lut_verify_kernel, dim3((unsigned)((srs->n_points + 255) / 256)), dim3(256), 0, ctx->stream, (const G1Affine*)srs->bases,
                 (const G1Affine*)t->data, srs->n_points, t->bits, d_mismatches);
    PLONK_LAUNCH(lut_verify_windows_kernel, dim3((LUT_VERIFY_SAMPLES * t->windows + 63) / 64), dim3(64), 0, ctx->stream,
                 (const G1Affine*)srs->bases, (const G1Affine*)t->data, srs->n_points, t->bits, t->windows, d_mismatches);
}

static int msm_run_windows(plonk_ctx* ctx, const plonk_srs* srs, const Fr* d_scalars, size_t n, size_t M, size_t stride, Fq* d_out_xy,
                           uint8_t* d_flags, size_t inner, size_t outer_stride) {
    const G1Affine* table = srs->shared->data;
    const unsigned c = srs->shared->bits, W = srs->shared->windows;
    const size_t items = n * W;
    PLONK_REQUIRE(items < ((size_t)1 << 32), PLONK_ERR_ARG, "MSM size %zu too large for the lookup path", n);
    // enough waves to occupy 1024 SIMDs three to four deep, in as few workgroups per MSM as that takes; at least two additions per lane
    const unsigned G = msm_groups_per_msm(ctx, M, 64, 3072 / (MSM_BLOCK / 64), 0.027, items, 2);
    MsmScratch s;
    const size_t part_off = s.take(M * G * sizeof(G1Xyzz)), cnt_off = s.take(M * 4), dfr_off = s.take(M * MSM_DEFER_CAP * sizeof(MsmDeferred));
    const size_t redo_off = s.take(msm_redo_words(M) * sizeof(uint32_t));  // the recovery list: a part of its own, a counter and M indices
    PLONK_TRY(ctx_scratch(ctx, 1, s.total, (void**)&s.base));
    G1Xyzz* partial = s.at<G1Xyzz>(part_off);
    uint32_t *n_deferred = s.at<uint32_t>(cnt_off), *redo = s.at<uint32_t>(redo_off);
    MsmDeferred* deferred = s.at<MsmDeferred>(dfr_off);
    MsmRecode rc;
    msm_recode_constant(c, W, &rc);
    // lanes walk scalars t, t + lanes, .. (window after window) whenever every lane gets a scalar: the chip then reads one
    // contiguous 1 - 2 GB of the table at a time, which the translation caches hold (see msm_lookup_kernel)
    const unsigned strided = n >= (size_t)G * MSM_BLOCK ? 1u : 0u;
    PLONK_CHECK_HIP(hipMemsetAsync(n_deferred, 0, M * 4, ctx->stream));
    PLONK_CHECK_HIP(hipMemsetAsync(redo, 0, sizeof(uint32_t), ctx->stream));  // the recovery list's counter
    PLONK_TRY(prof_begin(ctx, "msm_lookup", (double)M * (96.0 * (double)n + 64.0)));
    PLONK_LAUNCH(msm_lookup_kernel, dim3((unsigned)(M * G)), dim3(MSM_BLOCK), (size_t)MSM_BLOCK * sizeof(G1Xyzz), ctx->stream, table,
                 srs->n_points, c, W, d_scalars, n, stride, inner, outer_stride, rc, G, partial, deferred, (size_t)MSM_DEFER_CAP, n_deferred,
                 strided);
    PLONK_TRY(prof_end(ctx));
    if (G >= 8)  // few MSMs in many pieces: a wave per MSM sums the pieces in parallel
        PLONK_LAUNCH(msm_lookup_finalize_wave_kernel, dim3((unsigned)M), dim3(64), 0, ctx->stream, (const G1Xyzz*)partial, M, G, table,
                     srs->n_points, c, W, (const MsmDeferred*)deferred, (size_t)MSM_DEFER_CAP, (const uint32_t*)n_deferred, redo, d_out_xy, d_flags);
    else
        PLONK_LAUNCH(msm_lookup_finalize_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, ctx->stream, (const G1Xyzz*)partial, M, G, table,
                     srs->n_points, c, W, (const MsmDeferred*)deferred, (size_t)MSM_DEFER_CAP, (const uint32_t*)n_deferred, redo, d_out_xy, d_flags);
    PLONK_LAUNCH(msm_slow_kernel, dim3(msm_slow_grid(M)), dim3(256), 0, ctx->stream, 0, table, srs->n_points, c, W, d_scalars, n, stride, inner,
                 outer_stride, rc, (const uint32_t*)redo, (unsigned)M, d_out_xy, d_flags);
    PLONK_CHECK_HIP(hipGetLastError());
    ctx->msm_redo = redo;
    return PLONK_OK;
}

static bool msm_windows_takes_top(size_t, unsigned) { return false; }
static double msm_windows_additions(unsigned c, bool) { return (double)msm_windows_for(c); }
static const MsmTableLayout msm_windows_layout = {17,
                                                  msm_windows_takes_top,
                                                  msm_windows_additions,
                                                  msm_windows_bytes,
                                                  msm_windows_well_formed,
                                                  msm_windows_build,
                                                  msm_windows_verify,
                                                  msm_run_windows};
