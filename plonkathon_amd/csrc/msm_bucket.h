// msm_bucket.h — the bucket method (Pippenger) of msm.hip: arbitrary bases, or when no table fits.  Kernels:
// msm_sort_kernel, msm_accumulate_kernel, msm_bucket_reduce_kernel (described at the top of msm.hip).
#pragma once
#include "msm_common.h"

// Sorting.  Entry encoding: bits 0..14 base index, bit 15 sign, bits 16.. window.
// starts[m][k] (k = 0..K+1): starts[k] = number of entries in buckets 1..k-1, starts[K+1] = total.
// Scalar vector of MSM m: msm_scalar_row.
__global__ void __launch_bounds__(MSM_BLOCK) msm_sort_kernel(const Fr* scalars, size_t n, size_t stride, size_t inner,
                                                             size_t outer_stride, unsigned c, unsigned W, MsmRecode rc,
                                                             uint32_t* entries, size_t entry_stride, uint32_t* starts,
                                                             uint32_t* n_deferred, uint32_t* redo) {
    PLONK_DYN_SMEM(smem);
    __shared__ uint32_t chunk_tot[MSM_BLOCK];
    const unsigned K = 1u << (c - 1);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem);  // K + 2 counters; cnt[0] collects the zero digits
    const unsigned tid = threadIdx.x;
    const size_t m = blockIdx.x;
    const Fr* sc = msm_scalar_row(scalars, m, stride, inner, outer_stride);
    uint32_t* out = entries + m * entry_stride;
    uint32_t* st = starts + m * (size_t)(K + 2);

    for (unsigned k = tid; k < K + 2; k += MSM_BLOCK) cnt[k] = 0;
    __syncthreads();
    for (size_t i = tid; i < n; i += MSM_BLOCK) {
        uint32_t limb[10];
        msm_recode(sc, i, rc, limb);
        msm_for_each_digit(limb, c, W, [&](unsigned, int d) { atomicAdd(&cnt[d < 0 ? -d : d], 1u); });
    }
    __syncthreads();
    // exclusive scan of cnt[1..K] -> bucket starts (bucket 0 = zero digits, dropped)
    const unsigned per = (K + MSM_BLOCK - 1) / MSM_BLOCK;
    const unsigned lo = 1 + tid * per, hi = (lo + per < K + 1) ? lo + per : K + 1;
    uint32_t sum = 0;
    for (unsigned k = lo; k < hi; k++) sum += cnt[k];
    chunk_tot[tid] = sum;
    __syncthreads();
    for (unsigned off = 1; off < MSM_BLOCK; off <<= 1) {
        uint32_t v = chunk_tot[tid];
        if (tid >= off) v += chunk_tot[tid - off];
        __syncthreads();
        chunk_tot[tid] = v;
        __syncthreads();
    }
    uint32_t run = tid ? chunk_tot[tid - 1] : 0;
    for (unsigned k = lo; k < hi; k++) {
        uint32_t v = cnt[k];
        cnt[k] = run;  // becomes the scatter cursor
        st[k] = run;
        run += v;
    }
    if (tid == MSM_BLOCK - 1) {
        st[K + 1] = chunk_tot[MSM_BLOCK - 1];
        st[0] = 0;
        n_deferred[m] = 0;
        if (m == 0) redo[0] = 0;  // the recovery list's counter (msm_common.h)
    }
    __syncthreads();
    for (size_t i = tid; i < n; i += MSM_BLOCK) {
        uint32_t limb[10];
        msm_recode(sc, i, rc, limb);
        msm_for_each_digit(limb, c, W, [&](unsigned w, int d) {
            if (d) {
                uint32_t pos = atomicAdd(&cnt[d < 0 ? -d : d], 1u);
                out[pos] = (uint32_t)i | (d < 0 ? 0x8000u : 0u) | (w << 16);
            }
        });
    }
}

// ------------------------------------------------------------------------------------------------
// Entries per accumulate lane when E sorted entries are cut into `lanes` equal flat ranges (multiple of 4:
// the entry list is read with 16-byte loads).  Used identically by the two kernels below.
PLONK_HD uint32_t msm_lane_span(uint32_t E, uint32_t lanes) {
    uint32_t per = (E + lanes - 1) / lanes;
    per = (per + 3) & ~3u;
    return per ? per : 4;
}

// Lane t (0 .. 256*G-1 within its MSM) sums its flat range [t*per, (t+1)*per) of the sorted entry list,
// walking from the top entry down.  Whenever the walk leaves a bucket the partial sum of that bucket is
// stored ("piece") and the accumulator restarts: no weighting, no cross-lane reduction, and a bucket
// boundary costs eight 16-byte stores instead of a group addition, so lanes of a wave that cross
// boundaries at different steps do not serialise anything expensive.  Piece slot: t + k - 1 — lanes and
// the buckets they touch are both monotone, so the slot is unique, and msm_bucket_reduce_kernel can
// recompute which lanes touched bucket k from the bucket starts alone.
__global__ void __launch_bounds__(MSM_BLOCK, MSM_ACC_WAVES) msm_accumulate_kernel(const G1Affine* table, size_t table_n,
                                                                   const uint32_t* entries, size_t entry_stride,
                                                                   const uint32_t* starts, unsigned c, unsigned G,
                                                                   G1Xyzz* pieces, size_t piece_stride,
                                                                   MsmDeferred* deferred, uint32_t* n_deferred) {
    PLONK_DYN_SMEM(smem);
    const unsigned K = 1u << (c - 1);
    const unsigned m = blockIdx.x / G, g = blockIdx.x % G;
    const unsigned tid = threadIdx.x;
    uint32_t* st = reinterpret_cast<uint32_t*>(smem);  // K + 2 bucket starts
    const uint32_t* gst = starts + (size_t)m * (K + 2);
    for (unsigned k = tid; k < K + 2; k += MSM_BLOCK) st[k] = gst[k];
    __syncthreads();
    const uint32_t E = st[K + 1];
    const uint32_t* ent = entries + (size_t)m * entry_stride;
    const uint32_t per = msm_lane_span(E, G * MSM_BLOCK);
    const uint32_t t = g * MSM_BLOCK + tid;
    const uint64_t lo64 = (uint64_t)t * per;
    if (lo64 >= E) return;
    const uint32_t lo = (uint32_t)lo64;
    const uint32_t hi = (lo64 + per < E) ? (uint32_t)(lo64 + per) : E;

    // bucket of the top entry: largest k in [1, K] with st[k] <= hi - 1
    unsigned a = 1, b = K;
    while (a < b) {
        unsigned mid = (a + b + 1) >> 1;
        if (st[mid] <= hi - 1) a = mid;
        else b = mid - 1;
    }
    unsigned k = a;
    G1Xyzz* out = pieces + (size_t)m * piece_stride + t - 1;  // out[k] = slot t + k - 1
    // Accumulator kept as 9 signed 29-bit limbs with lazy reductions (fpl.h / g1l_madd_fast): the same ~1550
    // multiplier instructions per mixed addition as the packed canonical form but ~3x fewer of everything
    // else.  The rare steps the fast formulas cannot take (the accumulator equals +-the table point, i.e.
    // duplicate bases) are not resolved here — a call or an inlined general addition in this loop costs
    // 25 % of its speed — they are appended to the MSM's deferred list with their bucket, and
    // msm_bucket_reduce_kernel adds them to that bucket with the general formulas.
    G1XyzzL run = g1l_identity();
    auto flush = [&](unsigned kk) {
        out[kk] = g1l_to_piece(run);
        run.inf = true;
    };
    auto accumulate = [&](const Fq& x, const Fq& y, uint32_t en) {
        if (!g1l_madd_fast(run, x, y, (en & 0x8000u) != 0) && !(fp_is_zero(x) && fp_is_zero(y))) {
            const uint32_t slot = atomicAdd(n_deferred + m, 1u);
            if (slot < MSM_DEFER_CAP) deferred[(size_t)m * MSM_DEFER_CAP + slot] = MsmDeferred{k, en};
        }
    };
    auto step = [&](uint32_t e, uint32_t en) {
        if (e >= hi || e < lo) return;
        if (e < st[k]) {  // left bucket k: its partial sum is complete
            flush(k);
            do k--;
            while (e < st[k]);
        }
        const G1Affine* src = table + (size_t)(en >> 16) * table_n + (en & 0x7fffu);
        const Fq x = fp_load(&src->x), y = fp_load(&src->y);
        accumulate(x, y, en);
    };
    for (uint32_t base = (hi - 1) & ~3u;; base -= 4) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(ent + base);
        step(base + 3, q.w);
        step(base + 2, q.z);
        step(base + 1, q.y);
        step(base, q.x);
        if (base <= lo) break;
    }
    flush(k);
}

// sum_k k * B_k for one MSM from the pieces.  Lane l owns the buckets (l*pb, (l+1)*pb]: walking them from
// the top, run += (pieces of bucket k), tot += run, gives tot = sum (k - l*pb) B_k and run = sum B_k, so
// the lane's share is tot + (l*pb) * run; the shares are tree-reduced through LDS.  Every lane adds into
// tot once per bucket, so the wave stays converged; only the (1-3 piece) inner loop varies.
__global__ void __launch_bounds__(256) msm_bucket_reduce_kernel(const uint32_t* starts, unsigned c, unsigned acc_lanes,
                                                                 const G1Xyzz* pieces, size_t piece_stride,
                                                                 const G1Affine* table, size_t table_n, const MsmDeferred* deferred,
                                                                 size_t deferred_stride, const uint32_t* n_deferred, uint32_t* redo,
                                                                 unsigned M, Fq* out_xy, uint8_t* flags) {
    PLONK_DYN_SMEM(smem);
    G1Xyzz* red = reinterpret_cast<G1Xyzz*>(smem);
    const unsigned K = 1u << (c - 1);
    const unsigned m = blockIdx.x, tid = threadIdx.x, nl = blockDim.x;
    const uint32_t* gst = starts + (size_t)m * (K + 2);
    const uint32_t per = msm_lane_span(gst[K + 1], acc_lanes);
    const unsigned pb = (K + nl - 1) / nl;
    const unsigned b_lo = tid * pb < K ? tid * pb : K;
    const unsigned b_hi = b_lo + pb < K ? b_lo + pb : K;
    const G1Xyzz* pc = pieces + (size_t)m * piece_stride - 1;  // pc[t + k] = piece of lane t for bucket k
    G1Xyzz run = g1_xyzz_identity(), tot = g1_xyzz_identity();
    const MsmDeferred* dfr = deferred + (size_t)m * deferred_stride;
    // additions msm_accumulate_kernel left to the general formulas (normally 0); past the cap the MSM is redone by
    // msm_slow_kernel, which overwrites this kernel's output
    const uint32_t n_dfr = n_deferred[m] < MSM_DEFER_CAP ? n_deferred[m] : MSM_DEFER_CAP;
    if (tid == 0 && n_deferred[m] > MSM_DEFER_CAP) msm_redo_append(redo, m, M);  // (the accumulation is over: the count is final; one lane per MSM)
    uint32_t s_hi = gst[b_hi + 1];
    for (unsigned k = b_hi; k > b_lo; k--) {
        const uint32_t s_lo = gst[k];
        if (s_hi > s_lo) {
            const uint32_t t_last = (s_hi - 1) / per;
            for (uint32_t t = s_lo / per; t <= t_last; t++) g1_add(run, g1_piece_load(pc + (size_t)t + k));
            for (uint32_t i = 0; i < n_dfr; i++) {
                const MsmDeferred d = dfr[i];
                if (d.bucket != k) continue;
                const G1Affine* src = table + (size_t)(d.entry >> 16) * table_n + (d.entry & 0x7fffu);
                G1Affine pt;
                pt.x = fp_load(&src->x);
                pt.y = fp_load(&src->y);
                if (d.entry & 0x8000u) pt.y = fp_neg(pt.y);
                g1_madd(run, pt);
            }
        }
        g1_add(tot, run);
        s_hi = s_lo;
    }
    // The buckets of lane l weigh b_lo(l) = l pb more than its local walk gave them: sum_l l pb run_l = pb sum_{j >= 1} S_j with
    // S_j = sum_{l >= j} run_l — a suffix scan over the lanes (six general additions inside a wave, by cross-lane moves; wave
    // totals through LDS) and log2 pb doublings, where round 3 ran a c-bit double-and-add of (b_lo, run) per lane: c doublings
    // plus, because a wave executes every branch one of its lanes takes, c - 1 additions.
    {
        const unsigned lane = tid & 63u, wave = tid >> 6, nw = nl >> 6;
        G1Xyzz S = run;
        g1_wave_suffix_scan(S, lane);
        if (nw > 1) {
            if (lane == 0) red[wave] = S;  // lane 0 holds its wave's total
            __syncthreads();
            for (unsigned w = nw - 1; w > wave; w--) g1_add(S, red[w]);
            __syncthreads();
        }
        if (tid) {
            for (unsigned q = pb; q > 1; q >>= 1) g1_dbl(S);
            g1_add(tot, S);
        }
    }
    msm_fold_store(red, tot, tid, nl, m, out_xy, flags);
}

// srs->table = T[w][i] = 2^(c w) P_i for c-bit windows (kept until another c is asked for)
static int msm_build_table(plonk_ctx* ctx, plonk_srs* srs, unsigned c) {
    if (srs->table && srs->window_bits == c) return PLONK_OK;
    if (srs->table) {
        hipFree(srs->table);
        srs->table = nullptr;
    }
    const unsigned W = msm_windows_for(c);
    const size_t n = srs->n_points, total = n * W;
    void *tmp = nullptr, *tab = nullptr;
    if (!plonk_dev_malloc(&tmp, total * sizeof(G1Xyzz)) || !plonk_dev_malloc(&tab, total * sizeof(G1Affine))) {
        if (tmp) hipFree(tmp);
        plonk_set_error("hipMalloc of the %zu-point window table failed", total);
        return PLONK_ERR_NOMEM;
    }
    msm_window_bases(ctx, srs->bases, n, c, W, (G1Xyzz*)tmp);
    g1_batch_to_affine(ctx, (const G1Xyzz*)tmp, (G1Affine*)tab, total, 4096);
    PLONK_CHECK_HIP(hipGetLastError());
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    hipFree(tmp);
    srs->table = (G1Affine*)tab;
    srs->window_bits = c;
    srs->n_windows = W;
    return PLONK_OK;
}

// M MSMs of n scalars on c-bit windows
static int msm_run_bucket(plonk_ctx* ctx, plonk_srs* srs, unsigned c, const Fr* d_scalars, size_t n, size_t M, size_t stride, Fq* d_out_xy,
                          uint8_t* d_flags, size_t inner, size_t outer_stride) {
    PLONK_REQUIRE(n <= 32768, PLONK_ERR_ARG, "MSM size %zu > 32768 is not supported by the bucket method's entry encoding", n);
    PLONK_TRY(msm_build_table(ctx, srs, c));
    const unsigned W = srs->n_windows, K = 1u << (c - 1);
    const size_t max_entries = (size_t)W * n;
    // enough workgroups to fill 256 CUs a few times over, but no more pieces than needed (tiny MSMs: one segment is plenty)
    const unsigned G = msm_groups_per_msm(ctx, M, 16, 1024, 0.03, max_entries, 4);
    // lanes per MSM in the bucket reduction (shorter local walks vs more lanes paying the scan and the reduction): batches (G < 8)
    // take 128 — measured best with the suffix-scan weighting (profiles/r04_c_bucket_reduce_lanes_ab.jsonl: 23.3 k proofs/s against
    // 22.5 k at 64; round 3's double-and-add weighting: 22.8 k at 128) — a lone MSM cut into many workgroups (G >= 8) is latency
    // bound and takes 256.  (msm_bucket_reduce_kernel weighs a lane's run by pb = K / red_lanes through log2(pb) doublings: both are powers of two.)
    const unsigned red_lanes = G >= 8 ? 256 : 128;
    const size_t entry_stride = ((max_entries + 3) & ~(size_t)3) + 4;
    const size_t piece_stride = (size_t)G * MSM_BLOCK + K;
    MsmScratch s;
    const size_t ent_off = s.take(M * entry_stride * 4), st_off = s.take(M * (size_t)(K + 2) * 4), piece_off = s.take(M * piece_stride * sizeof(G1Xyzz));
    const size_t cnt_off = s.take(M * 4), dfr_off = s.take(M * MSM_DEFER_CAP * sizeof(MsmDeferred));  // bounded: an MSM that overflows is redone by msm_slow_kernel
    const size_t redo_off = s.take(msm_redo_words(M) * sizeof(uint32_t));  // the recovery list: a part of its own, a counter and M indices
    PLONK_TRY(ctx_scratch(ctx, 1, s.total, (void**)&s.base));
    uint32_t *entries = s.at<uint32_t>(ent_off), *starts = s.at<uint32_t>(st_off), *n_deferred = s.at<uint32_t>(cnt_off), *redo = s.at<uint32_t>(redo_off);
    G1Xyzz* pieces = s.at<G1Xyzz>(piece_off);
    MsmDeferred* deferred = s.at<MsmDeferred>(dfr_off);

    MsmRecode rc;
    msm_recode_constant(c, W, &rc);
    const size_t sort_lds = (size_t)(K + 2) * 4;
    if (!ctx->msm_attr_set) {  // a per-device attribute: tracked per context, not per process
        PLONK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_sort_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)(128 * 1024)));
        ctx->msm_attr_set = true;
    }
    PLONK_TRY(prof_begin(ctx, "msm_sort", (double)M * 32.0 * (double)n));
    PLONK_LAUNCH(msm_sort_kernel, dim3((unsigned)M), dim3(MSM_BLOCK), sort_lds, ctx->stream, d_scalars, n, stride, inner, outer_stride, c, W, rc,
                 entries, entry_stride, starts, n_deferred, redo);
    PLONK_TRY(prof_end(ctx));
    // algorithmic bytes of an MSM of size n: (64 + 32) * n + 64   
    PLONK_TRY(prof_begin(ctx, "msm_accumulate", (double)M * (96.0 * (double)n + 64.0)));
    PLONK_LAUNCH(msm_accumulate_kernel, dim3((unsigned)(M * G)), dim3(MSM_BLOCK), sort_lds, ctx->stream,
                 (const G1Affine*)srs->table, srs->n_points, (const uint32_t*)entries, entry_stride,
                 (const uint32_t*)starts, c, G, pieces, piece_stride, deferred, n_deferred);
    PLONK_TRY(prof_end(ctx));
    PLONK_TRY(prof_begin(ctx, "msm_bucket_reduce", (double)M * (double)piece_stride * sizeof(G1Xyzz)));
    PLONK_LAUNCH(msm_bucket_reduce_kernel, dim3((unsigned)M), dim3(red_lanes), (size_t)red_lanes * sizeof(G1Xyzz), ctx->stream,
                 (const uint32_t*)starts, c, G * MSM_BLOCK, (const G1Xyzz*)pieces, piece_stride,
                 (const G1Affine*)srs->table, srs->n_points, (const MsmDeferred*)deferred, (size_t)MSM_DEFER_CAP, (const uint32_t*)n_deferred, redo,
                 (unsigned)M, d_out_xy, d_flags);
    PLONK_TRY(prof_end(ctx));
    PLONK_LAUNCH(msm_slow_kernel, dim3(msm_slow_grid(M)), dim3(256), 0, ctx->stream, 1, (const G1Affine*)srs->table, srs->n_points, c, W,
                 d_scalars, n, stride, inner, outer_stride, rc, (const uint32_t*)redo, (unsigned)M, d_out_xy, d_flags);
    PLONK_CHECK_HIP(hipGetLastError());
    ctx->msm_redo = redo;
    return PLONK_OK;
}
