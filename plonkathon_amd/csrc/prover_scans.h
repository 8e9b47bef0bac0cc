// prover_scans.h — the three per-proof scans of the lock-step prover (included by prover.hip only): the permutation grand
// product of round 2, the evaluations of round 4 and the divisions by X - x0 of round 5.  Each family has a one-workgroup form
// (one workgroup per proof: S = 1) and a segmented form (below); both are built from the device steps of this file, every step
// written once, and the host reaches them through scan_grand_product / scan_evaluations / scan_divisions, which take S.
#pragma once
#include "prover.h"
#include "wave.h"  // wave_lane_xor: the evaluations' sums inside a wave

#define SCAN_THREADS 256  // lanes of every workgroup in this file

// ------------------------------------------------------------------------------------------------
// A lane's rows [lo, hi): `per` consecutive rows per lane.
struct LaneRange { size_t lo, hi, per; };
// one workgroup over all n rows (a lane past the end has lo >= hi: no rows)
PLONK_DEV LaneRange block_lane_range(size_t n, unsigned tid) {
    LaneRange r;
    r.per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    r.lo = tid * r.per;
    r.hi = (r.lo + r.per < n) ? r.lo + r.per : n;
    return r;
}
// segment `seg` of S.  n and S are powers of two, so a segment's L = n / S rows fall on its 256 lanes as `per` = max(L / 256, 1)
// rows each: lanes below min(L, 256) hold exactly `per` rows, the others none (lo == hi), and an empty lane carries the scan's
// neutral element.
PLONK_DEV LaneRange seg_lane_range(size_t n, unsigned S, unsigned seg, unsigned tid) {
    const size_t L = n / S, per = (L + SCAN_THREADS - 1) / SCAN_THREADS, s_lo = (size_t)seg * L, s_hi = s_lo + L;
    LaneRange r;
    r.per = per;
    r.lo = s_lo + (size_t)tid * per < s_hi ? s_lo + (size_t)tid * per : s_hi;
    r.hi = r.lo + per < s_hi ? r.lo + per : s_hi;
    return r;
}

// ------------------------------------------------------------------------------------------------
// Round 2 (prover.py:121-152): the permutation grand product.
//   num_i = (A_i + b w^i + g)(B_i + 2 b w^i + g)(C_i + 3 b w^i + g)
//   den_i = (A_i + b S1_i + g)(B_i + b S2_i + g)(C_i + b S3_i + g)
//   Z_0 = 1, Z_{i+1} = Z_i num_i / den_i
// With PN_i = prod_{j<i} num_j and SD_i = prod_{j>=i} den_j:  Z_i = PN_i * SD_i / prod_j den_j, so the
// whole column costs two block scans and ONE field inversion.  A zero denominator factor is skipped
// in the scans and zeroes the ratio it belongs to (py_ecc: x / 0 == 0).
// Inputs by pointer: proof b's columns at abc[k] + b n, the permutation polynomials sig[k] shared.  The challenges come
// from the proofs' transcript states (st, the lock-step prover) or, st == null, from `direct` (plonk_fr_grand_product).
// A table of circuits (cid != null): proof b's permutation polynomials are sig[k] + cid[b] * sig_stride.
struct GrandProductIn { const Fr* abc[3]; const Fr* sig[3]; const uint32_t* cid; size_t sig_stride; };
struct GpProducts { Fr n, d; };

// The factors of proof b's rows [r.lo, r.hi), once, into NUM / DEN (this proof's; a lane only ever touches its own chunk); the
// lane's two products.
PLONK_DEV GpProducts gp_chunk_factors(const GrandProductIn& in, const Fr* roots, const Fr& beta, const Fr& gamma, size_t b, size_t n,
                                      const LaneRange& r, Fr* NUM, Fr* DEN) {
    const Fr *A = in.abc[0] + b * n, *Bv = in.abc[1] + b * n, *C = in.abc[2] + b * n;
    const size_t so = in.cid ? (size_t)in.cid[b] * in.sig_stride : 0;
    const Fr *S1 = in.sig[0] + so, *S2 = in.sig[1] + so, *S3 = in.sig[2] + so;
    const Fr one = fp_one<FrParams>();
    GpProducts p = {one, one};
    for (size_t i = r.lo; i < r.hi; i++) {
        Fr a = fp_load(A + i), bb = fp_load(Bv + i), c = fp_load(C + i);
        Fr bw = fp_mul(beta, fp_load(roots + i));
        Fr ag = fp_add(a, gamma), bg = fp_add(bb, gamma), cg = fp_add(c, gamma);
        Fr num = fp_mul(fp_mul(fp_add(ag, bw), fp_add(bg, fp_dbl(bw))), fp_add(cg, fp_mul3(bw)));
        Fr den = fp_mul(fp_mul(fp_add(ag, fp_mul(beta, fp_load(S1 + i))), fp_add(bg, fp_mul(beta, fp_load(S2 + i)))),
                        fp_add(cg, fp_mul(beta, fp_load(S3 + i))));
        if (fp_is_zero(den)) {  // ratio num/0 == 0 (py_ecc): the factor leaves the denominator products
            num = fp_zero<FrParams>();
            den = one;
        }
        fp_store(NUM + i, num);
        fp_store(DEN + i, den);
        p.d = fp_mul(p.d, den);
        p.n = fp_mul(p.n, num);
    }
    return p;
}

// The lanes' products are in sc_n / sc_d (stored, and a barrier passed): inclusive prefix scan of sc_n (Hillis-Steele), inclusive
// suffix scan of sc_d.
PLONK_DEV void block_scan_products(Fr* sc_n, Fr* sc_d, unsigned tid) {
    for (unsigned off = 1; off < SCAN_THREADS; off <<= 1) {
        Fr vn = sc_n[tid], vd = sc_d[tid];
        if (tid >= off) vn = fp_mul(vn, sc_n[tid - off]);
        if (tid + off < SCAN_THREADS) vd = fp_mul(vd, sc_d[tid + off]);
        __syncthreads();
        sc_n[tid] = vn;
        sc_d[tid] = vd;
        __syncthreads();
    }
}

// The lane's rows, with run_n = prod of num before them and after_d = prod of den after them: (backwards) DEN[k] <- prod_{j >= k}
// den_j, then Z_i = PN_i * SD_i * tot_inv.  Returns prod of num up to the end of the rows.
PLONK_DEV Fr gp_chunk_apply(const Fr* NUM, Fr* DEN, Fr* Z, const LaneRange& r, Fr run_n, Fr after_d, const Fr& tinv) {
    for (size_t k = r.hi; k-- > r.lo;) {
        after_d = fp_mul(after_d, fp_load(DEN + k));
        fp_store(DEN + k, after_d);
    }
    for (size_t i = r.lo; i < r.hi; i++) {
        fp_store(Z + i, fp_mul(fp_mul(run_n, fp_load(DEN + i)), tinv));
        run_n = fp_mul(run_n, fp_load(NUM + i));
    }
    return run_n;
}

// One workgroup per proof.
__global__ void PLONK_BESIDE_ACC(SCAN_THREADS, 4) grand_product_kernel(GrandProductIn in, const Fr* roots, const ProofState* st,
                                                                     RoundChallenges direct, size_t n, Fr* z_out,
                                                                     uint32_t* closes, Fr* num_buf, Fr* den_buf) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc_n[SCAN_THREADS], sc_d[SCAN_THREADS];
    __shared__ Fr tot_inv;
    const size_t b = blockIdx.x;
    const unsigned tid = threadIdx.x;
    const Fr beta = st ? st[b].beta : direct.beta, gamma = st ? st[b].gamma : direct.gamma;
    Fr *NUM = num_buf + b * n, *DEN = den_buf + b * n;
    const LaneRange r = block_lane_range(n, tid);
    const Fr one = fp_one<FrParams>();
    const GpProducts p = gp_chunk_factors(in, roots, beta, gamma, b, n, r, NUM, DEN);
    sc_n[tid] = p.n;
    sc_d[tid] = p.d;
    __syncthreads();
    block_scan_products(sc_n, sc_d, tid);
    if (tid == 0) tot_inv = fp_inv(sc_d[0]);  // product of all non-zero denominators
    __syncthreads();
    const Fr run_n = tid ? sc_n[tid - 1] : one;                       // prod of num before this lane's chunk
    const Fr after_d = (tid + 1 < SCAN_THREADS) ? sc_d[tid + 1] : one;  // prod of den after this lane's chunk
    const Fr tinv = tot_inv;
    const Fr all_n = gp_chunk_apply(NUM, DEN, z_out + b * n, r, run_n, after_d, tinv);
    // prover.py:132 `assert Z_values.pop() == 1`: the full product of ratios must close to one
    if (tid == SCAN_THREADS - 1) closes[b] = fp_eq(fp_mul(all_n, tinv), fp_one<FrParams>()) ? 1u : 0u;
}

// ------------------------------------------------------------------------------------------------
// Round 4 (prover.py:228-239): evaluate coefficient forms at zeta (and Z at zeta*w): lane t Horner-evaluates its chunk of each
// polynomial, scales by x^(chunk start) and the workgroup adds the lanes' values up.  polys: Ac, Bc, Cc, S1c, S2c at zeta; Zc at
// zeta*w; PIc at zeta.  fixed_coef: [K][8][n], proof b is of circuit cid[b] (cid == null: circuit 0).
//
// The lane walks its rows once per PASS, a pass holding the chains of one evaluation point that fit in the 96 registers free
// beside the MSM accumulation (PLONK_BESIDE_ACC): {Z} at zeta*w, then {A, B, C} and {S1, S2, PI} at zeta.  Seven chains at once were 63
// accumulator registers beside the multiplication's temporaries (242 VGPRs).  Each sum is then reduced on its packed canonical
// value: inside the wave through wave_lane_xor (six steps, no LDS, no barrier), and the waves' values through wsum[wave][sum] —
// 896 bytes of LDS and one barrier where the tree over red[7][256] took 56 KB and nine.  Field addition is exact and every value
// canonical, so the order of the additions changes no bit of a sum.
#define EVAL_WAVES (SCAN_THREADS / 64)
struct EvalWaveSums { Fr v[EVAL_WAVES][NEVAL]; };

// all 64 lanes of the wave must call this together: afterwards every lane holds the wave's sum
PLONK_DEV Fr fr_wave_sum(Fr v, unsigned lane) {
    const auto step = [&](auto M_) PLONK_LAMBDA_INLINE {
        constexpr unsigned MASK = decltype(M_)::value;
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.v[i] = wave_lane_xor<MASK>(v.v[i], lane);
        v = fp_add(v, o);
    };
    step(WaveIdx<32>{});
    step(WaveIdx<16>{});
    step(WaveIdx<8>{});
    step(WaveIdx<4>{});
    step(WaveIdx<2>{});
    step(WaveIdx<1>{});
    return v;
}

// One pass: the chains polys[K0 .. K0 + NK) over the lane's rows at the point x (limbs xl, in scalar registers), scaled by
// shift = x^(chunk start); the wave's sum of chain K0 + k goes to ws.v[wave][slot[K0 + k]].
template <unsigned K0, unsigned NK>
PLONK_DEV void eval_pass(EvalWaveSums& ws, const Fr* const (&polys)[NEVAL], const unsigned (&slot)[NEVAL], const FpL<FrParams>& xl, const Fr& shift,
                         const LaneRange& r, unsigned tid) {
    typedef FpL<FrParams> L;
    // Horner on lazy limbs (fpl.h), the pass's chains side by side: acc x is normalised in (-m, 2m), plus a coefficient it is a
    // sum of two — a valid multiplicand as it stands
    L acc[NK];
    wave_for<NK>([&](auto K_) { acc[decltype(K_)::value] = fpl_zero<FrParams>(); });
#pragma unroll 1
    for (size_t i = r.hi; i-- > r.lo;)
        wave_for<NK>([&](auto K_) {
            constexpr unsigned k = decltype(K_)::value;
            acc[k] = fpl_add(fpl_mul(acc[k], xl), fpl_from_fp(fp_load(polys[K0 + k] + i)));  // (-m, 3m), limbs < 2^30
        });
    const L sh = fpl_from_fp(shift);
    const unsigned wave = tid / 64, lane = tid % 64;
    wave_for<NK>([&](auto K_) {
        constexpr unsigned k = decltype(K_)::value;
        const Fr mine = r.lo < r.hi ? fpl_pack_canonical(fpl_mul(acc[k], sh)) : fp_zero<FrParams>();  // an empty lane adds zero
        const Fr sum = fr_wave_sum(mine, lane);
        if (lane == 0) ws.v[wave][slot[K0 + k]] = sum;
    });
    PLONK_SCHED_FENCE();  // the next pass starts with this one's registers free
}

// Returns, in lane p < NEVAL, sum p over the workgroup's rows (the other lanes: nothing of use).  All lanes must call it.
PLONK_DEV Fr eval_chunk_sums(EvalWaveSums& ws, const Fr* coef, const Fr* fixed_coef, const uint32_t* cid, const Fr& zeta, const Fr& zeta_w,
                             size_t b, size_t n, size_t B, const LaneRange& r, unsigned tid) {
    if (cid) fixed_coef += (size_t)cid[b] * FX_COUNT * n;
    // in pass order; slot[k]: the place of chain k among the seven sums (Zc is sum 5, PIc sum 6)
    const Fr* const polys[NEVAL] = {coef + (4 * B + b) * n, coef + (0 * B + b) * n, coef + (1 * B + b) * n, coef + (2 * B + b) * n,
                                    fixed_coef + FX_S1 * n,  fixed_coef + FX_S2 * n,  coef + (3 * B + b) * n};
    const unsigned slot[NEVAL] = {5, 0, 1, 2, 3, 4, 6};
    // x^(chunk start) once per evaluation point and lane, before the passes: not once per polynomial, nor once per pass
    const Fr shift_z = fp_pow_u64(zeta, (uint64_t)r.lo), shift_zw = fp_pow_u64(zeta_w, (uint64_t)r.lo);
    // Zc first: its chunk power is then out of the way of the two passes of three chains
    eval_pass<0, 1>(ws, polys, slot, fpl_from_fp_uniform(zeta_w), shift_zw, r, tid);
    eval_pass<1, 3>(ws, polys, slot, fpl_from_fp_uniform(zeta), shift_z, r, tid);
    eval_pass<4, 3>(ws, polys, slot, fpl_from_fp_uniform(zeta), shift_z, r, tid);
    __syncthreads();
    Fr total = fp_zero<FrParams>();
    if (tid < NEVAL) {
        total = ws.v[0][tid];
        for (unsigned wv = 1; wv < EVAL_WAVES; wv++) total = fp_add(total, ws.v[wv][tid]);
    }
    return total;
}

// One workgroup per proof.
__global__ void PLONK_BESIDE_ACC(SCAN_THREADS, 8) eval_kernel(const Fr* coef, const Fr* fixed_coef, const uint32_t* cid, Fr w, ProofState* st,
                                                            size_t n, size_t B) {
    PLONK_SHORT_KERNEL();
    __shared__ EvalWaveSums ws;
    const size_t b = blockIdx.x;
    const unsigned tid = threadIdx.x;
    const Fr zeta = st[b].zeta, zeta_w = fp_mul(zeta, w);
    const Fr total = eval_chunk_sums(ws, coef, fixed_coef, cid, zeta, zeta_w, b, n, B, block_lane_range(n, tid), tid);
    if (tid < NEVAL) st[b].evals[tid] = total;
}

// ------------------------------------------------------------------------------------------------
// Round 5: q(X) = (p(X) - p(x0)) / (X - x0): q_{n-1} = 0, q_{i-1} = p_i + x0 q_i.  Lane t owns a chunk, the cross-chunk
// carries are a suffix scan under (a, m) o (b, m') = (a + m b, m m').
// x0 of proof b: zeta, or (which) zeta * w for W_zw (prover.py:292-297)
PLONK_DEV Fr divide_point(const ProofState* st, size_t b, const Fr& w, int which) {
    Fr x0 = st[b].zeta;
    if (which) x0 = fp_mul(x0, w);
    return x0;
}
// the lane's Horner value h = sum_{i in chunk} p_i x0^(i - lo)
PLONK_DEV Fr divide_chunk_horner(const Fr* p, const LaneRange& r, const Fr& x0) {
    Fr h = fp_zero<FrParams>();
    for (size_t i = r.hi; i-- > r.lo;) h = fp_add(fp_mul(h, x0), fp_load(p + i));
    return h;
}
// The lanes' h are in sc (stored, and a barrier passed); m = x0^per.  After the suffix scan sc[t] = sum_{u >= t} h_u x0^((u - t) per).
PLONK_DEV void block_suffix_scan_affine(Fr* sc, unsigned tid, Fr m) {
    for (unsigned off = 1; off < SCAN_THREADS; off <<= 1) {
        Fr vv = sc[tid];
        if (tid + off < SCAN_THREADS) vv = fp_add(vv, fp_mul(m, sc[tid + off]));
        __syncthreads();
        sc[tid] = vv;
        m = fp_sqr(m);
        __syncthreads();
    }
}
// the lane's rows of the quotient from the carry into its chunk: q = q_{hi-1} = sum_{j >= hi} p_j x0^(j - hi)
PLONK_DEV void divide_chunk_writeback(const Fr* p, Fr* out, const LaneRange& r, const Fr& x0, Fr q) {
    for (size_t i = r.hi; i-- > r.lo;) {
        fp_store(out + i, q);                       // q_i
        q = fp_add(fp_load(p + i), fp_mul(x0, q));  // q_{i-1} = p_i + x0 q_i
    }
}

// One workgroup per proof.
__global__ void __launch_bounds__(SCAN_THREADS) divide_linear_kernel(const Fr* p_in, size_t in_stride, int which,
                                                                     Fr w, const ProofState* st, size_t n, Fr* q_out) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc[SCAN_THREADS];
    const size_t b = blockIdx.x;
    const unsigned tid = threadIdx.x;
    const Fr x0 = divide_point(st, b, w, which);
    const Fr* p = p_in + b * in_stride;
    const LaneRange r = block_lane_range(n, tid);
    sc[tid] = divide_chunk_horner(p, r, x0);
    __syncthreads();
    block_suffix_scan_affine(sc, tid, fp_pow_u64(x0, (uint64_t)r.per));
    // the contribution of all higher chunks is sc[t + 1]
    divide_chunk_writeback(p, q_out + b * n, r, x0, (tid + 1 < SCAN_THREADS) ? sc[tid + 1] : fp_zero<FrParams>());
}

// ------------------------------------------------------------------------------------------------
// Segmented forms of the three scans for batches too small to fill the chip with one workgroup per proof.  A proof's n rows are
// cut into S equal segments (S a power of two, 2 <= S <= 256, n / S >= 16) and every scan becomes three launches, or two, on the
// prover's stream: per-segment work on a grid of (S, B) workgroups, a small per-proof launch that turns the S segment totals into
// carries, and a second (S, B) launch that applies them.  The launches are ordered by the stream alone: no workgroup ever waits
// for another inside a kernel.  Everything is a canonical residue of an associative operation, and the steps are the ones the
// one-workgroup kernels above (S = 1) are made of, so the results are the same bits.

// Grand product, launch 1 of 3, grid (S, B): the factors of the segment's rows into num_buf / den_buf, and the segment's two
// products into seg_n / seg_d [B][S].
__global__ void __launch_bounds__(SCAN_THREADS) gp_seg_factors_kernel(GrandProductIn in, const Fr* roots, const ProofState* st,
                                                                      RoundChallenges direct, size_t n, Fr* num_buf, Fr* den_buf,
                                                                      Fr* seg_n, Fr* seg_d) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc_n[SCAN_THREADS], sc_d[SCAN_THREADS];
    const size_t b = blockIdx.y;
    const unsigned tid = threadIdx.x, S = gridDim.x;
    const Fr beta = st ? st[b].beta : direct.beta, gamma = st ? st[b].gamma : direct.gamma;
    const GpProducts p = gp_chunk_factors(in, roots, beta, gamma, b, n, seg_lane_range(n, S, blockIdx.x, tid), num_buf + b * n, den_buf + b * n);
    sc_n[tid] = p.n;
    sc_d[tid] = p.d;
    __syncthreads();
    for (unsigned s = SCAN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sc_n[tid] = fp_mul(sc_n[tid], sc_n[tid + s]);
            sc_d[tid] = fp_mul(sc_d[tid], sc_d[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        fp_store(seg_n + b * S + blockIdx.x, sc_n[0]);
        fp_store(seg_d + b * S + blockIdx.x, sc_d[0]);
    }
}

// Launch 2 of 3, one workgroup per proof, lane s = segment s: seg_n[s] <- prod of the numerators BEFORE segment s, seg_d[s] <-
// prod of the denominators AFTER it, tot_inv[b] = the proof's one inversion, closes[b].
__global__ void __launch_bounds__(SCAN_THREADS) gp_seg_carries_kernel(unsigned S, Fr* seg_n, Fr* seg_d, Fr* tot_inv, uint32_t* closes) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc_n[SCAN_THREADS], sc_d[SCAN_THREADS];
    const size_t b = blockIdx.x;
    const unsigned tid = threadIdx.x;
    const Fr one = fp_one<FrParams>();
    sc_n[tid] = tid < S ? fp_load(seg_n + b * S + tid) : one;
    sc_d[tid] = tid < S ? fp_load(seg_d + b * S + tid) : one;
    __syncthreads();
    block_scan_products(sc_n, sc_d, tid);
    if (tid < S) {
        fp_store(seg_n + b * S + tid, tid ? sc_n[tid - 1] : one);
        fp_store(seg_d + b * S + tid, tid + 1 < SCAN_THREADS ? sc_d[tid + 1] : one);
    }
    if (tid == 0) {
        const Fr tinv = fp_inv(sc_d[0]);  // product of all non-zero denominators
        fp_store(tot_inv + b, tinv);
        closes[b] = fp_eq(fp_mul(sc_n[SCAN_THREADS - 1], tinv), one) ? 1u : 0u;  // prover.py:132
    }
}

// Launch 3 of 3, grid (S, B): the lanes' products of the stored factors, scanned and seeded with the segment's carries.
__global__ void __launch_bounds__(SCAN_THREADS) gp_seg_apply_kernel(size_t n, const Fr* seg_n, const Fr* seg_d, const Fr* tot_inv,
                                                                    const Fr* num_buf, Fr* den_buf, Fr* z_out) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc_n[SCAN_THREADS], sc_d[SCAN_THREADS];
    const size_t b = blockIdx.y;
    const unsigned tid = threadIdx.x, S = gridDim.x;
    const Fr* NUM = num_buf + b * n;
    Fr* DEN = den_buf + b * n;
    const LaneRange r = seg_lane_range(n, S, blockIdx.x, tid);
    const Fr one = fp_one<FrParams>();
    Fr pn = one, pd = one;
    for (size_t i = r.lo; i < r.hi; i++) {
        pn = fp_mul(pn, fp_load(NUM + i));
        pd = fp_mul(pd, fp_load(DEN + i));
    }
    sc_n[tid] = pn;
    sc_d[tid] = pd;
    __syncthreads();
    block_scan_products(sc_n, sc_d, tid);
    Fr run_n = fp_load(seg_n + b * S + blockIdx.x), after_d = fp_load(seg_d + b * S + blockIdx.x);
    if (tid) run_n = fp_mul(run_n, sc_n[tid - 1]);
    if (tid + 1 < SCAN_THREADS) after_d = fp_mul(after_d, sc_d[tid + 1]);
    gp_chunk_apply(NUM, DEN, z_out + b * n, r, run_n, after_d, fp_load(tot_inv + b));
}

// Evaluations, launch 1 of 2, grid (S, B): the blocked Horner over the segment's rows, every lane's chains scaled by x^(global
// chunk start); the segment's seven sums go to part[b][s][NEVAL].
__global__ void PLONK_BESIDE_ACC(SCAN_THREADS, 8) eval_seg_kernel(const Fr* coef, const Fr* fixed_coef, const uint32_t* cid, Fr w, const ProofState* st,
                                                                size_t n, size_t B, Fr* part) {
    PLONK_SHORT_KERNEL();
    __shared__ EvalWaveSums ws;
    const size_t b = blockIdx.y;
    const unsigned tid = threadIdx.x, S = gridDim.x;
    const Fr zeta = st[b].zeta, zeta_w = fp_mul(zeta, w);
    const Fr total = eval_chunk_sums(ws, coef, fixed_coef, cid, zeta, zeta_w, b, n, B, seg_lane_range(n, S, blockIdx.x, tid), tid);
    if (tid < NEVAL) fp_store(part + (b * S + blockIdx.x) * NEVAL + tid, total);
}

// Launch 2 of 2, one workgroup per proof: lane group p (32 lanes) adds the S partial sums of evaluation p into st[b].evals[p].
__global__ void __launch_bounds__(SCAN_THREADS) eval_seg_finish_kernel(const Fr* part, unsigned S, ProofState* st) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr red[SCAN_THREADS];
    const size_t b = blockIdx.x;
    const unsigned tid = threadIdx.x, p = tid / 32, l = tid % 32;
    Fr acc = fp_zero<FrParams>();
    if (p < NEVAL)
        for (unsigned s = l; s < S; s += 32) acc = fp_add(acc, fp_load(part + (b * S + s) * NEVAL + p));
    red[tid] = acc;
    __syncthreads();
    for (unsigned s = 16; s > 0; s >>= 1) {
        if (l < s) red[tid] = fp_add(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (l == 0 && p < NEVAL) st[b].evals[p] = red[tid];
}

// Division by X - x0, both openings at once: blockIdx.z = 0 divides p_in[0] by X - zeta, 1 divides p_in[1] by X - zeta w.
struct DivideIn { const Fr* p_in[2]; Fr* q_out[2]; };
// Launch 1 of 3, grid (S, B, 2): the segment's Horner value H_s = sum_{i in segment} p_i x0^(i - segment start) into seg_h[z][b][s].
__global__ void __launch_bounds__(SCAN_THREADS) divide_seg_horner_kernel(DivideIn in, Fr w, const ProofState* st, size_t n, Fr* seg_h) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc[SCAN_THREADS];
    const size_t b = blockIdx.y, B = gridDim.y;
    const unsigned tid = threadIdx.x, S = gridDim.x, z = blockIdx.z;
    const Fr x0 = divide_point(st, b, w, z);
    const LaneRange r = seg_lane_range(n, S, blockIdx.x, tid);
    sc[tid] = divide_chunk_horner(in.p_in[z] + b * n, r, x0);
    __syncthreads();
    Fr m = fp_pow_u64(x0, (uint64_t)r.per);  // x0^(per * off)
    for (unsigned off = 1; off < SCAN_THREADS; off <<= 1) {
        if ((tid & (2 * off - 1)) == 0) sc[tid] = fp_add(sc[tid], fp_mul(m, sc[tid + off]));
        m = fp_sqr(m);
        __syncthreads();
    }
    if (tid == 0) fp_store(seg_h + ((size_t)z * B + b) * S + blockIdx.x, sc[0]);
}

// Launch 2 of 3, grid (B, 1, 2), lane s = segment s: the suffix scan over segments with m = x0^(n / S); seg_h[s] <- the carry
// entering segment s, q at the segment's last index = sum_{j >= segment end} p_j x0^(j - end).
__global__ void __launch_bounds__(SCAN_THREADS) divide_seg_carries_kernel(unsigned S, Fr w, const ProofState* st, size_t n, Fr* seg_h) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc[SCAN_THREADS];
    const size_t b = blockIdx.x, B = gridDim.x;
    const unsigned tid = threadIdx.x, z = blockIdx.z;
    const Fr x0 = divide_point(st, b, w, z);
    Fr* h = seg_h + ((size_t)z * B + b) * S;
    sc[tid] = tid < S ? fp_load(h + tid) : fp_zero<FrParams>();
    __syncthreads();
    block_suffix_scan_affine(sc, tid, fp_pow_u64(x0, (uint64_t)(n / S)));
    if (tid < S) fp_store(h + tid, tid + 1 < SCAN_THREADS ? sc[tid + 1] : fp_zero<FrParams>());
}

// Launch 3 of 3, grid (S, B, 2): the division inside the segment; the segment's carry enters its last lane, as the value one
// chunk above that lane's rows.
__global__ void __launch_bounds__(SCAN_THREADS) divide_seg_apply_kernel(DivideIn in, Fr w, const ProofState* st, size_t n, const Fr* seg_h) {
    PLONK_SHORT_KERNEL();
    __shared__ Fr sc[SCAN_THREADS];
    const size_t b = blockIdx.y, B = gridDim.y;
    const unsigned tid = threadIdx.x, S = gridDim.x, z = blockIdx.z;
    const Fr x0 = divide_point(st, b, w, z);
    const Fr* p = in.p_in[z] + b * n;
    const LaneRange r = seg_lane_range(n, S, blockIdx.x, tid);
    const size_t L = n / S;
    const unsigned last = (unsigned)(L < SCAN_THREADS ? L : SCAN_THREADS) - 1;  // the last lane that holds rows
    const Fr carry = fp_load(seg_h + ((size_t)z * B + b) * S + blockIdx.x);
    const Fr m = fp_pow_u64(x0, (uint64_t)r.per);
    Fr h = divide_chunk_horner(p, r, x0);
    if (tid == last) h = fp_add(h, fp_mul(m, carry));
    sc[tid] = h;
    __syncthreads();
    block_suffix_scan_affine(sc, tid, m);
    divide_chunk_writeback(p, in.q_out[z] + b * n, r, x0, tid < last ? sc[tid + 1] : carry);
}

// ================================================================================================
// host side

// How many segments S the three per-proof scans are cut into for `B` proofs of 2^log_n rows on a device of `cus` compute units
// (1: the one-workgroup kernels).  Measured on an MI355X, 256 CUs (profiles/prover_large.json, tools/prover_scale.py; the table
// is in DESIGN.md 4.3), the three scans together, per plonk_prover_run:
//   * SEG_WORKGROUPS_PER_CU = 1.  The scans are fastest where B S reaches the number of CUs and lose beyond it: at 2^16,
//     B = 64: S = 1 / 2 / 4 / 8 / 64 -> 4.51 / 2.75 / 1.79 / 1.84 / 2.64 ms; B = 8: fastest at S = 32 (0.53 ms, 4.33 at S = 1).
//     So: S = 1 when B alone gives every CU a workgroup, else the smallest power of two with B S >= CUs.
//   * SEG_MIN_ROWS = 256: a segment keeps a row for every lane of its workgroup.  At B = 1 the time stops falling there —
//     2^13: 0.284 ms at S = 32 (256 rows), 0.287 / 0.286 / 0.308 at 64 / 128 / 256; 2^14: 0.291 at S = 64, 0.310 at 256 — and
//     shorter segments only add idle lanes to the three launches.
//   * SEG_MIN_LOG_N = 13 is not a measurement: up to 2^12 rows the launches are what the benchmark and the suite's fixtures have
//     pinned, and they stay one workgroup per proof (the table has 0.15 ms of 2.0 to gain at 2^12, B <= 8).
// With these the rule's choice beats S = 1 in every measured cell from 2^13 up, by more than the spread of five runs.
#define SEG_WORKGROUPS_PER_CU 1
#define SEG_MIN_ROWS 256
#define SEG_MIN_LOG_N 13
unsigned prover_plan_segments(unsigned cus, unsigned log_n, size_t B) {
    if (log_n < SEG_MIN_LOG_N) return 1;
    const size_t n = (size_t)1 << log_n, want = (size_t)SEG_WORKGROUPS_PER_CU * (cus ? cus : 1);
    unsigned S = 1;
    while ((size_t)S * B < want && S < SCAN_THREADS && n / (2 * S) >= SEG_MIN_ROWS) S *= 2;
    return S;
}

// Which form the witness solve of `B` proofs takes (witness_solve.h): PLONK_PROVER_SOLVE_LANES, one lane per proof walking the `active`
// rows in program order, or PLONK_PROVER_SOLVE_LEVELS, one workgroup of `threads` lanes per proof walking `steps` = sum over the
// dependency levels of ceil(width / threads) steps, each a row and a workgroup barrier.  Both are chains of dependent loads, so a
// launch costs its serial steps times the rounds the chip needs to hold every wave of it:
//     lanes    active x SOLVE_ROW_NS             x ceil(ceil(B / 64) / (cus x SOLVE_WAVES_PER_CU))
//     levels   steps  x SOLVE_LEVEL_STEP[_WIDE]_NS x ceil(B x threads / 64 / (cus x SOLVE_WAVES_PER_CU))
// Measured on an MI355X (profiles/witness_levels.json, tools/witness_levels_bench.py; the table is in DESIGN.md 4.3).  The three
// step costs are fitted on the B = 1 cells, where nothing but the chain of steps is timed: a row of the one-lane form costs
// 1.16 - 1.41 us over the four circuits (median 1.23); a level step 1.40 - 1.47 us (median 1.45) where the workgroup is one wave (T = 64: the barrier is nearly
// free) and 2.15 us where it is four (T = 256, poseidon_multi(64)).  SOLVE_WAVES_PER_CU is not a measurement: both kernels compile to
// 7 waves per SIMD (profiles/witness_levels_kernel_resource_usage.txt), and no batch of the table fills the chip with them.  A
// level step costs more than a row step, so a circuit whose levels are one row wide (steps == active: a chain) keeps the one-lane
// form for every B.  With these the rule's pick is the faster forced form in all 16 measured cells.
// NOT measured: the rule models one prover alone on the chip.  The levelised form holds threads / 64 waves per proof where the
// one-lane form holds 1 / 64 of a wave, so under several contexts proving at once (bench.py's 20 streams) its shorter latency is
// bought with wave slots the other streams' kernels could use; the multi-stream step from inputs (tools/witness_bench.py part b) has
// been measured on the chain only, which stays on the one-lane form.  No measured cell has rounds > 1 either.
#define SOLVE_ROW_NS 1231.0
#define SOLVE_LEVEL_STEP_NS 1454.0
#define SOLVE_LEVEL_STEP_WIDE_NS 2147.0
#define SOLVE_WAVES_PER_CU 28
unsigned solve_plan_form(unsigned cus, uint32_t active, uint32_t steps, uint32_t threads, size_t B) {
    const size_t slots = (size_t)(cus ? cus : 1) * SOLVE_WAVES_PER_CU;
    auto rounds = [slots](size_t waves) { return (double)((waves + slots - 1) / slots); };
    const double lanes = (double)active * SOLVE_ROW_NS * rounds((B + 63) / 64);
    const double levels = (double)steps * (threads > 64 ? SOLVE_LEVEL_STEP_WIDE_NS : SOLVE_LEVEL_STEP_NS) * rounds(B * (threads / 64));
    return levels < lanes ? PLONK_PROVER_SOLVE_LEVELS : PLONK_PROVER_SOLVE_LANES;
}

// The scratch of the segmented scans, `seg`: the carries and partial sums of the S segments of B proofs, none while S = 1.  The
// three families follow each other on one stream and share it from its start: the evaluations' seven partial sums per segment
// are the largest (7 B S), the grand product takes 2 B S + B (numerator carries, denominator carries, the proofs' inversions), the
// two divisions 2 B S.  These two functions are the only place that knows the layout.
static size_t scan_scratch_elems(size_t B, unsigned S) { return S > 1 ? (size_t)NEVAL * B * S + B : 0; }
struct ScanScratch {
    Fr *gp_n, *gp_d, *gp_tot_inv;  // [B][S], [B][S], [B]
    Fr* eval_part;                 // [B][S][NEVAL]
    Fr* div_h;                     // [2][B][S]
};
static ScanScratch scan_scratch_parts(Fr* seg, size_t B, unsigned S) { return {seg, seg + B * S, seg + 2 * B * S, seg, seg}; }

// The launchers: S = 1 is the one-workgroup kernel, S > 1 the segmented launches; `seg` holds scan_scratch_elems(B, S).
static int scan_grand_product(hipStream_t s, unsigned S, const GrandProductIn& gp, const Fr* roots, const ProofState* st,
                              const RoundChallenges& direct, size_t n, size_t B, Fr* z_out, uint32_t* closes, Fr* num, Fr* den, Fr* seg) {
    if (S == 1) {
        PLONK_LAUNCH(grand_product_kernel, dim3((unsigned)B), dim3(SCAN_THREADS), 0, s, gp, roots, st, direct, n, z_out, closes, num, den);
        return PLONK_OK;
    }
    const ScanScratch sc = scan_scratch_parts(seg, B, S);
    PLONK_LAUNCH(gp_seg_factors_kernel, dim3(S, (unsigned)B), dim3(SCAN_THREADS), 0, s, gp, roots, st, direct, n, num, den, sc.gp_n, sc.gp_d);
    PLONK_LAUNCH(gp_seg_carries_kernel, dim3((unsigned)B), dim3(SCAN_THREADS), 0, s, S, sc.gp_n, sc.gp_d, sc.gp_tot_inv, closes);
    PLONK_LAUNCH(gp_seg_apply_kernel, dim3(S, (unsigned)B), dim3(SCAN_THREADS), 0, s, n, (const Fr*)sc.gp_n, (const Fr*)sc.gp_d,
                 (const Fr*)sc.gp_tot_inv, (const Fr*)num, den, z_out);
    return PLONK_OK;
}

static int scan_evaluations(hipStream_t s, unsigned S, const Fr* coef, const Fr* fixed_coef, const uint32_t* cid, const Fr& w, ProofState* st,
                            size_t n, size_t B, Fr* seg) {
    if (S == 1) {
        PLONK_LAUNCH(eval_kernel, dim3((unsigned)B), dim3(SCAN_THREADS), 0, s, coef, fixed_coef, cid, w, st, n, B);
        return PLONK_OK;
    }
    Fr* part = scan_scratch_parts(seg, B, S).eval_part;
    PLONK_LAUNCH(eval_seg_kernel, dim3(S, (unsigned)B), dim3(SCAN_THREADS), 0, s, coef, fixed_coef, cid, w, (const ProofState*)st, n, B, part);
    PLONK_LAUNCH(eval_seg_finish_kernel, dim3((unsigned)B), dim3(SCAN_THREADS), 0, s, (const Fr*)part, S, st);
    return PLONK_OK;
}

// S = 1: one launch per opening; S > 1: both openings share the launches (blockIdx.z)
static int scan_divisions(hipStream_t s, unsigned S, const DivideIn& dv, const Fr& w, const ProofState* st, size_t n, size_t B, Fr* seg) {
    if (S == 1) {
        for (int z = 0; z < 2; z++)
            PLONK_LAUNCH(divide_linear_kernel, dim3((unsigned)B), dim3(SCAN_THREADS), 0, s, dv.p_in[z], n, z, w, st, n, dv.q_out[z]);
        return PLONK_OK;
    }
    Fr* seg_h = scan_scratch_parts(seg, B, S).div_h;
    PLONK_LAUNCH(divide_seg_horner_kernel, dim3(S, (unsigned)B, 2), dim3(SCAN_THREADS), 0, s, dv, w, st, n, seg_h);
    PLONK_LAUNCH(divide_seg_carries_kernel, dim3((unsigned)B, 1, 2), dim3(SCAN_THREADS), 0, s, S, w, st, n, seg_h);
    PLONK_LAUNCH(divide_seg_apply_kernel, dim3(S, (unsigned)B, 2), dim3(SCAN_THREADS), 0, s, dv, w, st, n, (const Fr*)seg_h);
    return PLONK_OK;
}
