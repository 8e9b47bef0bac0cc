// verifier.hip — the batch verifier (plonk_verifier_*, plonk_g1_mul_many): N proofs of one circuit, or of a table of circuits
// of one setup, under one pairing check.
//
// Reference behaviour replaced: verify_proof of TESTING_verifier_DO_NOT_OPEN.py:39-163 (challenges :266-277) for a batch.  Every
// proof's check is e(L_i, [x]_2) == e(R_i, [1]_2) with L_i, R_i in G1, so with random 128-bit weights rho_i the batch is accepted
// iff e(sum rho_i L_i, [x]_2) == e(sum rho_i R_i, [1]_2): the device returns the two sums, the pairing stays on the host
// (plonk_pairing_check).  The record layout and the resident batch are prover.h's, the device transcript transcript_device.h's.
// Three steps per loaded batch:
//   verify_scalars_kernel   32 lanes per proof: well-formedness, transcript replay, the weighted scalars of the proof's terms
//   g1_mul_many_kernel      one lane per (proof, term): k * P by double-and-add on the complete formulas of g1.h
//   verify_fold_proof_kernel / verify_fold_kernel   L_i, R_i per proof (kept), then the sum over any range [lo, hi) + the nine
//                           fixed-point products (their scalars are summed over the range in Fr first) -> two affine points
// A table of K > 1 circuits folds with verify_fold_circuit_kernel (one workgroup per circuit: its eight key-point sums and
// products -> one partial point) and verify_fold_multi_kernel (L, R over the range + the partials) in place of the last.
// Per-proof verdicts without bisection (plonk_verifier_check_each): verify_fixed_products_kernel (the nine fixed-point products of
// EVERY proof, which the folds only ever form over a range), verify_own_points_kernel (L_b and -R_b complete, affine) and the
// per-lane pairing check of pairing_device.h over the line tables of [x]_2 and [1]_2 (plonk_verifier_set_x2).
#include <string.h>

#include "plonk_internal.h"
#include "transcript.h"
#include "transcript_device.h"
#include "prover.h"
#include "pairing_device.h"

#define VF_OWN 11    // a_1, b_1, c_1, z_1, t_lo_1, t_mid_1, t_hi_1, W_z_1, W_zw_1 in R_i;  W_z_1, W_zw_1 in L_i
#define VF_FIXED 9   // Qm, Ql, Qr, Qo, Qc, S1, S2, S3, G1
#define VF_MALFORMED 1u
#define VF_OFF_CURVE 2u
#define VF_IDENTITY 4u

// k * p for a canonical k < 2^254 and an affine p: left-to-right double-and-add on the complete formulas of g1.h.  The scalar
// is shifted out of its top bit, so its words keep constant indices; the fences keep the scheduler from interleaving the
// doubling's multiplications with the addition's (which multiplies the live registers).  Leading doublings of the identity
// return at once.
PLONK_DEV G1Xyzz g1_mul_affine(const G1Affine& p, Fr k) {
    G1Xyzz acc = g1_xyzz_identity();
    if (g1_affine_is_identity(p)) return acc;
#pragma unroll
    for (int i = 7; i > 0; i--) k.v[i] = (k.v[i] << 2) | (k.v[i - 1] >> 30);
    k.v[0] <<= 2;
#pragma unroll 1
    for (int bit = 0; bit < 254; bit++) {
        g1_dbl(acc);
        PLONK_SCHED_FENCE();
        if (k.v[7] >> 31) g1_madd<true>(acc, p);  // the rare acc == +-p exit as a call (g1.h:79-81)
        PLONK_SCHED_FENCE();
#pragma unroll
        for (int i = 7; i > 0; i--) k.v[i] = (k.v[i] << 1) | (k.v[i - 1] >> 31);
        k.v[0] <<= 1;
    }
    return acc;
}

// out[j] = scalars[j] * points[j]: points affine in Montgomery form ((0, 0) = identity), scalars canonical
__global__ void __launch_bounds__(64) g1_mul_many_kernel(const G1Affine* points, const Fr* scalars, size_t count, G1Xyzz* out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    G1Affine p;
    p.x = fp_load(&points[j].x);
    p.y = fp_load(&points[j].y);
    const G1Xyzz r = g1_mul_affine(p, fp_load(scalars + j));
    fp_store(&out[j].x, r.x);
    fp_store(&out[j].y, r.y);
    fp_store(&out[j].zz, r.zz);
    fp_store(&out[j].zzz, r.zzz);
}

PLONK_DEV G1Xyzz vf_load_xyzz(const G1Xyzz* p) {
    G1Xyzz r;
    r.x = fp_load(&p->x);
    r.y = fp_load(&p->y);
    r.zz = fp_load(&p->zz);
    r.zzz = fp_load(&p->zzz);
    return r;
}
PLONK_DEV void vf_store_xyzz(G1Xyzz* p, const G1Xyzz& r) {
    fp_store(&p->x, r.x);
    fp_store(&p->y, r.y);
    fp_store(&p->zz, r.zz);
    fp_store(&p->zzz, r.zzz);
}

// Per proof: plain record (prover.h) + public inputs -> status byte, the eleven points in Montgomery form, their weighted scalars
// (canonical: g1_mul_many_kernel reads bits) and the nine weighted fixed-point scalars (Montgomery: verify_fold_kernel sums them).
// Lane layout of transcript_kernel: 32 lanes per proof, two proofs per workgroup, barriers uniform — a malformed proof replays the
// transcript over its bytes as they are and its results are dropped (weight zero: identity points, zero scalars).
//   init[0] = the transcript after Transcript(b"plonk"); init[1] = the weight transcript after the seed
//   inv_tmp [B][max(n_public, 1)]: prefix products of the shared inversion (PI(zeta) and L0(zeta) need 1 / (zeta - w^i))
// The domain and the number of public inputs are those of the proof's circuit: table[circuit[b]], public row at pub_off[b], inversion
// row at inv_off[b] (exclusive sums of n_public and of max(n_public, 1) over the batch).  circuit == nullptr: every proof is of
// table[0] and the rows are uniform, no offsets needed.  Only lane 0's tail, behind the last barrier, reads any of it, so the two
// proofs of a workgroup may be of circuits of different size.
struct VfShared {
    TcShared tc;
    uint32_t status;
    uint32_t pad_[3];
};
struct VfCircuit { Fr w, w_inv, n_inv; uint32_t log_n, n_public; };
__global__ void __launch_bounds__(2 * TC_LANES) verify_scalars_kernel(const uint8_t* proofs, const Fr* pub, size_t B, const MerlinState* init,
                                                                      ChallengeConsts cc, const VfCircuit* table, const uint32_t* circuit,
                                                                      const size_t* pub_off, const size_t* inv_off, Fr* inv_tmp, G1Affine* pts,
                                                                      Fr* own, Fr* fixed, uint8_t* status) {
    __shared__ VfShared shared[2];
    const unsigned grp = threadIdx.x / TC_LANES, lane = threadIdx.x % TC_LANES;
    TcShared& sh = shared[grp].tc;
    size_t b = (size_t)blockIdx.x * 2 + grp;
    const bool live = b < B;
    if (!live) b = B - 1;  // shadow the last proof so the barriers stay uniform; nothing is stored
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(proofs + b * PROOF_BYTES);
    if (lane == 0) shared[grp].status = 0;
    __syncthreads();

    // ---- well-formedness: lane k < 11 owns the point of term k (W_z_1, W_zw_1 twice), lanes 11..16 an evaluation
    uint32_t bad = 0;
    G1Affine P = g1_affine_identity();
    if (lane < VF_OWN) {
        const unsigned k = lane < 9 ? lane : lane - 2;
        Fq x, y;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            x.v[i] = rec[proof_point_word(k, 0) + i];
            y.v[i] = rec[proof_point_word(k, 1) + i];
        }
        if (!fp_below_modulus<FqParams>(x.v) || !fp_below_modulus<FqParams>(y.v)) bad = VF_MALFORMED;
        else if (fp_is_zero(x) && fp_is_zero(y)) bad = VF_IDENTITY;  // the reference's transcript refuses None (transcript.py:62-67)
        else {
            P.x = fp_to_mont(x);
            P.y = fp_to_mont(y);
            if (!g1_affine_on_curve(P.x, P.y)) bad = VF_OFF_CURVE;  // cofactor 1: on the curve is in the group
        }
    } else if (lane < VF_OWN + PROOF_EVALS) {
        uint32_t e[8];
#pragma unroll
        for (int i = 0; i < 8; i++) e[i] = rec[proof_eval_word(lane - VF_OWN) + i];
        if (!fp_below_modulus<FrParams>(e)) bad = VF_MALFORMED;
    }
    if (bad) atomicOr(&shared[grp].status, bad);
    __syncthreads();
    const uint32_t st = shared[grp].status;

    // ---- transcript replay (TESTING_verifier:266-277)
    TcState t = tc_load(init[0], lane);
    Fr beta, gamma, alpha, zeta, v, u, unused;
    // staging: `count` 32-byte values from rec[word], big-endian, to sh.msg
    const auto round = [&](int r, unsigned word, unsigned count, Fr& c0, Fr& c1) PLONK_LAMBDA_INLINE {
        __syncthreads();  // earlier readers of sh.msg are done
        if (lane < count) {
            uint32_t x[8];
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = rec[word + 8 * lane + i];
            limbs_to_be32(x, sh.msg + 32 * lane);
        }
        __syncthreads();
        tc_round(t, sh, lane, cc, r, c0, c1);
    };
    round(1, proof_point_word(0, 0), 6, beta, gamma);
    round(2, proof_point_word(3, 0), 2, alpha, unused);  // fft_cofactor is drawn and dropped
    round(3, proof_point_word(4, 0), 6, zeta, unused);
    round(4, proof_eval_word(0), PROOF_EVALS, v, unused);
    round(5, proof_point_word(7, 0), 4, u, unused);

    // ---- the weight: a clone of the seeded transcript, the proof's index, 16 challenge bytes read little-endian
    TcState tr = tc_load(init[1], lane);
    __syncthreads();
    if (lane < 8) sh.msg[lane] = (uint8_t)((uint64_t)b >> (8 * lane));
    __syncthreads();
    tc_append_message(tr, sh, lane, "index", 5, sh.msg, 8);
    tc_frame(tr, sh, lane, "rho", 3, 16);
    tc_begin_op(tr, sh, lane, STROBE_FLAG_I | STROBE_FLAG_A | STROBE_FLAG_C);
    __syncthreads();
    tc_squeeze(tr, sh, lane, sh.msg, 16);
    __syncthreads();

    if (!live) return;
    if (lane < VF_OWN) {
        if (st) P = g1_affine_identity();
        fp_store(&pts[b * VF_OWN + lane].x, P.x);
        fp_store(&pts[b * VF_OWN + lane].y, P.y);
    }
    if (lane != 0) return;
    status[b] = (uint8_t)st;
    Fr* o_own = own + b * VF_OWN;
    Fr* o_fix = fixed + b * VF_FIXED;
    if (st) {  // takes part in no fold
        for (int k = 0; k < VF_OWN; k++) fp_store(o_own + k, fp_zero<FrParams>());
        for (int k = 0; k < VF_FIXED; k++) fp_store(o_fix + k, fp_zero<FrParams>());
        return;
    }
    const Fr one = fp_one<FrParams>();
    Fr rho = fp_zero<FrParams>();
#pragma unroll
    for (int i = 0; i < 4; i++)
        rho.v[i] = (uint32_t)sh.msg[4 * i] | ((uint32_t)sh.msg[4 * i + 1] << 8) | ((uint32_t)sh.msg[4 * i + 2] << 16) | ((uint32_t)sh.msg[4 * i + 3] << 24);
    rho = fp_to_mont(rho);
    Fr ev[PROOF_EVALS];
#pragma unroll
    for (int e = 0; e < PROOF_EVALS; e++) {
        Fr x;
#pragma unroll
        for (int i = 0; i < 8; i++) x.v[i] = rec[proof_eval_word(e) + i];
        ev[e] = fp_to_mont(x);
    }
    const Fr a = ev[0], bb = ev[1], c = ev[2], s1 = ev[3], s2 = ev[4], zw = ev[5];
    const VfCircuit* circ = table + (circuit ? circuit[b] : 0);
    const Fr dom_w = fp_load(&circ->w), dom_w_inv = fp_load(&circ->w_inv), dom_n_inv = fp_load(&circ->n_inv);
    const unsigned log_n = circ->log_n;
    const size_t n_public = circ->n_public;
    Fr zn = zeta;
    for (unsigned i = 0; i < log_n; i++) zn = fp_sqr(zn);
    const Fr zh = fp_sub(zn, one);
    // 1 / (zeta - w^i), i < m, by ONE inversion (Montgomery's trick; a zero denominator inverts to zero, as the reference's field does)
    const size_t m = n_public ? n_public : 1;
    Fr* tmp = inv_tmp + (circuit ? inv_off[b] : b * m);
    const Fr* row = pub + (circuit ? pub_off[b] : b * n_public);
    Fr run = one, wi = one, w_last = one;
    for (size_t i = 0; i < m; i++) {
        Fr d = fp_sub(zeta, wi);
        if (fp_is_zero(d)) d = one;
        fp_store(tmp + i, run);
        run = fp_mul(run, d);
        w_last = wi;
        wi = fp_mul(wi, dom_w);
    }
    Fr inv = fp_inv(run), sum = fp_zero<FrParams>(), inv0 = fp_zero<FrParams>();
    wi = w_last;
    for (size_t i = m; i-- > 0;) {
        const Fr d = fp_sub(zeta, wi);
        Fr inv_i = fp_zero<FrParams>();
        if (!fp_is_zero(d)) {
            inv_i = fp_mul(inv, fp_load(tmp + i));
            inv = fp_mul(inv, d);
        }
        if (i < n_public) sum = fp_add(sum, fp_mul(fp_mul(fp_load(row + i), wi), inv_i));
        if (i == 0) inv0 = inv_i;
        wi = fp_mul(wi, dom_w_inv);
    }
    const Fr zhn = fp_mul(zh, dom_n_inv);
    const Fr pi = fp_neg(fp_mul(zhn, sum));  // PI = sum (-public_i) L_i(zeta), poly.py:181-195
    const Fr l0 = fp_mul(zhn, inv0);         // L0 = Z_H / (n (zeta - 1))
    const Fr bz = fp_mul(beta, zeta);
    const Fr k1 = fp_mul(fp_mul(fp_add(fp_add(a, bz), gamma), fp_add(fp_add(bb, fp_dbl(bz)), gamma)), fp_add(fp_add(c, fp_mul3(bz)), gamma));
    const Fr e12 = fp_mul(fp_add(fp_add(a, fp_mul(beta, s1)), gamma), fp_add(fp_add(bb, fp_mul(beta, s2)), gamma));
    const Fr l0a2 = fp_mul(l0, fp_sqr(alpha));
    const Fr ae12zw = fp_mul(fp_mul(alpha, e12), zw);
    const Fr r0 = fp_sub(fp_sub(pi, l0a2), fp_mul(ae12zw, fp_add(c, gamma)));
    const Fr v2 = fp_sqr(v), v3 = fp_mul(v2, v), v4 = fp_sqr(v2), v5 = fp_mul(v4, v);
    Fr open = fp_add(fp_mul(v, a), fp_mul(v2, bb));
    open = fp_add(open, fp_add(fp_mul(v3, c), fp_mul(v4, s1)));
    open = fp_add(open, fp_add(fp_mul(v5, s2), fp_mul(u, zw)));
    const Fr nzh = fp_neg(zh);
    const Fr s_own[VF_OWN] = {v, v2, v3, fp_add(fp_add(fp_mul(alpha, k1), l0a2), u), nzh, fp_mul(nzh, zn), fp_mul(nzh, fp_sqr(zn)),
                              zeta, fp_mul(fp_mul(u, zeta), dom_w), one, u};
    const Fr s_fix[VF_FIXED] = {fp_mul(a, bb), a, bb, c, one, v4, v5, fp_neg(fp_mul(ae12zw, beta)), fp_sub(r0, open)};
#pragma unroll
    for (int k = 0; k < VF_OWN; k++) fp_store(o_own + k, fp_from_mont(fp_mul(s_own[k], rho)));
#pragma unroll
    for (int k = 0; k < VF_FIXED; k++) fp_store(o_fix + k, fp_mul(s_fix[k], rho));
}

// lr[2 b] = L_b = products 9, 10 of proof b; lr[2 b + 1] = R_b = products 0..8.  One lane per (proof, side).
__global__ void __launch_bounds__(64) verify_fold_proof_kernel(const G1Xyzz* prod, size_t B, G1Xyzz* lr) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * B) return;
    const size_t b = j >> 1;
    const unsigned first = (j & 1) ? 0 : 9, count = (j & 1) ? 9 : 2;
    G1Xyzz acc = vf_load_xyzz(prod + b * VF_OWN + first);
#pragma unroll 1
    for (unsigned k = 1; k < count; k++) g1_add(acc, vf_load_xyzz(prod + b * VF_OWN + first + k));
    vf_store_xyzz(lr + j, acc);
}

#define VF_FOLD_THREADS 256
// red[0] = the sum of red[0 .. VF_FOLD_THREADS) (tree through LDS; every lane of the workgroup calls, the result is behind a barrier)
PLONK_DEV void vf_tree_points(G1Xyzz* red, unsigned tid) {
    __syncthreads();
#pragma unroll 1
    for (unsigned s = VF_FOLD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            G1Xyzz x = red[tid];
            g1_add(x, red[tid + s]);
            red[tid] = x;
        }
        __syncthreads();
    }
}
// total[side] = the sum of lr[2 b + side] over the well-formed proofs lo <= b < hi, side = 0 (L), 1 (R)
PLONK_DEV void vf_sum_lr(const G1Xyzz* lr, const uint8_t* status, size_t lo, size_t hi, G1Xyzz* red, G1Xyzz* total, unsigned tid) {
#pragma unroll 1
    for (unsigned side = 0; side < 2; side++) {
        G1Xyzz acc = g1_xyzz_identity();
#pragma unroll 1
        for (size_t b = lo + tid; b < hi; b += VF_FOLD_THREADS)
            if (!status[b]) g1_add(acc, vf_load_xyzz(lr + 2 * b + side));
        red[tid] = acc;
        vf_tree_points(red, tid);
        if (tid == 0) total[side] = red[0];
        __syncthreads();
    }
}
// fsum[k] = the sum of fixed[b][k] over the well-formed proofs lo <= b < hi — of circuit `c` only, if `circuit` is given
PLONK_DEV void vf_sum_fixed(const Fr* fixed, const uint8_t* status, const uint32_t* circuit, uint32_t c, size_t lo, size_t hi, unsigned k, Fr* fred,
                            Fr* fsum, unsigned tid) {
    Fr acc = fp_zero<FrParams>();
    for (size_t b = lo + tid; b < hi; b += VF_FOLD_THREADS)
        if (!status[b] && (!circuit || circuit[b] == c)) acc = fp_add(acc, fp_load(fixed + b * VF_FIXED + k));
    fred[tid] = acc;
    __syncthreads();
    for (unsigned s = VF_FOLD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) fred[tid] = fp_add(fred[tid], fred[tid + s]);
        __syncthreads();
    }
    if (tid == 0) fsum[k] = fred[0];
    __syncthreads();
}
// out_xy = L.x, L.y, R.x, R.y canonical; out_flags[side] = 1 for the identity.  Lanes 0 (L) and 1 (R); `extra` goes into R.
PLONK_DEV void vf_fold_out(const G1Xyzz* total, const G1Xyzz* extra, unsigned n_extra, Fq* out_xy, uint8_t* out_flags, unsigned tid) {
    if (tid >= 2) return;
    G1Xyzz acc = total[tid];
    if (tid == 1)
#pragma unroll 1
        for (unsigned k = 0; k < n_extra; k++) g1_add(acc, extra[k]);
    const G1Affine r = g1_to_affine(acc);
    fp_store(out_xy + 2 * tid, fp_from_mont(r.x));
    fp_store(out_xy + 2 * tid + 1, fp_from_mont(r.y));
    out_flags[tid] = g1_is_identity(acc) ? 1 : 0;
}

// One circuit.  One workgroup: sum of L_b, of R_b and of the nine fixed-point scalars over lo <= b < hi (tree through LDS), the nine
// fixed-point products, R += them, both sums to affine.
__global__ void __launch_bounds__(VF_FOLD_THREADS) verify_fold_kernel(const G1Xyzz* lr, const Fr* fixed, const uint8_t* status, size_t lo, size_t hi,
                                                                      const G1Affine* bases, Fq* out_xy, uint8_t* out_flags) {
    __shared__ G1Xyzz red[VF_FOLD_THREADS];
    __shared__ Fr fred[VF_FOLD_THREADS];
    __shared__ G1Xyzz total[2];
    __shared__ Fr fsum[VF_FIXED];
    const unsigned tid = threadIdx.x;
    vf_sum_lr(lr, status, lo, hi, red, total, tid);
#pragma unroll 1
    for (unsigned k = 0; k < VF_FIXED; k++) vf_sum_fixed(fixed, status, nullptr, 0, lo, hi, k, fred, fsum, tid);
    if (tid < VF_FIXED) {
        G1Affine p;
        p.x = fp_load(&bases[tid].x);
        p.y = fp_load(&bases[tid].y);
        red[tid] = g1_mul_affine(p, fp_from_mont(fsum[tid]));
    }
    __syncthreads();
    vf_fold_out(total, red, VF_FIXED, out_xy, out_flags, tid);
}

// A table of K circuits, workgroup c = circuit c: the eight key-point scalars summed over the well-formed proofs OF CIRCUIT c in
// lo <= b < hi, times bases[8 c + k], summed -> partial[c] (the identity if the range holds no such proof: every sum is zero).
// The ninth scalar multiplies G1 whatever the circuit: workgroup 0 sums it over the whole range, partial[K] = that product.
__global__ void __launch_bounds__(VF_FOLD_THREADS) verify_fold_circuit_kernel(const Fr* fixed, const uint8_t* status, const uint32_t* circuit, size_t lo,
                                                                              size_t hi, const G1Affine* bases, unsigned K, G1Xyzz* partial) {
    __shared__ Fr fred[VF_FOLD_THREADS];
    __shared__ Fr fsum[VF_FIXED];
    __shared__ G1Xyzz prod[VF_FIXED];
    const unsigned tid = threadIdx.x, c = blockIdx.x;
    const unsigned terms = c == 0 ? VF_FIXED : VF_FIXED - 1;  // uniform over the workgroup
#pragma unroll 1
    for (unsigned k = 0; k < terms; k++) vf_sum_fixed(fixed, status, k < VF_FIXED - 1 ? circuit : nullptr, c, lo, hi, k, fred, fsum, tid);
    if (tid < terms) {
        const G1Affine* base = tid < VF_FIXED - 1 ? bases + (size_t)c * (VF_FIXED - 1) + tid : bases + (size_t)K * (VF_FIXED - 1);
        G1Affine p;
        p.x = fp_load(&base->x);
        p.y = fp_load(&base->y);
        prod[tid] = g1_mul_affine(p, fp_from_mont(fsum[tid]));
    }
    __syncthreads();
    if (tid == 0) {
        G1Xyzz acc = prod[0];
#pragma unroll 1
        for (unsigned k = 1; k < VF_FIXED - 1; k++) g1_add(acc, prod[k]);
        vf_store_xyzz(partial + c, acc);
        if (terms == VF_FIXED) vf_store_xyzz(partial + K, prod[VF_FIXED - 1]);
    }
}

// ... and one workgroup after them: sum of L_b and of R_b over lo <= b < hi, R += the n_partial <= VF_FOLD_THREADS partial points
__global__ void __launch_bounds__(VF_FOLD_THREADS) verify_fold_multi_kernel(const G1Xyzz* lr, const uint8_t* status, size_t lo, size_t hi,
                                                                            const G1Xyzz* partial, unsigned n_partial, Fq* out_xy, uint8_t* out_flags) {
    __shared__ G1Xyzz red[VF_FOLD_THREADS];
    __shared__ G1Xyzz total[2];
    const unsigned tid = threadIdx.x;
    vf_sum_lr(lr, status, lo, hi, red, total, tid);
    red[tid] = tid < n_partial ? vf_load_xyzz(partial + tid) : g1_xyzz_identity();
    vf_tree_points(red, tid);
    vf_fold_out(total, red, 1, out_xy, out_flags, tid);
}

// check_each, one lane per (proof, fixed term k): prod[9 b + k] = fixed[b][k] * (Qm .. S3 of the proof's circuit, k < 8; G1, k = 8);
// the identity for a proof that is not well-formed.  circuit == nullptr: every proof is of circuit 0.
__global__ void __launch_bounds__(64) verify_fixed_products_kernel(const Fr* fixed, const uint8_t* status, const uint32_t* circuit, const G1Affine* bases,
                                                                   unsigned K, size_t B, G1Xyzz* prod) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B * VF_FIXED) return;
    const size_t b = j / VF_FIXED;
    const unsigned k = (unsigned)(j % VF_FIXED);
    if (status[b]) {
        vf_store_xyzz(prod + j, g1_xyzz_identity());
        return;
    }
    const G1Affine* base = k < VF_FIXED - 1 ? bases + (size_t)(circuit ? circuit[b] : 0) * (VF_FIXED - 1) + k : bases + (size_t)K * (VF_FIXED - 1);
    G1Affine p;
    p.x = fp_load(&base->x);
    p.y = fp_load(&base->y);
    vf_store_xyzz(prod + j, g1_mul_affine(p, fp_from_mont(fp_load(fixed + j))));
}
// check_each, one lane per (proof, side): pts[2 b] = L_b, pts[2 b + 1] = -(R_b + the proof's nine fixed-point products), affine with
// (0, 0) for the identity: the proof's own check is e(pts[2 b], [x]_2) e(pts[2 b + 1], [1]_2) == 1.  Reads lr, writes none of it.
__global__ void __launch_bounds__(64) verify_own_points_kernel(const G1Xyzz* lr, const G1Xyzz* prod, const uint8_t* status, size_t B, G1Affine* pts) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * B) return;
    const size_t b = j >> 1;
    G1Affine r = g1_affine_identity();
    if (!status[b]) {
        G1Xyzz acc = vf_load_xyzz(lr + j);
        if (j & 1)
#pragma unroll 1
            for (unsigned k = 0; k < VF_FIXED; k++) g1_add(acc, vf_load_xyzz(prod + b * VF_FIXED + k));
        r = g1_to_affine(acc);
        if (j & 1) r = g1_affine_neg(r);
    }
    fp_store(&pts[j].x, r.x);
    fp_store(&pts[j].y, r.y);
}

// plonk_g1_mul_many's marshalling: canonical points -> Montgomery form with the range / curve tests, products -> canonical affine
__global__ void g1_mul_many_in_kernel(Fq* xy, const Fr* scalars, size_t count, uint32_t* bad) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const Fq x = fp_load(xy + 2 * j), y = fp_load(xy + 2 * j + 1);
    const Fr k = fp_load(scalars + j);
    if (!fp_below_modulus<FqParams>(x.v) || !fp_below_modulus<FqParams>(y.v) || !fp_below_modulus<FrParams>(k.v)) {
        atomicOr(bad, 1u);
        fp_store(xy + 2 * j, fp_zero<FqParams>());
        fp_store(xy + 2 * j + 1, fp_zero<FqParams>());
        return;
    }
    if (fp_is_zero(x) && fp_is_zero(y)) return;
    const Fq xm = fp_to_mont(x), ym = fp_to_mont(y);
    if (!g1_affine_on_curve(xm, ym)) atomicOr(bad, 2u);
    fp_store(xy + 2 * j, xm);
    fp_store(xy + 2 * j + 1, ym);
}
__global__ void g1_mul_many_out_kernel(const G1Xyzz* prod, size_t count, Fq* out_xy, uint8_t* flags) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const G1Xyzz p = vf_load_xyzz(prod + j);
    const G1Affine r = g1_to_affine(p);
    fp_store(out_xy + 2 * j, fp_from_mont(r.x));
    fp_store(out_xy + 2 * j + 1, fp_from_mont(r.y));
    flags[j] = g1_is_identity(p) ? 1 : 0;
}

// ================================================================================================
// host side
static_assert(PLONK_VERIFIER_MAX_CIRCUITS + 1 <= VF_FOLD_THREADS, "verify_fold_multi_kernel: one lane per partial point");

struct plonk_verifier {
    plonk_ctx* ctx;
    unsigned n_circuits;     // K
    VfCircuit* h_circ;       // [K] domain and number of public inputs of each circuit
    VfCircuit* d_circ;
    ChallengeConsts chal;
    MerlinState h_init[2];   // [0] Transcript(b"plonk"), [1] the weight transcript after the seed of the last load
    MerlinState* d_init;
    G1Affine* d_bases;       // [8 K + 1] Qm, Ql, Qr, Qo, Qc, S1, S2, S3 of every circuit, then G1 (Montgomery)
    G1Xyzz* d_partial;       // [K + 1] verify_fold_circuit_kernel's points
    size_t cap, cap_pub, cap_inv, batch;  // allocated proofs / public values / inversion values; loaded proofs
    uint8_t* d_proofs;       // [B][PROOF_BYTES]
    Fr* d_pub;               // [B][n_public of the proof's circuit] Montgomery
    Fr* d_inv_tmp;           // [B][max(n_public, 1)]
    size_t* d_off;           // [2][B] each proof's row in d_pub and in d_inv_tmp  } of a batch loaded with circuit labels:
    uint32_t* d_circuit;     // [B] each proof's circuit                           } h_meta holds the three as they are uploaded
    void* h_meta;
    size_t h_meta_cap;
    G1Affine* d_pts;         // [B][11]
    Fr* d_own;               // [B][11] canonical
    Fr* d_fixed;             // [B][9] Montgomery
    G1Xyzz* d_prod;          // [B][11]
    G1Xyzz* d_lr;            // [B][2]  L_b, R_b: any sub-range folds again from these
    uint8_t* d_status;       // [B]
    Fq* d_out;               // [4] + 2 flag bytes behind them
    hipEvent_t* evs;         // [n_evs] a prover's pack is done (plonk_verifier_load_prover, _load_provers: one per prover)
    size_t n_evs;
    PairingLine* d_lines;    // [2][PAIRING_ATE_LINES] the ate loop's lines over [x]_2 and over [1]_2 (plonk_verifier_set_x2; null before)
};

static void verifier_free_batch(plonk_verifier* v) {
    dev_free_all({(void**)&v->d_proofs, (void**)&v->d_pub, (void**)&v->d_inv_tmp, (void**)&v->d_off, (void**)&v->d_circuit, (void**)&v->d_pts,
                  (void**)&v->d_own, (void**)&v->d_fixed, (void**)&v->d_prod, (void**)&v->d_lr, (void**)&v->d_status});
    v->cap = v->cap_pub = v->cap_inv = v->batch = 0;
}

// room for B proofs with n_pub public values and n_inv inversion values in all
static int verifier_ensure(plonk_verifier* v, size_t B, size_t n_pub, size_t n_inv) {
    if (B <= v->cap && n_pub <= v->cap_pub && n_inv <= v->cap_inv) return PLONK_OK;
    PLONK_CHECK_HIP(hipStreamSynchronize(v->ctx->stream));
    B = B > v->cap ? B : v->cap;
    n_pub = n_pub > v->cap_pub ? n_pub : v->cap_pub;
    n_inv = n_inv > v->cap_inv ? n_inv : v->cap_inv;
    verifier_free_batch(v);
    PLONK_TRY(dev_alloc((void**)&v->d_proofs, B * PROOF_BYTES));
    PLONK_TRY(dev_alloc((void**)&v->d_pub, n_pub * sizeof(Fr)));
    PLONK_TRY(dev_alloc((void**)&v->d_inv_tmp, n_inv * sizeof(Fr)));
    PLONK_TRY(dev_alloc((void**)&v->d_off, 2 * B * sizeof(size_t)));
    PLONK_TRY(dev_alloc((void**)&v->d_circuit, B * sizeof(uint32_t)));
    PLONK_TRY(dev_alloc((void**)&v->d_pts, B * VF_OWN * sizeof(G1Affine)));
    PLONK_TRY(dev_alloc((void**)&v->d_own, B * VF_OWN * sizeof(Fr)));
    PLONK_TRY(dev_alloc((void**)&v->d_fixed, B * VF_FIXED * sizeof(Fr)));
    PLONK_TRY(dev_alloc((void**)&v->d_prod, B * VF_OWN * sizeof(G1Xyzz)));
    PLONK_TRY(dev_alloc((void**)&v->d_lr, B * 2 * sizeof(G1Xyzz)));
    PLONK_TRY(dev_alloc((void**)&v->d_status, B));
    v->cap = B;
    v->cap_pub = n_pub;
    v->cap_inv = n_inv;
    return PLONK_OK;
}

// Host staging of a labelled batch: pub_off[B], inv_off[B] (size_t), circuit[B] (uint32_t), in the order they lie in h_meta
struct VfMeta { size_t *pub_off, *inv_off; uint32_t* circuit; };
static int verifier_meta(plonk_verifier* v, size_t B, VfMeta* m) {
    const size_t bytes = B * (2 * sizeof(size_t) + sizeof(uint32_t));
    if (bytes > v->h_meta_cap) {
        PLONK_CHECK_HIP(hipStreamSynchronize(v->ctx->stream));  // an upload from the old block may be on its way
        free(v->h_meta);
        v->h_meta_cap = 0;
        v->h_meta = malloc(bytes);
        PLONK_REQUIRE(v->h_meta, PLONK_ERR_NOMEM, "malloc(%zu) failed", bytes);
        v->h_meta_cap = bytes;
    }
    m->pub_off = (size_t*)v->h_meta;
    m->inv_off = m->pub_off + B;
    m->circuit = (uint32_t*)(m->inv_off + B);
    return PLONK_OK;
}
// proof b of the staging is of circuit c: its label and its rows; *n_pub and *n_inv run along
static void verifier_meta_set(const plonk_verifier* v, const VfMeta& m, size_t b, uint32_t c, size_t* n_pub, size_t* n_inv) {
    const size_t l = v->h_circ[c].n_public;
    m.circuit[b] = c;
    m.pub_off[b] = *n_pub;
    m.inv_off[b] = *n_inv;
    *n_pub += l;
    *n_inv += l ? l : 1;
}
static int verifier_meta_upload(plonk_verifier* v, size_t B, const VfMeta& m) {
    hipStream_t s = v->ctx->stream;
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_off, m.pub_off, B * sizeof(size_t), hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_off + v->cap, m.inv_off, B * sizeof(size_t), hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_circuit, m.circuit, B * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    return PLONK_OK;
}

// the proofs and public inputs of `B` proofs are in place on the verifier's stream (`labelled`: and their circuits and rows):
// weights, scalars, products, L_b and R_b
static int verifier_run(plonk_verifier* v, size_t B, const uint8_t seed[32], bool labelled) {
    plonk_ctx* ctx = v->ctx;
    hipStream_t s = ctx->stream;
    merlin_init(v->h_init[1], (const uint8_t*)"plonk-batch-verify", 18);
    merlin_append_message(v->h_init[1], (const uint8_t*)"seed", 4, seed, 32);
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_init, v->h_init, sizeof v->h_init, hipMemcpyHostToDevice, s));
    PLONK_LAUNCH(verify_scalars_kernel, dim3((unsigned)((B + 1) / 2)), dim3(2 * TC_LANES), 0, s, (const uint8_t*)v->d_proofs, (const Fr*)v->d_pub, B,
                 (const MerlinState*)v->d_init, v->chal, (const VfCircuit*)v->d_circ, labelled ? (const uint32_t*)v->d_circuit : (const uint32_t*)nullptr,
                 (const size_t*)v->d_off, (const size_t*)(v->d_off + v->cap), v->d_inv_tmp, v->d_pts, v->d_own, v->d_fixed, v->d_status);
    const size_t count = B * VF_OWN;
    PLONK_LAUNCH(g1_mul_many_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, (const G1Affine*)v->d_pts, (const Fr*)v->d_own, count,
                 v->d_prod);
    PLONK_LAUNCH(verify_fold_proof_kernel, dim3((unsigned)((2 * B + 63) / 64)), dim3(64), 0, s, (const G1Xyzz*)v->d_prod, B, v->d_lr);
    PLONK_CHECK_HIP(hipGetLastError());
    PLONK_CHECK_HIP(hipStreamSynchronize(s));
    v->batch = B;
    return PLONK_OK;
}

static int verifier_events(plonk_verifier* v, size_t n) {
    if (n <= v->n_evs) return PLONK_OK;
    hipEvent_t* evs = (hipEvent_t*)realloc(v->evs, n * sizeof(hipEvent_t));
    PLONK_REQUIRE(evs, PLONK_ERR_NOMEM, "realloc(%zu) failed", n * sizeof(hipEvent_t));
    v->evs = evs;
    for (; v->n_evs < n; v->n_evs++) PLONK_CHECK_HIP(hipEventCreate(&v->evs[v->n_evs]));
    return PLONK_OK;
}

static int verifier_init(plonk_verifier* v, plonk_ctx* ctx, unsigned K, const unsigned* log_n, const uint8_t* vk_xy_le, const size_t* n_public) {
    v->ctx = ctx;
    v->n_circuits = K;
    v->chal = challenge_consts();
    merlin_init(v->h_init[0], (const uint8_t*)"plonk", 5);
    v->h_init[1] = v->h_init[0];
    v->h_circ = (VfCircuit*)calloc(K, sizeof(VfCircuit));
    G1Affine* bases = (G1Affine*)calloc(8 * (size_t)K + 1, sizeof(G1Affine));
    int rc = v->h_circ && bases ? PLONK_OK : PLONK_ERR_NOMEM;
    if (rc != PLONK_OK) plonk_set_error("calloc failed for %u circuits", K);
    for (unsigned c = 0; c < K && rc == PLONK_OK; c++) {
        rc = [&]() -> int {
            PLONK_REQUIRE(log_n[c] >= 1 && log_n[c] <= PLONK_FR_TWO_ADICITY, PLONK_ERR_ARG, "circuit %u: group_order 2^%u out of range", c, log_n[c]);
            PLONK_REQUIRE(n_public[c] <= ((size_t)1 << log_n[c]), PLONK_ERR_ARG, "circuit %u: more public inputs than rows", c);
            VfCircuit& t = v->h_circ[c];
            t.log_n = log_n[c];
            t.n_public = (uint32_t)n_public[c];
            t.w = host_root_of_unity(log_n[c], false);
            t.w_inv = host_root_of_unity(log_n[c], true);
            t.n_inv = host_fp_inv_pow2<FrParams>(log_n[c]);
            for (int k = 0; k < 8; k++) {
                const uint8_t* q = vk_xy_le + 64 * (8 * (size_t)c + k);
                G1Affine& base = bases[8 * (size_t)c + k];
                PLONK_REQUIRE(le32_below_modulus(q, true) && le32_below_modulus(q + 32, true), PLONK_ERR_ARG, "circuit %u, verification key point %d: a coordinate is not below p", c, k);
                Fq x, y;
                memcpy(x.v, q, 32);
                memcpy(y.v, q + 32, 32);
                base.x = fp_to_mont(x);
                base.y = fp_to_mont(y);
                PLONK_REQUIRE(g1_affine_is_identity(base) || g1_affine_on_curve(base.x, base.y), PLONK_ERR_ARG, "circuit %u, verification key point %d is not on the curve", c, k);
            }
            return PLONK_OK;
        }();
    }
    if (rc == PLONK_OK) rc = [&]() -> int {
        G1Affine& g = bases[8 * (size_t)K];
        g.x = fp_one<FqParams>();  // G1 = (1, 2)
        g.y = fp_dbl(g.x);
        const size_t base_bytes = (8 * (size_t)K + 1) * sizeof(G1Affine);
        PLONK_TRY(dev_alloc((void**)&v->d_init, sizeof v->h_init));
        PLONK_TRY(dev_alloc((void**)&v->d_bases, base_bytes));
        PLONK_TRY(dev_alloc((void**)&v->d_circ, K * sizeof(VfCircuit)));
        PLONK_TRY(dev_alloc((void**)&v->d_partial, ((size_t)K + 1) * sizeof(G1Xyzz)));
        PLONK_TRY(dev_alloc((void**)&v->d_out, 4 * sizeof(Fq) + 16));
        PLONK_TRY(verifier_events(v, 1));
        PLONK_CHECK_HIP(hipMemcpy(v->d_bases, bases, base_bytes, hipMemcpyHostToDevice));
        PLONK_CHECK_HIP(hipMemcpy(v->d_circ, v->h_circ, K * sizeof(VfCircuit), hipMemcpyHostToDevice));
        return PLONK_OK;
    }();
    free(bases);
    return rc;
}

static int verifier_create(plonk_ctx* ctx, unsigned K, const unsigned* log_n, const uint8_t* vk_xy_le, const size_t* n_public, plonk_verifier** out) {
    plonk_verifier* v = new plonk_verifier();
    memset((void*)v, 0, sizeof *v);
    const int rc = verifier_init(v, ctx, K, log_n, vk_xy_le, n_public);
    if (rc != PLONK_OK) {
        plonk_verifier_destroy(v);
        return rc;
    }
    *out = v;
    return PLONK_OK;
}

extern "C" {

int plonk_verifier_create(plonk_ctx* ctx, unsigned log_n, const uint8_t vk_xy_le[8 * 64], size_t n_public, plonk_verifier** out) {
    PLONK_REQUIRE(ctx && vk_xy_le && out, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(ctx);
    return verifier_create(ctx, 1, &log_n, vk_xy_le, &n_public, out);
}

int plonk_verifier_create_multi(plonk_ctx* ctx, size_t n_circuits, const unsigned* log_n, const uint8_t* vk_xy_le, const size_t* n_public,
                                plonk_verifier** out) {
    PLONK_REQUIRE(ctx && log_n && vk_xy_le && n_public && out, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(n_circuits >= 1 && n_circuits <= PLONK_VERIFIER_MAX_CIRCUITS, PLONK_ERR_ARG, "%zu circuits: a table holds 1 to %d", n_circuits,
                  PLONK_VERIFIER_MAX_CIRCUITS);
    PLONK_ENTER(ctx);
    return verifier_create(ctx, (unsigned)n_circuits, log_n, vk_xy_le, n_public, out);
}

int plonk_verifier_destroy(plonk_verifier* v) {
    if (!v) return PLONK_OK;
    if (v->ctx) {
        plonk_use_device(v->ctx->device);
        hipStreamSynchronize(v->ctx->stream);
    }
    verifier_free_batch(v);
    dev_free_all({(void**)&v->d_init, (void**)&v->d_bases, (void**)&v->d_circ, (void**)&v->d_partial, (void**)&v->d_out, (void**)&v->d_lines});
    for (size_t i = 0; i < v->n_evs; i++) hipEventDestroy(v->evs[i]);
    free(v->evs);
    free(v->h_circ);
    free(v->h_meta);
    delete v;
    return PLONK_OK;
}

int plonk_verifier_load(plonk_verifier* v, const uint8_t* proofs, const uint8_t* public_le32, size_t batch, const uint8_t seed[32]) {
    PLONK_REQUIRE(v && proofs && batch && seed, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(v->n_circuits == 1, PLONK_ERR_STATE, "a verifier of %u circuits loads with plonk_verifier_load_multi", v->n_circuits);
    const size_t n_public = v->h_circ[0].n_public;
    PLONK_REQUIRE(public_le32 || !n_public, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(v->ctx);
    v->batch = 0;  // until the new batch is in place
    PLONK_TRY(verifier_ensure(v, batch, batch * n_public, batch * (n_public ? n_public : 1)));
    if (n_public) PLONK_TRY(plonk_fr_upload(v->ctx, v->d_pub, public_le32, batch * n_public));  // a value not below r: PLONK_ERR_ARG
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_proofs, proofs, batch * PROOF_BYTES, hipMemcpyHostToDevice, v->ctx->stream));
    return verifier_run(v, batch, seed, false);
}

int plonk_verifier_load_multi(plonk_verifier* v, const uint8_t* proofs, const uint32_t* circuit, const uint8_t* public_le32, size_t n_public_values,
                              size_t batch, const uint8_t seed[32]) {
    PLONK_REQUIRE(v && proofs && circuit && batch && seed, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(v->ctx);
    v->batch = 0;
    VfMeta m;
    PLONK_TRY(verifier_meta(v, batch, &m));
    size_t n_pub = 0, n_inv = 0;
    for (size_t b = 0; b < batch; b++) {
        PLONK_REQUIRE(circuit[b] < v->n_circuits, PLONK_ERR_ARG, "proof %zu: circuit %u of a table of %u", b, circuit[b], v->n_circuits);
        verifier_meta_set(v, m, b, circuit[b], &n_pub, &n_inv);
    }
    PLONK_REQUIRE(n_public_values == n_pub, PLONK_ERR_ARG, "%zu public values, the circuits of the batch take %zu", n_public_values, n_pub);
    PLONK_REQUIRE(public_le32 || !n_pub, PLONK_ERR_ARG, "bad argument");
    PLONK_TRY(verifier_ensure(v, batch, n_pub, n_inv));
    if (n_pub) PLONK_TRY(plonk_fr_upload(v->ctx, v->d_pub, public_le32, n_pub));  // a value not below r: PLONK_ERR_ARG
    PLONK_CHECK_HIP(hipMemcpyAsync(v->d_proofs, proofs, batch * PROOF_BYTES, hipMemcpyHostToDevice, v->ctx->stream));
    PLONK_TRY(verifier_meta_upload(v, batch, m));
    return verifier_run(v, batch, seed, true);
}

int plonk_verifier_load_prover(plonk_verifier* v, plonk_prover* p, size_t batch, const uint8_t seed[32]) {
    PLONK_REQUIRE(v && p && batch && seed, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(v->n_circuits == 1, PLONK_ERR_STATE, "a verifier of %u circuits loads with plonk_verifier_load_provers", v->n_circuits);
    const VfCircuit& c = v->h_circ[0];
    PLONK_REQUIRE(p->circuit.n_circuits == 1, PLONK_ERR_ARG, "a prover over a table of %u circuits is loaded with plonk_verifier_load_multi_prover", p->circuit.n_circuits);
    PLONK_REQUIRE(p->circuit.ctx->device == v->ctx->device, PLONK_ERR_ARG, "the prover lives on device %d, the verifier on %d", p->circuit.ctx->device, v->ctx->device);
    PLONK_REQUIRE(p->circuit.log_n == c.log_n && p->circuit.n_public == c.n_public, PLONK_ERR_ARG, "the prover's circuit (2^%u rows, %zu public inputs) is not the verifier's (2^%u, %u)",
                  p->circuit.log_n, p->circuit.n_public, c.log_n, c.n_public);
    PLONK_REQUIRE(batch == p->intake.resident_b, PLONK_ERR_STATE, "verify: batch %zu, but %zu proofs are resident in the prover", batch, p->intake.resident_b);
    PLONK_ENTER(v->ctx);
    v->batch = 0;
    PLONK_TRY(verifier_ensure(v, batch, batch * c.n_public, batch * (c.n_public ? c.n_public : 1)));
    // on the prover's stream, behind its five rounds.  The PROVER's status bytes land in d_status and are discarded on purpose
    // (verify_scalars_kernel overwrites them): a proof its prover flagged is verified like any other, and rejected
    PLONK_TRY(prover_pack_device(p, batch, 0, v->d_proofs, v->d_status, v->evs[0]));
    PLONK_CHECK_HIP(hipStreamWaitEvent(v->ctx->stream, v->evs[0], 0));
    if (c.n_public)
        PLONK_CHECK_HIP(hipMemcpyAsync(v->d_pub, p->intake.pub, batch * c.n_public * sizeof(Fr), hipMemcpyDeviceToDevice, v->ctx->stream));
    return verifier_run(v, batch, seed, false);
}

int plonk_verifier_load_provers(plonk_verifier* v, size_t n_provers, plonk_prover* const* provers, const uint32_t* circuit, const uint8_t seed[32]) {
    PLONK_REQUIRE(v && n_provers && provers && circuit && seed, PLONK_ERR_ARG, "bad argument");
    size_t batch = 0;
    for (size_t i = 0; i < n_provers; i++) {
        plonk_prover* p = provers[i];
        PLONK_REQUIRE(p, PLONK_ERR_ARG, "prover %zu is null", i);
        PLONK_REQUIRE(circuit[i] < v->n_circuits, PLONK_ERR_ARG, "prover %zu: circuit %u of a table of %u", i, circuit[i], v->n_circuits);
        const VfCircuit& c = v->h_circ[circuit[i]];
        PLONK_REQUIRE(p->circuit.n_circuits == 1, PLONK_ERR_ARG, "prover %zu is over a table of %u circuits: plonk_verifier_load_multi_prover loads it", i,
                      p->circuit.n_circuits);
        PLONK_REQUIRE(p->circuit.ctx->device == v->ctx->device, PLONK_ERR_ARG, "prover %zu lives on device %d, the verifier on %d", i, p->circuit.ctx->device, v->ctx->device);
        PLONK_REQUIRE(p->circuit.log_n == c.log_n && p->circuit.n_public == c.n_public, PLONK_ERR_ARG,
                      "prover %zu's circuit (2^%u rows, %zu public inputs) is not circuit %u of the table (2^%u, %u)", i, p->circuit.log_n, p->circuit.n_public,
                      circuit[i], c.log_n, c.n_public);
        PLONK_REQUIRE(p->intake.resident_b, PLONK_ERR_STATE, "prover %zu has no resident batch", i);
        batch += p->intake.resident_b;
    }
    PLONK_ENTER(v->ctx);
    v->batch = 0;
    VfMeta m;
    PLONK_TRY(verifier_meta(v, batch, &m));
    size_t n_pub = 0, n_inv = 0, b = 0;
    for (size_t i = 0; i < n_provers; i++)
        for (size_t j = 0; j < provers[i]->intake.resident_b; j++) verifier_meta_set(v, m, b++, circuit[i], &n_pub, &n_inv);
    PLONK_TRY(verifier_ensure(v, batch, n_pub, n_inv));
    PLONK_TRY(verifier_events(v, n_provers));
    // every prover packs its slice on its own stream, behind its five rounds (its status bytes are overwritten, as above)
    b = 0;
    for (size_t i = 0; i < n_provers; i++) {
        PLONK_TRY(prover_pack_device(provers[i], provers[i]->intake.resident_b, 0, v->d_proofs + b * PROOF_BYTES, v->d_status + b, v->evs[i]));
        b += provers[i]->intake.resident_b;
    }
    b = 0;
    for (size_t i = 0; i < n_provers; i++) {
        plonk_prover* p = provers[i];
        PLONK_CHECK_HIP(hipStreamWaitEvent(v->ctx->stream, v->evs[i], 0));
        if (p->circuit.n_public)
            PLONK_CHECK_HIP(hipMemcpyAsync(v->d_pub + m.pub_off[b], p->intake.pub, p->intake.resident_b * p->circuit.n_public * sizeof(Fr), hipMemcpyDeviceToDevice,
                                           v->ctx->stream));
        b += p->intake.resident_b;
    }
    PLONK_TRY(verifier_meta_upload(v, batch, m));
    return verifier_run(v, batch, seed, true);
}

// The resident batch of a prover over a table of circuits (plonk_prover_create_multi), packed on the device: proof b is labelled
// circuit_map[the prover's label of b], and its public row is the prover's, [l_max] wide at b * l_max, of which the verifier reads its
// circuit's own count.
int plonk_verifier_load_multi_prover(plonk_verifier* v, plonk_prover* p, const uint32_t* circuit_map, const uint8_t seed[32]) {
    PLONK_REQUIRE(v && p && circuit_map && seed, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(p->circuit.ctx->device == v->ctx->device, PLONK_ERR_ARG, "the prover lives on device %d, the verifier on %d", p->circuit.ctx->device, v->ctx->device);
    for (unsigned k = 0; k < p->circuit.n_circuits; k++) {
        PLONK_REQUIRE(circuit_map[k] < v->n_circuits, PLONK_ERR_ARG, "the prover's circuit %u: circuit %u of a table of %u", k, circuit_map[k], v->n_circuits);
        const VfCircuit& c = v->h_circ[circuit_map[k]];
        PLONK_REQUIRE(p->circuit.log_n == c.log_n && p->circuit.n_public_of[k] == c.n_public, PLONK_ERR_ARG,
                      "the prover's circuit %u (2^%u rows, %zu public inputs) is not circuit %u of the table (2^%u, %u)", k, p->circuit.log_n,
                      p->circuit.n_public_of[k], circuit_map[k], c.log_n, c.n_public);
    }
    const size_t batch = p->intake.resident_b, l_max = p->circuit.n_public;
    PLONK_REQUIRE(batch, PLONK_ERR_STATE, "the prover has no resident batch");
    PLONK_ENTER(v->ctx);
    v->batch = 0;
    VfMeta m;
    PLONK_TRY(verifier_meta(v, batch, &m));
    size_t n_pub = 0, n_inv = 0;
    for (size_t b = 0; b < batch; b++) {
        verifier_meta_set(v, m, b, circuit_map[p->labels.host[b]], &n_pub, &n_inv);
        m.pub_off[b] = b * l_max;  // the prover's rows are not ragged
    }
    PLONK_TRY(verifier_ensure(v, batch, batch * l_max, n_inv));
    PLONK_TRY(prover_pack_device(p, batch, 0, v->d_proofs, v->d_status, v->evs[0]));  // (its status bytes are overwritten, as above)
    PLONK_CHECK_HIP(hipStreamWaitEvent(v->ctx->stream, v->evs[0], 0));
    if (l_max) PLONK_CHECK_HIP(hipMemcpyAsync(v->d_pub, p->intake.pub, batch * l_max * sizeof(Fr), hipMemcpyDeviceToDevice, v->ctx->stream));
    PLONK_TRY(verifier_meta_upload(v, batch, m));
    return verifier_run(v, batch, seed, true);
}

int plonk_verifier_status(plonk_verifier* v, uint8_t* out_status) {
    PLONK_REQUIRE(v && out_status, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(v->batch, PLONK_ERR_STATE, "no batch is loaded");
    PLONK_ENTER(v->ctx);
    PLONK_CHECK_HIP(hipMemcpyAsync(out_status, v->d_status, v->batch, hipMemcpyDeviceToHost, v->ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(v->ctx->stream));
    return PLONK_OK;
}

int plonk_verifier_fold(plonk_verifier* v, size_t lo, size_t hi, uint8_t out_L[64], uint8_t out_R[64], uint8_t out_is_identity[2]) {
    PLONK_REQUIRE(v && out_L && out_R && out_is_identity, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(v->batch, PLONK_ERR_STATE, "no batch is loaded");
    PLONK_REQUIRE(lo <= hi && hi <= v->batch, PLONK_ERR_ARG, "fold: range [%zu, %zu) of a batch of %zu", lo, hi, v->batch);
    PLONK_ENTER(v->ctx);
    hipStream_t s = v->ctx->stream;
    uint8_t* d_flags = reinterpret_cast<uint8_t*>(v->d_out + 4);
    const unsigned K = v->n_circuits;
    if (K == 1) {  // every proof is of circuit 0, labelled or not
        PLONK_LAUNCH(verify_fold_kernel, dim3(1), dim3(VF_FOLD_THREADS), 0, s, (const G1Xyzz*)v->d_lr, (const Fr*)v->d_fixed, (const uint8_t*)v->d_status, lo, hi,
                     (const G1Affine*)v->d_bases, v->d_out, d_flags);
    } else {
        PLONK_LAUNCH(verify_fold_circuit_kernel, dim3(K), dim3(VF_FOLD_THREADS), 0, s, (const Fr*)v->d_fixed, (const uint8_t*)v->d_status,
                     (const uint32_t*)v->d_circuit, lo, hi, (const G1Affine*)v->d_bases, K, v->d_partial);
        PLONK_LAUNCH(verify_fold_multi_kernel, dim3(1), dim3(VF_FOLD_THREADS), 0, s, (const G1Xyzz*)v->d_lr, (const uint8_t*)v->d_status, lo, hi,
                     (const G1Xyzz*)v->d_partial, K + 1, v->d_out, d_flags);
    }
    PLONK_CHECK_HIP(hipGetLastError());
    PLONK_CHECK_HIP(hipMemcpyAsync(out_L, v->d_out, 64, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(out_R, v->d_out + 2, 64, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(out_is_identity, d_flags, 2, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipStreamSynchronize(s));
    return PLONK_OK;
}

int plonk_verifier_set_x2(plonk_verifier* v, const uint8_t x2_le[128]) {
    PLONK_REQUIRE(v && x2_le, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(v->ctx);
    Fq2 x, y;
    PLONK_TRY(pairing_g2_decode(x2_le, &x, &y));
    std::vector<PairingLine> lines(2 * PAIRING_ATE_LINES);
    pairing_line_table(x, y, lines.data());
    pairing_line_table(pairing_g2_generator_x(), pairing_g2_generator_y(), lines.data() + PAIRING_ATE_LINES);
    const size_t bytes = lines.size() * sizeof(PairingLine);
    PLONK_CHECK_HIP(hipStreamSynchronize(v->ctx->stream));  // a check over the old tables may be running
    if (!v->d_lines) PLONK_TRY(dev_alloc((void**)&v->d_lines, bytes));
    PLONK_CHECK_HIP(hipMemcpy(v->d_lines, lines.data(), bytes, hipMemcpyHostToDevice));
    return PLONK_OK;
}

int plonk_verifier_check_each(plonk_verifier* v, uint8_t* out_ok) {
    PLONK_REQUIRE(v && out_ok, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(v->d_lines, PLONK_ERR_STATE, "check_each: plonk_verifier_set_x2 has not been called");
    PLONK_REQUIRE(v->batch, PLONK_ERR_STATE, "no batch is loaded");
    PLONK_ENTER(v->ctx);
    const size_t B = v->batch, n_prod = B * VF_FIXED;
    void* buf;
    PLONK_TRY(ctx_scratch(v->ctx, 3, n_prod * sizeof(G1Xyzz) + 2 * B * sizeof(G1Affine) + B, &buf));
    G1Xyzz* d_prod = (G1Xyzz*)buf;
    G1Affine* d_pts = (G1Affine*)(d_prod + n_prod);
    uint8_t* d_ok = (uint8_t*)(d_pts + 2 * B);
    hipStream_t s = v->ctx->stream;
    // (per-kernel times for tools/verify_bench.py --each: no-ops unless the context is profiling)
    PLONK_TRY(prof_begin(v->ctx, "verify_each_fixed_products", (double)n_prod * sizeof(G1Xyzz)));
    PLONK_LAUNCH(verify_fixed_products_kernel, dim3((unsigned)((n_prod + 63) / 64)), dim3(64), 0, s, (const Fr*)v->d_fixed, (const uint8_t*)v->d_status,
                 v->n_circuits > 1 ? (const uint32_t*)v->d_circuit : (const uint32_t*)nullptr, (const G1Affine*)v->d_bases, v->n_circuits, B, d_prod);
    PLONK_LAUNCH(verify_own_points_kernel, dim3((unsigned)((2 * B + 63) / 64)), dim3(64), 0, s, (const G1Xyzz*)v->d_lr, (const G1Xyzz*)d_prod,
                 (const uint8_t*)v->d_status, B, d_pts);
    PLONK_CHECK_HIP(hipGetLastError());
    PLONK_TRY(prof_end(v->ctx));
    PLONK_TRY(prof_begin(v->ctx, "verify_each_pairings", (double)B * 2 * sizeof(G1Affine)));
    PLONK_TRY(pairing_check_fixed_launch(s, d_pts, v->d_lines, v->d_status, B, d_ok));
    PLONK_TRY(prof_end(v->ctx));
    PLONK_CHECK_HIP(hipMemcpyAsync(out_ok, d_ok, B, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipStreamSynchronize(s));
    return PLONK_OK;
}

int plonk_g1_mul_many(plonk_ctx* ctx, const uint8_t* h_xy_le, const uint8_t* h_scalars_le32, size_t count, uint8_t* h_out_xy_le, uint8_t* h_out_is_identity) {
    PLONK_REQUIRE(ctx && (count == 0 || (h_xy_le && h_scalars_le32 && h_out_xy_le && h_out_is_identity)), PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(ctx);
    if (!count) return PLONK_OK;
    void* buf;
    PLONK_TRY(ctx_scratch(ctx, 3, count * (2 * sizeof(Fq) + sizeof(Fr) + sizeof(G1Xyzz) + 2 * sizeof(Fq) + 1) + 64, &buf));
    Fq* d_xy = (Fq*)buf;
    Fr* d_k = (Fr*)(d_xy + 2 * count);
    G1Xyzz* d_prod = (G1Xyzz*)(d_k + count);
    Fq* d_out = (Fq*)(d_prod + count);
    uint32_t* d_bad = (uint32_t*)(d_out + 2 * count);
    uint8_t* d_flags = (uint8_t*)(d_bad + 4);
    hipStream_t s = ctx->stream;
    const dim3 grid((unsigned)((count + 63) / 64));
    PLONK_CHECK_HIP(hipMemcpyAsync(d_xy, h_xy_le, count * 64, hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(d_k, h_scalars_le32, count * 32, hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipMemsetAsync(d_bad, 0, 4, s));
    PLONK_LAUNCH(g1_mul_many_in_kernel, grid, dim3(64), 0, s, d_xy, (const Fr*)d_k, count, d_bad);
    PLONK_LAUNCH(g1_mul_many_kernel, grid, dim3(64), 0, s, (const G1Affine*)d_xy, (const Fr*)d_k, count, d_prod);
    PLONK_LAUNCH(g1_mul_many_out_kernel, grid, dim3(64), 0, s, (const G1Xyzz*)d_prod, count, d_out, d_flags);
    PLONK_CHECK_HIP(hipGetLastError());
    uint32_t bad = 0;
    PLONK_CHECK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(h_out_xy_le, d_out, count * 64, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(h_out_is_identity, d_flags, count, hipMemcpyDeviceToHost, s));
    PLONK_CHECK_HIP(hipStreamSynchronize(s));
    PLONK_REQUIRE(!(bad & 1), PLONK_ERR_ARG, "a coordinate is not below p, or a scalar not below r");
    PLONK_REQUIRE(!(bad & 2), PLONK_ERR_ARG, "a point is not on the curve");
    return PLONK_OK;
}

}  // extern "C"
