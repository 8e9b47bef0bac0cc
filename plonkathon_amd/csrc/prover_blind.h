// prover_blind.h — zero-knowledge blinding of the lock-step prover (included by prover.hip only; PLONK_PROVER_BLINDING).
//
// The PLONK paper's blinders b1..b11 (rounds 1-3 of its section 8.3) in split form: every blinded polynomial is
//     p = p0 + q Z_H,    Z_H = X^n - 1,
// with p0 of degree < n — what the n-vectors of the unblinded prover hold, untouched — and q a tail of at most six coefficients
// per proof that lives in a BlindState beside the ProofState.  Tails, low coefficient first, from the blinders b[0..10]:
//     a, b, c   [b1, b0], [b3, b2], [b5, b4]          z   [b8, b7, b6]
//     t_lo      [b9]     (and t_lo0[0]  += b9)
//     t_mid     [b10]    (and t_mid0[0] += b10 - b9)
//     t_hi      T4 = T[3n : 3n + 6], which is also added into t_hi0[0..5]  (and t_hi0[0] -= b10)
//     W_z, W_zw (X - x0)-quotients of the numerators' tails, five and two coefficients
// Everything here is a correction launched BESIDE the unblinded prover's kernels, which are not touched and not templated: a
// prover without the option launches none of this file.  A correction runs behind the scan or the MSM it corrects, on the same
// stream, so the one-workgroup and the segmented scans (prover_scans.h) are corrected alike and give the same bytes.
//   commitments   [p] = MSM(p0) + sum_k q_k H_k with the six fixed points H_k = [tau^(n+k)] - [tau^k]   (blind_commit_kernel)
//   round 3       on coset r Z_H is the constant zh_r: a(x) = A0(x) + (b0 x + b1) zh_r, ... added to the coset forms in place;
//                 deg t = 3n + 5, so FOUR cosets g mu^r H and a 4 x 4 combine                          (blind_coset / blind_combine)
//   round 4       a_eval = A0(zeta) + (b0 zeta + b1) Z_H(zeta), ..., z_shifted_eval = Z0(zeta w) + q_z(zeta w) Z_H(zeta)
//   round 5       numerator N = N0 + qN Z_H; W0 = quot(N0) + qN(x0) sum_i x0^(n-1-i) X^i, qW = (qN - qN(x0)) / (X - x0)
#pragma once
#include "prover.h"
#include "g1.h"

#define BLIND_COUNT 11  // blinders per proof
#define BLIND_TAIL 6    // coefficients of the longest tail (t_hi's)

struct BlindState {
    Fr b[BLIND_COUNT];       // the blinders (Montgomery)
    Fr q_hi[BLIND_TAIL];     // T4, round 3
    Fr q_w[2][BLIND_TAIL];   // tails of W_z (five coefficients) and W_zw (two), zero above; round 5
    Fr e[2];                 // qN(zeta), q_z(zeta w): the factors of the geometric rows added to W_z0, W_zw0
};

// tail of proof record point `point` (PROOF_POINTS order) -> q[0..BLIND_TAIL), zero padded
PLONK_DEV void blind_tail(const BlindState& s, unsigned point, Fr q[BLIND_TAIL]) {
    const Fr zero = fp_zero<FrParams>();
    for (int k = 0; k < BLIND_TAIL; k++) q[k] = zero;
    if (point < 3) {
        q[0] = s.b[2 * point + 1];
        q[1] = s.b[2 * point];
    } else if (point == 3) {
        q[0] = s.b[8];
        q[1] = s.b[7];
        q[2] = s.b[6];
    } else if (point == 4) {
        q[0] = s.b[9];
    } else if (point == 5) {
        q[0] = s.b[10];
    } else if (point == 6) {
        for (int k = 0; k < BLIND_TAIL; k++) q[k] = s.q_hi[k];
    } else {
        for (int k = 0; k < BLIND_TAIL; k++) q[k] = s.q_w[point - 7][k];
    }
}
// q(x) of a tail, Horner
PLONK_DEV Fr blind_tail_eval(const Fr q[BLIND_TAIL], const Fr& x) {
    Fr acc = q[BLIND_TAIL - 1];
    for (int k = BLIND_TAIL - 2; k >= 0; k--) acc = fp_add(fp_mul(acc, x), q[k]);
    return acc;
}

// ------------------------------------------------------------------------------------------------
// The blinders.  Explicit ones (plonk_prover_set_blinders) are copied in; seeded ones are drawn on the device: per proof a
// Merlin transcript "plonk-blinding" absorbs seed, run counter and proof index and gives eleven wide challenges "b".
__global__ void blind_load_kernel(const Fr* explicit_b, size_t B, BlindState* bs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * BLIND_COUNT) bs[i / BLIND_COUNT].b[i % BLIND_COUNT] = fp_load(explicit_b + i);
}

struct BlindSeed { uint8_t seed[32]; unsigned long long run; };
__global__ void __launch_bounds__(2 * TC_LANES) blind_derive_kernel(BlindSeed in, size_t B, ChallengeConsts cc, BlindState* bs) {
    __shared__ TcShared shared[2];
    const unsigned grp = threadIdx.x / TC_LANES, lane = threadIdx.x % TC_LANES;
    TcShared& sh = shared[grp];
    size_t b = (size_t)blockIdx.x * 2 + grp;
    const bool live = b < B;
    if (!live) b = B - 1;  // as transcript_kernel: the barriers stay uniform, nothing is stored
    TcState t;
    t.w = 0;
    t.pos = t.pos_begin = 0;
    sh.msg[lane] = in.seed[lane];                                                                   // 32 lanes, 32 bytes
    if (lane < 8) sh.msg[32 + lane] = (uint8_t)(in.run >> (8 * lane));
    else if (lane < 16) sh.msg[32 + lane] = (uint8_t)((unsigned long long)b >> (8 * (lane - 8)));
    __syncthreads();
    tc_open(t, sh, lane, "plonk-blinding", 14);
    tc_append_message(t, sh, lane, "seed", 4, sh.msg, 32);
    tc_append_message(t, sh, lane, "run", 3, sh.msg + 32, 8);
    tc_append_message(t, sh, lane, "index", 5, sh.msg + 40, 8);
    for (int k = 0; k < BLIND_COUNT; k++) {
        const Fr f = tc_challenge_wide(t, sh, lane, cc, "b", 1);
        if (live && lane == 0) bs[b].b[k] = f;
    }
}

// ------------------------------------------------------------------------------------------------
// Commitment corrections.  The six H_k are fixed, so a tail's scalar multiplications are cut into 16-bit windows over a table
// of 2^(16 w) H_k: a lane owns one (term, window) pair — sixteen doublings and at most sixteen mixed additions instead of 254
// and 127 — and the 8 x 16 lanes of a workgroup sum their shares in LDS, add the commitment MSM(p0) left in the record and
// write the affine point back.  One workgroup (two waves) per (proof, point): B = 512 gives rounds 1 and 3 3 072 waves, round
// 5 2 048 and round 2 1 024 on the 1 024 SIMDs, each a chain of ~32 group operations and a seven-level tree.  One lane per
// (proof, point) running a joint double-and-add would be 12 waves per round at that batch, each 254 doublings long.
#define BLIND_WIN_BITS 16
#define BLIND_WINDOWS 16   // 16 x 16 bits >= 254
#define BLIND_TERMS 8      // term slots of a workgroup (six used at most)
#define BLIND_LANES (BLIND_TERMS * BLIND_WINDOWS)

// htab[k * BLIND_WINDOWS + w] = 2^(16 w) ([tau^(n+k)] - [tau^k]), affine, Montgomery.  Once per option switch: one lane per entry.
__global__ void blind_h_kernel(const G1Affine* bases, size_t n, G1Affine* htab) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= BLIND_TAIL * BLIND_WINDOWS) return;
    const unsigned k = j / BLIND_WINDOWS, w = j % BLIND_WINDOWS;
    G1Affine hi, lo;
    hi.x = fp_load(&bases[n + k].x);
    hi.y = fp_load(&bases[n + k].y);
    lo.x = fp_load(&bases[k].x);
    lo.y = fp_load(&bases[k].y);
    G1Xyzz acc = g1_xyzz_from_affine(hi);
    g1_madd<true>(acc, g1_affine_is_identity(lo) ? lo : g1_affine_neg(lo));
    for (unsigned d = 0; d < BLIND_WIN_BITS * w; d++) g1_dbl(acc);
    const G1Affine a = g1_to_affine(acc);
    fp_store(&htab[j].x, a.x);
    fp_store(&htab[j].y, a.y);
}

// grid (B, count): points first_point .. first_point + count - 1 of every proof record
__global__ void __launch_bounds__(BLIND_LANES) blind_commit_kernel(const BlindState* bs, const G1Affine* htab, unsigned first_point, size_t B, Fq* commit_xy,
                                                                    uint8_t* flags) {
    PLONK_SHORT_KERNEL();
    __shared__ G1Xyzz red[BLIND_LANES];
    const size_t b = blockIdx.x;
    const unsigned point = first_point + blockIdx.y, tid = threadIdx.x, term = tid / BLIND_WINDOWS, win = tid % BLIND_WINDOWS;
    G1Xyzz acc = g1_xyzz_identity();
    if (term < BLIND_TAIL) {
        Fr q[BLIND_TAIL];
        blind_tail(bs[b], point, q);
        Fr sel = q[0];
        for (unsigned k = 1; k < BLIND_TAIL; k++)
            if (k == term) sel = q[k];
        const Fr c = fp_from_mont(sel);  // canonical: the windows are bits of the integer
        const uint32_t digit = (c.v[win / 2] >> (16 * (win & 1))) & 0xffffu;
        if (digit) {
            G1Affine h;
            h.x = fp_load(&htab[term * BLIND_WINDOWS + win].x);
            h.y = fp_load(&htab[term * BLIND_WINDOWS + win].y);
            for (int bit = BLIND_WIN_BITS - 1; bit >= 0; bit--) {
                g1_dbl(acc);
                if ((digit >> bit) & 1u) g1_madd<true>(acc, h);
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (unsigned s = BLIND_LANES / 2; s > 0; s >>= 1) {
        if (tid < s) {
            G1Xyzz x = red[tid];
            g1_add(x, red[tid + s]);
            red[tid] = x;
        }
        __syncthreads();
    }
    if (tid) return;
    G1Xyzz sum = red[0];
    if (g1_is_identity(sum)) return;  // a zero tail: the record keeps MSM(p0) as it is
    const size_t m = (size_t)point * B + b;
    if (!flags[m]) {
        G1Affine c0;
        c0.x = fp_to_mont(fp_load(commit_xy + 2 * m));
        c0.y = fp_to_mont(fp_load(commit_xy + 2 * m + 1));
        g1_madd<true>(sum, c0);
    }
    const G1Affine a = g1_to_affine(sum);
    flags[m] = g1_affine_is_identity(a) ? 1 : 0;
    fp_store(commit_xy + 2 * m, fp_from_mont(a.x));
    fp_store(commit_xy + 2 * m + 1, fp_from_mont(a.y));
}

// ------------------------------------------------------------------------------------------------
// Round 3.  big = A, B, C, PI, Z on the four cosets, [5][B][4n] coset-major; point k = r n + j is x = xs[k], where Z_H = zh.v[r].
// Z(w x) is read from the same row one place ahead inside the coset (quotient_kernel), so correcting Z's row corrects both.
struct BlindZh { Fr v[4]; };
__global__ void blind_coset_kernel(const BlindState* bs, const Fr* xs, BlindZh zh, unsigned log_n, size_t B, Fr* big) {
    PLONK_SHORT_KERNEL();
    const size_t n4 = (size_t)4 << log_n, total = B * n4;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n4, k = gI - b * n4;
        const BlindState& s = bs[b];
        const Fr x = fp_load(xs + k), z = zh.v[k >> log_n];
        for (int p = 0; p < 3; p++) {
            Fr* v = big + (size_t)p * total + gI;
            fp_store(v, fp_add(fp_load(v), fp_mul(fp_add(fp_mul(s.b[2 * p], x), s.b[2 * p + 1]), z)));
        }
        Fr* v = big + 4 * total + gI;
        const Fr qz = fp_add(fp_mul(fp_add(fp_mul(s.b[6], x), s.b[7]), x), s.b[8]);
        fp_store(v, fp_add(fp_load(v), fp_mul(qz, z)));
    }
}

// The quotient's 3n + 6 coefficients from its values on four cosets, then the fold.  As quotient_combine_kernel: slice r of
// quot[b] holds u_r[i] / 2 with u_r = sum_k (g^n i^r)^k T_k[i], k < 4 (i = mu^n, i^4 = 1), so
//     T_k[i] = (1 / 2 g^kn) sum_r i^(-rk) (u_r[i] / 2):
//     T_0 = (s + t) / 2,  T_2 = (s - t) / 2 g^2n         s = h_0 + h_2,  t = h_1 + h_3
//     T_1 = (d - i e) / 2 g^n,  T_3 = (d + i e) / 2 g^3n  d = h_0 - h_2,  e = h_1 - h_3
// In place: slices 0..2 <- t_lo0, t_mid0, t_hi0 (the table at the top of this file), T_3[0..5] -> BlindState::q_hi; slice 3 is
// not read again.  With all blinders zero T_3 is zero and the three slices are quotient_combine_kernel's residues.
struct BlindCombine { Fr ci, half, g1h, g2h, g3h; };  // i, 1/2, 1 / 2 g^n, 1 / 2 g^2n, 1 / 2 g^3n
__global__ void blind_combine_kernel(Fr* quot, size_t n, size_t stride, size_t B, BlindCombine k, BlindState* bs) {
    PLONK_SHORT_KERNEL();
    const size_t total = B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n, i = gI - b * n;
        Fr* q = quot + b * stride + i;
        const Fr h0 = fp_load(q), h1 = fp_load(q + n), h2 = fp_load(q + 2 * n), h3 = fp_load(q + 3 * n);
        const Fr s = fp_add(h0, h2), t = fp_add(h1, h3), d = fp_sub(h0, h2), ie = fp_mul(k.ci, fp_sub(h1, h3));
        Fr t0 = fp_mul(fp_add(s, t), k.half), t1 = fp_mul(fp_sub(d, ie), k.g1h), t2 = fp_mul(fp_sub(s, t), k.g2h);
        if (i < BLIND_TAIL) {
            const Fr t3 = fp_mul(fp_add(d, ie), k.g3h);
            t2 = fp_add(t2, t3);
            bs[b].q_hi[i] = t3;
            if (i == 0) {
                const Fr b9 = bs[b].b[9], b10 = bs[b].b[10];
                t0 = fp_add(t0, b9);
                t1 = fp_add(t1, fp_sub(b10, b9));
                t2 = fp_sub(t2, b10);
            }
        }
        fp_store(q, t0);
        fp_store(q + n, t1);
        fp_store(q + 2 * n, t2);
    }
}

// ------------------------------------------------------------------------------------------------
// Round 4, one lane per proof, behind the evaluation scan: s1_eval, s2_eval and PI(zeta) stay.  (zeta w)^n = zeta^n.
__global__ void __launch_bounds__(64) blind_evals_kernel(const BlindState* bs, ProofState* st, Fr w, unsigned log_n, size_t B) {
    PLONK_SHORT_KERNEL();
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const BlindState& s = bs[b];
    const Fr zeta = st[b].zeta, zw = fp_mul(zeta, w);
    Fr zn = zeta;
    for (unsigned i = 0; i < log_n; i++) zn = fp_sqr(zn);
    const Fr zh = fp_sub(zn, fp_one<FrParams>());
    for (int p = 0; p < 3; p++) st[b].evals[p] = fp_add(st[b].evals[p], fp_mul(fp_add(fp_mul(s.b[2 * p], zeta), s.b[2 * p + 1]), zh));
    const Fr qz = fp_add(fp_mul(fp_add(fp_mul(s.b[6], zw), s.b[7]), zw), s.b[8]);
    st[b].evals[5] = fp_add(st[b].evals[5], fp_mul(qz, zh));
}

// Round 5, one lane per proof, behind linearisation_weights_kernel (whose weights already carry the blinded evaluations):
//     qN = w_Z q_z + w_T1 q_lo + w_T2 q_mid + w_T3 q_hi + v q_a + v^2 q_b + v^3 q_c      (LinWeights order: 5, 7, 8, 9, 10, 11, 12)
// for W_z and qN = q_z for W_zw; per opening e = qN(x0) and qW = (qN - e) / (X - x0) by synthetic division.  lin_w: [B][15].
__global__ void __launch_bounds__(64) blind_openings_kernel(BlindState* bs, const ProofState* st, const Fr* lin_w, Fr w, size_t B) {
    PLONK_SHORT_KERNEL();
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    BlindState& s = bs[b];
    const Fr* lw = lin_w + 15 * b;
    const unsigned src[7] = {3, 4, 5, 6, 0, 1, 2}, wi[7] = {5, 7, 8, 9, 10, 11, 12};
    Fr qn[2][BLIND_TAIL];
    for (int k = 0; k < BLIND_TAIL; k++) qn[0][k] = fp_zero<FrParams>();
    for (int t = 0; t < 7; t++) {
        Fr q[BLIND_TAIL];
        blind_tail(s, src[t], q);
        const Fr wt = fp_load(lw + wi[t]);
        for (int k = 0; k < BLIND_TAIL; k++) qn[0][k] = fp_add(qn[0][k], fp_mul(wt, q[k]));
    }
    blind_tail(s, 3, qn[1]);
    for (int z = 0; z < 2; z++) {
        const Fr x0 = z ? fp_mul(st[b].zeta, w) : st[b].zeta;
        Fr carry = fp_zero<FrParams>();  // q_{k-1} = p_k + x0 q_k from the top; the last carry is the remainder qN(x0)
        for (int k = BLIND_TAIL - 1; k >= 0; k--) {
            const Fr next = fp_add(qn[z][k], fp_mul(x0, carry));
            s.q_w[z][k] = carry;
            carry = next;
        }
        s.e[z] = carry;
    }
}

// W0[i] += e x0^(n - 1 - i) for both openings, behind the division scan: grid (n / (8 x 256), B, 2), eight rows per lane.
#define BLIND_ROWS_PER_LANE 8
__global__ void __launch_bounds__(256) blind_division_kernel(const BlindState* bs, const ProofState* st, Fr w, size_t n, size_t B, Fr* wz) {
    PLONK_SHORT_KERNEL();
    const size_t b = blockIdx.y, z = blockIdx.z;
    const size_t lo = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * BLIND_ROWS_PER_LANE;
    if (lo >= n) return;
    const size_t hi = lo + BLIND_ROWS_PER_LANE < n ? lo + BLIND_ROWS_PER_LANE : n;
    const Fr x0 = z ? fp_mul(st[b].zeta, w) : st[b].zeta;
    Fr term = fp_mul(bs[b].e[z], fp_pow_u64(x0, (uint64_t)(n - hi)));
    Fr* row = wz + (z * B + b) * n;
    for (size_t i = hi; i-- > lo;) {
        fp_store(row + i, fp_add(fp_load(row + i), term));
        term = fp_mul(term, x0);
    }
}
