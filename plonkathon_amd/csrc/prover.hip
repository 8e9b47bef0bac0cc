// prover.hip — the batched, GPU-resident five-round PLONK prover (plonk_prover_*).
//
// Reference behaviour replaced: Prover.prove / round_1..round_5 (/root/reference/prover.py:51-306,
// spec in SURVEY.md §3.2) for B independent proofs of one circuit run in lock-step, including the
// Fiat-Shamir transcript (transcript.py:77-123), which runs on the device (32 lanes per proof) so
// that a whole batch is one uninterrupted stream of kernel launches with no host round trip.  A prover over a TABLE of circuits of
// one group order (plonk_prover_create_multi) labels every proof with its circuit: only the kernels that read the fixed polynomials
// or the wiring take the label array (null for a table of one, which is plonk_prover_create's prover), the rest never see the circuit.
//
// Every committed polynomial is uniquely determined by (circuit, witness, challenges) — the
// reference adds no blinding (README.md:31-32); PLONK_PROVER_BLINDING adds the PLONK paper's as correction launches beside these
// kernels (prover_blind.h) — so the schedule is free to differ from the
// reference's as long as the polynomials are the same:
//   * the coset offset used for the quotient is a FIXED generator g = 5 instead of the per-proof
//     `fft_cofactor` challenge (which is still drawn, to keep the transcript identical); the
//     circuit's selector / permutation polynomials are therefore extended ONCE per circuit;
//   * coset extensions start from the coefficient forms the commitments already produced;
//   * T1..T3 are committed straight from the quotient's coefficient slices (commit(fft(c)) = MSM(c));
//   * round 4 evaluates coefficient forms by a blocked Horner; round 5 builds the opening
//     polynomials in coefficient form (linear combination + synthetic division by X - z), so the
//     reference's ~15 further coset extensions and its 4n-point divisions never happen.
#include <assert.h>
#include <string.h>

#include <array>
#include <vector>

#include "prover.h"
#include "g1_codec.h"
#include "prover_scans.h"  // rounds 2, 4 and 5: the grand product, the evaluations, the divisions — kernels and launchers
#include "prover_intake.h"  // a batch from the caller's bytes to resident witnesses: the uploads, the wiring, the witness solver
#include "prover_blind.h"  // PLONK_PROVER_BLINDING: the blinders, the tails and every correction they add beside the kernels of this file

// ------------------------------------------------------------------------------------------------
// Sparse public inputs.  PI = sum_{i < l} (-pub_i) L_i with L_i the Lagrange basis of the n-th roots of unity:
//   coefficient j of L_i is  w^(-ij) / n            (an inverse DFT of a unit vector)
//   L_i(x) = (w^i / n) (x^n - 1) / (x - w^i)        (li_big holds it on the coset points: [3][n] coset-major)
__global__ void pi_coeffs_kernel(const Fr* pub, size_t l, const Fr* roots_inv, size_t n, size_t B, Fr n_inv, Fr* pic) {
    PLONK_SHORT_KERNEL();
    const size_t total = B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n, j = gI - b * n;
        Fr acc = fp_zero<FrParams>();
        for (size_t i = 0; i < l; i++) acc = fp_add(acc, fp_mul(fp_load(pub + b * l + i), fp_load(roots_inv + ((i * j) & (n - 1)))));
        fp_store(pic + gI, fp_neg(fp_mul(acc, n_inv)));
    }
}
__global__ void pi_coset_kernel(const Fr* pub, size_t l, const Fr* li_big, size_t n4, size_t B, Fr* pi_big) {
    PLONK_SHORT_KERNEL();
    const size_t total = B * n4;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n4, k = gI - b * n4;
        Fr acc = fp_zero<FrParams>();
        for (size_t i = 0; i < l; i++) acc = fp_add(acc, fp_mul(fp_load(pub + b * l + i), fp_load(li_big + i * n4 + k)));
        fp_store(pi_big + gI, fp_neg(acc));
    }
}
// li[i][k] = (w^i / n) zh[k / n] / (x_k - w^i), k = r n + j (Z_H is constant on coset r); one field inversion per entry, once per circuit
struct Zh4 { Fr v[4]; };
__global__ void li_coset_kernel(const Fr* xs, const Fr* roots, size_t n4, size_t n, size_t l, Zh4 zh, Fr n_inv, Fr* li) {
    const size_t total = l * n4;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t i = gI / n4, k = gI - i * n4;
        const Fr wi = fp_load(roots + i);
        const Fr num = fp_mul(fp_mul(wi, n_inv), zh.v[k / n]);
        fp_store(li + gI, fp_mul(num, fp_inv(fp_sub(fp_load(xs + k), wi))));  // x_k is never an n-th root of unity
    }
}

// ------------------------------------------------------------------------------------------------
// One transcript round of every proof (transcript_device.h): the round's commitments, or evaluations, are staged big-endian in
// sh.msg; an identity commitment (flag set) is absorbed as zeros and reported through `error`.
// Round 0 also opens the batch's failure flags: it zeroes the proof's word of gate_fail (plonk_prover::Rounds::closes + B), which
// gate_check_kernel, the next kernel on the stream, ORs into — one dispatch fewer per batch than a memset in between.
__global__ void __launch_bounds__(2 * TC_LANES) transcript_kernel(int round, ProofState* st, size_t B, const Fq* commit_xy,
                                                                  const uint8_t* flags, ChallengeConsts cc, uint32_t* gate_fail) {
    PLONK_SHORT_KERNEL();
    __shared__ TcShared shared[2];
    const unsigned grp = threadIdx.x / TC_LANES, lane = threadIdx.x % TC_LANES;
    TcShared& sh = shared[grp];
    size_t b = (size_t)blockIdx.x * 2 + grp;
    const bool live = b < B;
    if (!live) b = B - 1;  // shadow the last proof so the barriers stay uniform; nothing is stored
    ProofState& s = st[b];
    TcState t = tc_load(s.transcript, lane);
    uint32_t error = 0;
    Fr c0 = fp_zero<FrParams>(), c1 = fp_zero<FrParams>();

    if (round >= 1 && round <= 3) {  // slots 0..2, 3, 4..6: x and y of each commitment
        const unsigned first_slot = round == 1 ? 0 : round == 2 ? 3 : 4, count = round == 2 ? 1 : 3;
        if (lane < 2 * count) {
            const size_t slot = (size_t)first_slot + lane / 2;
            const uint8_t fl = flags[slot * B + b];
            Fq v = fp_load(commit_xy + 2 * (slot * B + b) + (lane & 1));
            if (fl) {
                v = fp_zero<FqParams>();
                error = 1;
            }
            limbs_to_be32(v.v, sh.msg + 32 * lane);
        }
    } else if (round == 4 && lane < PROOF_EVALS) {
        Fr e = fp_from_mont(s.evals[lane]);
        limbs_to_be32(e.v, sh.msg + 32 * lane);
    }
    __syncthreads();
    tc_round(t, sh, lane, cc, round, c0, c1);
    if (!live) return;
    tc_store(t, lane, s.transcript);
    // `error` was raised by the lanes that staged a flagged coordinate
    if (error) s.error = 1;
    if (lane == 0) {
        if (round == 0) {
            s.error = 0;
            gate_fail[b] = 0;  // gate_check_kernel, next on the stream, only ever ORs into the word
        }
        if (round == 1) { s.beta = c0; s.gamma = c1; }
        if (round == 2) { s.alpha = c0; s.fft_cofactor = c1; }
        if (round == 3) s.zeta = c0;
        if (round == 4) s.v = c0;
    }
}

// ------------------------------------------------------------------------------------------------
// Round 3 (prover.py:188-203): quotient evaluations on the coset points, fully fused.
//   wit = A, B, C, PI, Z on the points, proof b at + b n4; fixed = QM, QL, QR, QO, QC, S1, S2, S3 (FX_* order), l0, xs: [n4].
//   Challenges from the transcript states (st) or, st == null, from `direct` (plonk_fr_quotient).
//   coset_log == 0: the reference's layout — n4 = 4n points g mu^k in natural order, Z(w x) four places ahead (prover.py:173),
//   Z_H by k & 3 (plonk_fr_quotient).  coset_log == log2 n: the lock-step prover's — n4 = 3n points [r][j] = g mu^r w^j, Z(w x)
//   one place ahead INSIDE the coset, Z_H by r.  The quotient goes to quot[b * out_stride + k].
struct ZhInv { Fr v[4]; };
//   A table of circuits (cid != null): proof b reads fixed[k] + cid[b] * fixed_stride.
struct QuotientIn { const Fr* wit[5]; const Fr* fixed[FX_COUNT]; const Fr* l0; const Fr* xs; const uint32_t* cid; unsigned fixed_stride; };
// Round 4: the arithmetic runs on lazy limbs (fpl.h) — operands stay unpacked between the 19 products of a point, the gate's
// four products share two reductions (fpl_mul_add), sums of two are multiplied as they stand and only the seven sums of three
// or more are carry-swept: ~4 800 instructions per point against ~5 800 on packed residues.  Bounds, in units of m, beside
// each line ("n" = normalised: limbs 0..7 in [0, 2^29)); the emulator build asserts them on every operand.
__global__ void PLONK_BESIDE_ACC(256, 64) quotient_kernel(QuotientIn in, ZhInv zh, const ProofState* st, RoundChallenges direct, unsigned n4, Fr* quot,
                                                       unsigned coset_log, unsigned out_stride) {
    PLONK_WORK_KERNEL();
    typedef FpL<FrParams> L;
    // blockIdx.y = proof, blockIdx.x * blockDim.x + threadIdx.x = point (32-bit indices, no divisions)
    const unsigned b = blockIdx.y;
    // the challenges are the same for every lane of the block: limbs in scalar registers
    const L beta = fpl_from_fp_uniform(st ? st[b].beta : direct.beta), gamma = fpl_from_fp_uniform(st ? st[b].gamma : direct.gamma),
            alpha = fpl_from_fp_uniform(st ? st[b].alpha : direct.alpha);                                   // n, [0, 1)
    const L one = fpl_one<FrParams>();
    const size_t row = (size_t)b * n4;
    const size_t fx = in.cid ? (size_t)in.cid[b] * in.fixed_stride : 0;  // the proof's circuit: the same for the block, like the challenges
    for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += gridDim.x * blockDim.x) {
        const unsigned cr = coset_log ? k >> coset_log : 0u, cmask = coset_log ? (1u << coset_log) - 1u : 0u;
        const unsigned kw = coset_log ? ((k & ~cmask) | ((k + 1) & cmask))            // the next point of the same coset
                                      : ((k + 4 < n4) ? k + 4 : k + 4 - n4);          // Z(w x) = Z_big.shift(4), prover.py:173
        const auto ld = [&](const Fr* p) PLONK_LAMBDA_INLINE { return fpl_from_fp(fp_load(p)); };          // n, [0, 1)
        const L a = ld(in.wit[0] + row + k), bb = ld(in.wit[1] + row + k), c = ld(in.wit[2] + row + k);
        // gate: A QL + B QR + A B QM + C QO + PI + QC
        const L t1 = fpl_mul_add(a, ld(in.fixed[FX_QL] + fx + k), bb, ld(in.fixed[FX_QR] + fx + k));               // n, (-1, 2)
        const L ab = fpl_mul(a, bb);                                                                       // n, (-1, 2)
        const L t2 = fpl_mul_add(ab, ld(in.fixed[FX_QM] + fx + k), c, ld(in.fixed[FX_QO] + fx + k));               // n, (-1, 2)
        const L gate = fpl_norm(fpl_add(fpl_add(t1, t2), fpl_add(ld(in.wit[3] + row + k), ld(in.fixed[FX_QC] + fx + k))));  // four terms: limbs < 2^31; n, (-2, 6)
        // permutation: (A + g + b x)(B + g + 2 b x)(C + g + 3 b x) Z - (A + g + b S1)(B + g + b S2)(C + g + b S3) Z(w x)
        const L bx = fpl_mul(beta, ld(in.xs + k));                                                         // n, (-1, 2)
        const L u1 = fpl_norm(fpl_add(gamma, bx));                                                         // n, (-1, 3)
        const L u2 = fpl_norm(fpl_add(u1, bx));                                                            // n, (-2, 5)
        const L u3 = fpl_norm(fpl_add(u2, bx));                                                            // n, (-3, 7)
        const L z = ld(in.wit[4] + row + k);
        L p1 = fpl_mul(fpl_add(a, u1), z);                                                                 // (two terms) x n: |.| < 4;  n, (-1, 2)
        p1 = fpl_mul(fpl_add(bb, u2), p1);                                                                 // < 6 x 2
        p1 = fpl_mul(fpl_add(c, u3), p1);                                                                  // < 8 x 2
        const L v1 = fpl_norm(fpl_add(gamma, fpl_mul(beta, ld(in.fixed[FX_S1] + fx + k))));                     // n, (-1, 3)
        L p2 = fpl_mul(fpl_add(a, v1), ld(in.wit[4] + row + kw));                                          // < 4 x 1
        const L v2 = fpl_norm(fpl_add(gamma, fpl_mul(beta, ld(in.fixed[FX_S2] + fx + k))));
        p2 = fpl_mul(fpl_add(bb, v2), p2);                                                                 // < 4 x 2
        const L v3 = fpl_norm(fpl_add(gamma, fpl_mul(beta, ld(in.fixed[FX_S3] + fx + k))));
        p2 = fpl_mul(fpl_add(c, v3), p2);
        // (Z - 1) L0, and the sum under alpha
        const L first = fpl_mul(fpl_sub(z, one), ld(in.l0 + k));                     // difference x n;  n, (-1, 2)
        const L inner = fpl_add(fpl_sub(p1, p2), fpl_mul(alpha, first));                                   // limbs within (-2^29, 2^30); (-4, 5)
        const L acc = fpl_add(gate, fpl_mul(alpha, inner));                                                // two n terms; (-3, 8)
        L zhi;
        if (coset_log >= 6) zhi = fpl_from_fp_uniform(zh.v[cr]);  // a wave's 64 points lie in one coset (64 | n): scalar registers
        else zhi = fpl_from_fp(zh.v[coset_log ? cr : (k & 3)]);
        fp_store(quot + (size_t)b * out_stride + k, fpl_pack_canonical(fpl_mul(acc, zhi)));
    }
}

// The quotient's coefficients from its values on three cosets.  With t = T_0 + X^n T_1 + X^2n T_2 (deg T_q < n) and
// x^n = g^n i^r on coset r (i = mu^n, a primitive fourth root of unity), the polynomial U_r = T_0 + (g^n i^r) T_1 + (g^n i^r)^2 T_2
// agrees with t on coset r; the size-n inverse transforms (with their (g mu^r)^-i store-side scaling, which also halves)
// leave u_r[i] / 2 in slice r of quot.  Per i, with s_1 = g^n t_{n+i}, s_2 = g^2n t_{2n+i}:
//   u_0 = t_i + s_1 + s_2,   u_1 = t_i + i s_1 - s_2,   u_2 = t_i - s_1 + s_2
//   =>  s_1 = u_0/2 - u_2/2,   p = t_i + s_2 = u_0/2 + u_2/2,   m = t_i - s_2 = u_1 - i s_1,   t_i = (p + m)/2,  s_2 = (p - m)/2.
// in place: slice q of quot[b] <- T_q.  Three multiplications per i (by i, 1/g^n, 1/(2 g^2n)) and a halving.
__global__ void quotient_combine_kernel(Fr* quot, size_t n, size_t stride, size_t B, Fr ci, Fr g1_inv, Fr g2_inv_half, Fr half) {
    PLONK_SHORT_KERNEL();
    const size_t total = B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n, i = gI - b * n;
        Fr* q = quot + b * stride + i;
        const Fr h0 = fp_load(q), h1 = fp_load(q + n), h2 = fp_load(q + 2 * n);  // u_r / 2
        const Fr s1 = fp_sub(h0, h2), p = fp_add(h0, h2);
        const Fr m = fp_sub(fp_dbl(h1), fp_mul(ci, s1));
        fp_store(q, fp_mul(fp_add(p, m), half));
        fp_store(q + n, fp_mul(s1, g1_inv));
        fp_store(q + 2 * n, fp_mul(fp_sub(p, m), g2_inv_half));
    }
}

// prover.py:108-116 — the gate identity on H, row by row: A QL + B QR + A B QM + C QO + PI + QC = 0.  flags[b] |= 1 otherwise
// (status bit 2).  Together with "Z closes to 1" (prover.py:132, status bit 1) this is exactly when the quotient's numerator is
// divisible by Z_H — the condition the reference re-checks on the quotient's top coefficients (prover.py:205-208), which a
// quotient interpolated from 3n points no longer has.  fixed_lag: [K][8][n], proof b's circuit is cid[b] (cid == null: circuit 0).
__global__ void gate_check_kernel(const Fr* abc, const Fr* pub, size_t l, const Fr* pi_or_null, const Fr* fixed_lag, const uint32_t* cid, size_t n, size_t B,
                                  uint32_t* bad) {
    PLONK_SHORT_KERNEL();
    const size_t total = B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n, i = gI - b * n;
        const Fr a = fp_load(abc + gI), bb = fp_load(abc + total + gI), c = fp_load(abc + 2 * total + gI);
        Fr pi = fp_zero<FrParams>();
        if (pi_or_null) pi = fp_load(pi_or_null + gI);
        else if (i < l) pi = fp_neg(fp_load(pub + b * l + i));
        const Fr* fl = cid ? fixed_lag + (size_t)cid[b] * FX_COUNT * n : fixed_lag;  // a lane finds its proof by division: per lane
        Fr gate = fp_add(fp_mul(a, fp_load(fl + FX_QL * n + i)), fp_mul(bb, fp_load(fl + FX_QR * n + i)));
        gate = fp_add(gate, fp_mul(fp_mul(a, bb), fp_load(fl + FX_QM * n + i)));
        gate = fp_add(gate, fp_mul(c, fp_load(fl + FX_QO * n + i)));
        gate = fp_add(gate, fp_add(pi, fp_load(fl + FX_QC * n + i)));
        if (!fp_is_zero(gate)) atomicOr(&bad[b], 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// Round 5 (prover.py:241-306) in coefficient form.  numerator of W_z:
//   R + v(A - a) + v^2(B - b) + v^3(C - c) + v^4(S1 - s1) + v^5(S2 - s2)
// is a linear combination of 15 coefficient vectors; the constants only change the remainder of the
// division by (X - zeta), which is zero by construction, so they are not needed for the quotient.
struct LinWeights { Fr w[15]; };
PLONK_DEV LinWeights linearisation_weights(const ProofState& s, unsigned log_n, Fr n_inv) {
    const Fr one = fp_one<FrParams>();
    const Fr a = s.evals[0], b = s.evals[1], c = s.evals[2], s1 = s.evals[3], s2 = s.evals[4], zw = s.evals[5];
    const Fr beta = s.beta, gamma = s.gamma, alpha = s.alpha, zeta = s.zeta, v = s.v;
    Fr zn = zeta;
    for (unsigned i = 0; i < log_n; i++) zn = fp_sqr(zn);
    const Fr zh = fp_sub(zn, one);                                       // Z_H(zeta)
    const Fr l0 = fp_mul(fp_mul(zh, n_inv), fp_inv(fp_sub(zeta, one)));  // L0(zeta) = Z_H / (n (zeta - 1))
    const Fr bz = fp_mul(beta, zeta);
    const Fr k1 = fp_mul(fp_mul(fp_add(fp_add(a, bz), gamma), fp_add(fp_add(b, fp_dbl(bz)), gamma)),
                         fp_add(fp_add(c, fp_mul3(bz)), gamma));
    const Fr k2 = fp_mul(fp_mul(fp_add(fp_add(a, fp_mul(beta, s1)), gamma), fp_add(fp_add(b, fp_mul(beta, s2)), gamma)), zw);
    const Fr a2 = fp_sqr(alpha);
    LinWeights L;
    L.w[0] = fp_mul(a, b);                                  // QM
    L.w[1] = a;                                             // QL
    L.w[2] = b;                                             // QR
    L.w[3] = c;                                             // QO
    L.w[4] = one;                                           // QC
    L.w[5] = fp_add(fp_mul(alpha, k1), fp_mul(a2, l0));     // Z
    L.w[6] = fp_neg(fp_mul(fp_mul(alpha, beta), k2));       // S3
    L.w[7] = fp_neg(zh);                                    // T1
    L.w[8] = fp_neg(fp_mul(zh, zn));                        // T2
    L.w[9] = fp_neg(fp_mul(zh, fp_sqr(zn)));                // T3
    Fr vp = v;
    L.w[10] = vp;                                           // A
    vp = fp_mul(vp, v); L.w[11] = vp;                       // B
    vp = fp_mul(vp, v); L.w[12] = vp;                       // C
    vp = fp_mul(vp, v); L.w[13] = vp;                       // S1
    vp = fp_mul(vp, v); L.w[14] = vp;                       // S2
    return L;
}

// one lane per proof: the 15 weights (one field inversion each) are computed once, not once per tile
__global__ void PLONK_BESIDE_ACC(64, 16) linearisation_weights_kernel(const ProofState* st, unsigned log_n, Fr n_inv, size_t B, LinWeights* out) {
    PLONK_SHORT_KERNEL();
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = linearisation_weights(st[b], log_n, n_inv);
}

// (lazy limbs, round 4: the 15 products of a coefficient pair up under 8 reductions — fpl_mul_add — with the weights unpacked
// once per block into LDS; the sum of the first seven results rides as "1 x sum" in the eighth, which leaves it reduced)
// fixed_coef: [K][8][n], the block's proof is of circuit cid[b] (cid == null: circuit 0)
__global__ void __launch_bounds__(256, 4) linearisation_kernel(const Fr* coef, const Fr* fixed_coef, const uint32_t* cid, const Fr* tcoef,
                                                              const LinWeights* weights, unsigned log_n, size_t B,
                                                              Fr* out) {
    PLONK_SHORT_KERNEL();
    typedef FpL<FrParams> L;
    __shared__ int32_t WL[16][12];  // the weights as limbs (9 of 12 words used); [15] = R mod m, the Montgomery form of 1
    const size_t n = (size_t)1 << log_n;
    const size_t b = blockIdx.y;
    if (threadIdx.x < 16) {
        const L w = threadIdx.x < 15 ? fpl_from_fp(fp_load(&weights[b].w[threadIdx.x])) : fpl_one<FrParams>();
#pragma unroll
        for (int q = 0; q < 9; q++) WL[threadIdx.x][q] = w.l[q];
    }
    __syncthreads();
    if (cid) fixed_coef += (size_t)cid[b] * FX_COUNT * n;
    const Fr* vec[15] = {fixed_coef + FX_QM * n, fixed_coef + FX_QL * n, fixed_coef + FX_QR * n, fixed_coef + FX_QO * n,
                         fixed_coef + FX_QC * n, coef + (4 * B + b) * n, fixed_coef + FX_S3 * n, tcoef + b * 4 * n,
                         tcoef + b * 4 * n + n,   tcoef + b * 4 * n + 2 * n, coef + (0 * B + b) * n,
                         coef + (1 * B + b) * n,  coef + (2 * B + b) * n,    fixed_coef + FX_S1 * n, fixed_coef + FX_S2 * n};
    const auto weight = [&](unsigned j) PLONK_LAMBDA_INLINE {
        L w;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            w.l[q] = WL[j][q];
            FPL_ANY_SIGN(w.l[q]);
        }
        return w;  // normalised, [0, m)
    };
    const auto value = [&](unsigned j, size_t i) PLONK_LAMBDA_INLINE { return fpl_from_fp(fp_load(vec[j] + i)); };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        L s = fpl_zero<FrParams>();
        wave_for<4>([&](auto Q) {  // four results, each normalised in (-m, 2m): limbs of the sum < 2^31
            constexpr unsigned j = 2 * decltype(Q)::value;
            s = fpl_add(s, fpl_mul_add(weight(j), value(j, i), weight(j + 1), value(j + 1, i)));
            PLONK_SCHED_FENCE();
        });
        s = fpl_norm(s);  // (-4 m, 8 m)
        L t = fpl_zero<FrParams>();
        wave_for<3>([&](auto Q) {
            constexpr unsigned j = 8 + 2 * decltype(Q)::value;
            t = fpl_add(t, fpl_mul_add(weight(j), value(j, i), weight(j + 1), value(j + 1, i)));
            PLONK_SCHED_FENCE();
        });
        const L u = fpl_norm(fpl_add(s, fpl_norm(t)));  // (-7 m, 14 m), normalised
        fp_store(out + b * n + i, fpl_pack_canonical(fpl_mul_add(weight(14), value(14, i), weight(15), u)));  // |.| < 1 + 14
    }
}

// ------------------------------------------------------------------------------------------------
// pack results: [B] proof records (prover.h), plain or compressed
__global__ void pack_proofs_kernel(const Fq* commit_xy, const ProofState* st, size_t B, uint8_t* out, int compressed) {
    PLONK_SHORT_KERNEL();
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (compressed) {
        uint8_t* o = out + b * PROOF_BYTES_COMPRESSED;
        for (int slot = 0; slot < PROOF_POINTS; slot++) {
            const Fq x = fp_load(commit_xy + 2 * ((size_t)slot * B + b)), y = fp_load(commit_xy + 2 * ((size_t)slot * B + b) + 1);
            g1c_compress<FqParams>(x.v, y.v, o + 32 * slot);
        }
        for (int e = 0; e < PROOF_EVALS; e++) {
            const Fr v = fp_from_mont(st[b].evals[e]);
            g1c_be32(v.v, o + PROOF_COMPRESSED_EVALS + 32 * e);
        }
        return;
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(out + b * PROOF_BYTES);
    for (int slot = 0; slot < PROOF_POINTS; slot++)
        for (int h = 0; h < 2; h++) {
            Fq v = fp_load(commit_xy + 2 * ((size_t)slot * B + b) + h);
            for (int i = 0; i < 8; i++) o[proof_point_word(slot, h) + i] = v.v[i];
        }
    for (int e = 0; e < PROOF_EVALS; e++) {
        Fr v = fp_from_mont(st[b].evals[e]);
        for (int i = 0; i < 8; i++) o[proof_eval_word(e) + i] = v.v[i];
    }
}

// the status byte of every proof (PROVER_ST_*); closes = plonk_prover::closes; bad_stride = values per proof of the upload that
// filled *bad_input; solve_bad = plonk_prover::solve_bad, or null for a batch that did not come through the solver
__global__ void pack_status_kernel(const ProofState* st, const uint32_t* closes, const uint8_t* flags, const unsigned long long* bad_input,
                                   size_t bad_stride, const uint32_t* solve_bad, size_t B, uint8_t* out) {
    PLONK_SHORT_KERNEL();
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint8_t f = 0;
    for (int slot = 0; slot < PROOF_POINTS; slot++) f |= flags[(size_t)slot * B + b] ? PROVER_ST_IDENTITY : 0;
    if (st[b].error) f |= PROVER_ST_IDENTITY;
    if (!closes[b]) f |= PROVER_ST_Z_OPEN;
    if (closes[B + b]) f |= PROVER_ST_GATE;
    if (bad_input && *bad_input != ~0ull && bad_stride && *bad_input / bad_stride == b) f |= PROVER_ST_BAD_INPUT;
    if (solve_bad && solve_bad[b]) f |= PROVER_ST_ASSERT;
    out[b] = f;
}

// ================================================================================================
// host side

// S of a prover's batch: PLONK_PROVER_SEGMENTS_LOG2 where it was set, the automatic rule otherwise
static unsigned prover_segments(const plonk_prover* p, size_t B) {
    return p->seg_forced ? 1u << (p->seg_forced - 1) : prover_plan_segments(device_cus(p->circuit.ctx->device), p->circuit.log_n, B);
}

// The per-batch buffers, once: what ensure_batch allocates, free_batch frees and the out-of-memory message adds up.  Per proof a buffer
// holds n_vectors Fr vectors of n elements and `bytes` more; `extra` bytes once.  in_set: the buffer belongs to the resident batch's set
// (prover_intake.h): an advance exchanges it with the staged set's, which staged_grow sizes on its own.
struct BatchBuffer { void** slot; size_t n_vectors, bytes, extra; bool in_set; };
// n-vectors of 32 bytes per proof, the figure of the out-of-memory message: 32, or 37 on the four cosets of a blinded prover
static size_t batch_n_vectors(const plonk_prover* p) { return 17 + 5 * p->circuit.qcosets; }
static std::array<BatchBuffer, 14> batch_buffers(plonk_prover* p) {
    plonk_prover::Rounds& r = p->rounds;
    plonk_prover::Results& o = p->results;
    const size_t e = sizeof(Fr);
    return {{{(void**)&r.wit_lag, STAGED_N_VECTORS, 0, 0, true}, {(void**)&r.z_lag, 1}, {(void**)&r.coef, 5}, {(void**)&r.big, 5 * p->circuit.qcosets}, {(void**)&r.quot, 4},
             {(void**)&r.num, 1}, {(void**)&r.wz, 2}, {(void**)&r.closes, 0, 2 * sizeof(uint32_t)}, {(void**)&r.lin_w, 0, sizeof(LinWeights)}, {(void**)&r.blind, 0, sizeof(BlindState)},
             {(void**)&o.commit_xy, 0, PROOF_POINTS * 2 * sizeof(Fq)}, {(void**)&o.commit_flags, 0, PROOF_POINTS},
             {(void**)&o.state, 0, sizeof(ProofState)}, {(void**)&p->intake.pub, 0, p->circuit.n_public * e, e, true}}};
}

// all of them, or (rounds_only) all but the resident set's
static void free_batch(plonk_prover* p, bool rounds_only = false) {
    for (const BatchBuffer& b : batch_buffers(p))
        if (!(rounds_only && b.in_set)) dev_free_all({b.slot});
    dev_free_all({(void**)&p->rounds.seg});  // sized by the batch too: it makes room for a larger one
    p->rounds.seg_cap = p->intake.resident_b = p->rounds.cap_b = 0;
    if (rounds_only) return;
    dev_free_all({(void**)&p->intake.vars.buf});  // the same
    p->intake.vars.cap = p->intake.cap_b = 0;
}

// the carries and partial sums of the segmented scans (prover_scans.h: scan_scratch_elems)
static int ensure_segments(plonk_prover* p, size_t B) {
    const size_t need = scan_scratch_elems(B, prover_segments(p, B));
    return dev_grow(p->circuit.ctx->stream, &p->rounds.seg_cap, need, {{(void**)&p->rounds.seg, need * sizeof(Fr)}});
}

// The per-batch buffers (rounds_only: as free_batch) for B proofs: nothing while they hold B, otherwise all of them anew.
static int ensure_buffers(plonk_prover* p, size_t B, bool rounds_only) {
    if (B <= p->rounds.cap_b && (rounds_only || B <= p->intake.cap_b)) return ensure_segments(p, B);
    PLONK_CHECK_HIP(hipStreamSynchronize(p->circuit.ctx->stream));
    free_batch(p, rounds_only);
    int rc = PLONK_OK;
    size_t vectors = 0;
    for (const BatchBuffer& b : batch_buffers(p)) {
        if (rc == PLONK_OK && !(rounds_only && b.in_set)) rc = dev_alloc(b.slot, B * (b.n_vectors * p->circuit.n * sizeof(Fr) + b.bytes) + b.extra);
        vectors += b.n_vectors;
    }
    assert(vectors == batch_n_vectors(p));
    if (rc != PLONK_OK) {
        free_batch(p, rounds_only);
        if (rc == PLONK_ERR_NOMEM)
            plonk_set_error("a batch of %zu proofs of group_order %zu needs %zu bytes of device memory", B, p->circuit.n,
                            batch_n_vectors(p) * B * p->circuit.n * sizeof(Fr));
        return rc;
    }
    p->rounds.cap_b = B;
    if (!rounds_only) p->intake.cap_b = B;
    return ensure_segments(p, B);
}
static int ensure_batch(plonk_prover* p, size_t B) { return ensure_buffers(p, B, false); }
static int ensure_rounds(plonk_prover* p, size_t B) { return ensure_buffers(p, B, true); }

// One transcript round of every proof: round 0 opens the transcripts, round r absorbs what round r of the prover produced.
static void transcript_round(plonk_prover* p, size_t B, int round) {
    PLONK_LAUNCH(transcript_kernel, dim3((unsigned)((B + 1) / 2)), dim3(2 * TC_LANES), 0, p->circuit.ctx->stream, round, p->results.state, B,
                 (const Fq*)p->results.commit_xy, (const uint8_t*)p->results.commit_flags, p->circuit.chal, p->rounds.closes + B);
}

// `count` x B commitments into the proof records' points from `first_point` on: of the Lagrange values under the Lagrange-basis
// SRS where PLONK_PROVER_LAGRANGE_COMMITS is set (the same points), of the coefficient forms otherwise
static int commit(plonk_prover* p, size_t B, const Fr* lag, const Fr* coef, size_t count, size_t first_point) {
    const plonk_prover::Circuit& c = p->circuit;
    return msm_run_device(c.ctx, p->lag_srs ? p->lag_srs : c.srs, p->lag_srs ? lag : coef, c.n, count * B, c.n, p->results.commit_xy + 2 * first_point * B,
                          p->results.commit_flags + first_point * B);
}

// sum_k q_k H_k into `count` x B commitments of the proof records from `first_point` on, behind the MSMs that left MSM(p0) there
static void blind_commit(plonk_prover* p, size_t B, unsigned first_point, unsigned count) {
    PLONK_LAUNCH(blind_commit_kernel, dim3((unsigned)B, count), dim3(BLIND_LANES), 0, p->circuit.ctx->stream, (const BlindState*)p->rounds.blind,
                 (const G1Affine*)p->blinding_src.htab, first_point, B, p->results.commit_xy, p->results.commit_flags);
}

// The blinders of this run into the BlindStates: the explicit ones where plonk_prover_set_blinders left some for this batch size
// (they serve one run), the seed's draws otherwise.  Every blinded run counts, so that one seed never blinds two batches alike.
static int blinders_for_run(plonk_prover* p, size_t B) {
    plonk_prover::Blinding& bl = p->blinding_src;
    hipStream_t s = p->circuit.ctx->stream;
    PLONK_REQUIRE(!bl.explicit_batch || bl.explicit_batch == B, PLONK_ERR_STATE, "run: batch %zu, but the blinders were set for a batch of %zu", B,
                  bl.explicit_batch);
    PLONK_REQUIRE(bl.explicit_batch || bl.seeded, PLONK_ERR_STATE,
                  "run: batch %zu is to be blinded, but neither plonk_prover_set_blinders nor plonk_prover_seed_blinders has been called", B);
    if (bl.explicit_batch) {
        PLONK_LAUNCH(blind_load_kernel, grid1(B * BLIND_COUNT), dim3(256), 0, s, (const Fr*)bl.explicit_b, B, p->rounds.blind);
        bl.explicit_batch = 0;
    } else {
        BlindSeed in;
        memcpy(in.seed, bl.seed, 32);
        in.run = bl.runs;
        PLONK_LAUNCH(blind_derive_kernel, dim3((unsigned)((B + 1) / 2)), dim3(2 * TC_LANES), 0, s, in, B, p->circuit.chal, p->rounds.blind);
    }
    bl.runs++;
    return PLONK_OK;
}

static int prover_init(plonk_prover* p, plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, unsigned K, const uint8_t* selectors_le32, const size_t* n_public);

// plonk_prover_create (K = 1) and plonk_prover_create_multi: a table of K circuits of group order 2^log_n, selectors [K][8][n]
static int prover_create(plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, unsigned K, const uint8_t* selectors_le32, const size_t* n_public, plonk_prover** out) {
    PLONK_ENTER(ctx);
    PLONK_REQUIRE(log_n >= 1 && log_n + 2 <= PLONK_FR_TWO_ADICITY, PLONK_ERR_ARG, "group_order 2^%u out of range", log_n);
    const size_t n = (size_t)1 << log_n;
    PLONK_REQUIRE(log_n <= PROVER_MAX_LOG_N, PLONK_ERR_ARG, "the batched prover supports group_order <= %u (got %zu)", 1u << PROVER_MAX_LOG_N, n);
    PLONK_REQUIRE(srs->n_points >= n, PLONK_ERR_ARG, "SRS has %zu powers, group_order is %zu", srs->n_points, n);
    for (unsigned c = 0; c < K; c++) PLONK_REQUIRE(n_public[c] <= n, PLONK_ERR_ARG, "more public inputs than rows");
    plonk_prover* p = new plonk_prover();
    memset((void*)p, 0, sizeof *p);
    const int rc = prover_init(p, ctx, srs, log_n, K, selectors_le32, n_public);
    if (rc != PLONK_OK) {  // a single cleanup path: everything allocated so far goes with the half-built object
        plonk_prover_destroy(p);
        return rc;
    }
    *out = p;
    return PLONK_OK;
}

extern "C" {

int plonk_prover_create(plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, const uint8_t* selectors_le32,
                        size_t n_public, plonk_prover** out) {
    PLONK_REQUIRE(ctx && srs && selectors_le32 && out, PLONK_ERR_ARG, "bad argument");
    return prover_create(ctx, srs, log_n, 1, selectors_le32, &n_public, out);
}

int plonk_prover_create_multi(plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, size_t n_circuits, const uint8_t* selectors_le32, const size_t* n_public,
                              plonk_prover** out) {
    PLONK_REQUIRE(ctx && srs && selectors_le32 && n_public && out, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(n_circuits >= 1 && n_circuits <= PLONK_PROVER_MAX_CIRCUITS, PLONK_ERR_ARG, "%zu circuits: a table holds 1 to %d", n_circuits,
                  PLONK_PROVER_MAX_CIRCUITS);
    return prover_create(ctx, srs, log_n, (unsigned)n_circuits, selectors_le32, n_public, out);
}

}  // extern "C"

// `batch` coefficient vectors onto the cosets g mu^r H: P(g mu^r w^j) is the size-n transform of c_i (g mu^r)^i — one input, qcosets
// scalings, outputs [r][n] side by side
static NttCall coset_call(const plonk_prover::Circuit& c, const Fr* in, Fr* out, size_t batch) {
    NttCall t = ntt_forward(in, out, c.log_n, batch);
    t.out_bstride = c.qcosets * c.n;
    t.in_scale = c.g_pow;
    t.fan = NttFan{c.qcosets, 0u, (unsigned)c.n, (unsigned)c.n};
    return t;
}

// Everything of the circuit that lives on the cosets g mu^r H, r < qcosets, anew: plonk_prover_create for three, and
// plonk_prover_set_options when PLONK_PROVER_BLINDING changes their number.
static void free_coset_tables(plonk_prover::Circuit& c) {
    dev_free_all({(void**)&c.fixed_big, (void**)&c.l0_big, (void**)&c.x_big, (void**)&c.g_pow, (void**)&c.ginv_pow, (void**)&c.li_big});
}
static int coset_tables(plonk_prover* p) {
    plonk_prover::Circuit& c = p->circuit;
    plonk_ctx* ctx = c.ctx;
    const size_t n = c.n, e = sizeof(Fr), n3 = c.qcosets * n, K = c.n_circuits;
    const unsigned log_n = c.log_n;
    free_coset_tables(c);
    PLONK_TRY(dev_alloc((void**)&c.fixed_big, K * 8 * n3 * e));
    PLONK_TRY(dev_alloc((void**)&c.l0_big, n3 * e));
    PLONK_TRY(dev_alloc((void**)&c.x_big, n3 * e));
    PLONK_TRY(dev_alloc((void**)&c.g_pow, n3 * e));
    PLONK_TRY(dev_alloc((void**)&c.ginv_pow, n3 * e));
    const Fr one = fp_one<FrParams>();
    const Fr mu = host_root_of_unity(log_n + 2, false);
    Fr base = c.g;  // g mu^r
    for (unsigned r = 0; r < c.qcosets; r++) {
        PLONK_TRY(k_fr_powers(ctx, base, one, c.g_pow + r * n, n));
        PLONK_TRY(k_fr_powers(ctx, fp_inv(base), fp_mul(c.half, c.n_inv), c.ginv_pow + r * n, n));
        PLONK_TRY(k_fr_powers(ctx, c.w, base, c.x_big + r * n, n));
        base = fp_mul(base, mu);
    }
    PLONK_TRY(ntt_run(ctx, coset_call(c, c.fixed_coef, c.fixed_big, 8 * K)));  // the circuit polynomials' values on the cosets: [K][8][qcosets][n]
    // L0: Lagrange vector e_0 has coefficient form (1/n, 1/n, ...)          prover.py:184-186
    void* tmpv;
    PLONK_TRY(ctx_scratch(ctx, 2, n * e, &tmpv));  // context-owned scratch: nothing to leak on an error path
    Fr* tmp = (Fr*)tmpv;
    PLONK_TRY(k_fr_powers(ctx, one, c.n_inv, tmp, n));
    PLONK_TRY(ntt_run(ctx, coset_call(c, tmp, c.l0_big, 1)));
    if (c.sparse_pi && c.n_public) {
        Zh4 zh4;
        for (int k = 0; k < 4; k++) zh4.v[k] = c.zh[k];
        PLONK_TRY(dev_alloc((void**)&c.li_big, c.n_public * n3 * e));
        PLONK_LAUNCH(li_coset_kernel, grid1(c.n_public * n3), dim3(256), 0, ctx->stream, (const Fr*)c.x_big, c.roots, n3, n, c.n_public,
                     zh4, c.n_inv, c.li_big);
        PLONK_CHECK_HIP(hipGetLastError());
    }
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return PLONK_OK;
}

// PLONK_PROVER_BLINDING on or off (prover_blind.h).  The quotient of a blinded proof has 3n + 6 coefficients, so it is interpolated
// from four cosets, which takes n >= 8 (3n + 5 < 4n); its commitments add multiples of [tau^(n+k)] - [tau^k], k < 6, which takes
// n + 6 monomial powers.  The coset forms are rebuilt for the new number of cosets and the per-batch buffers are dropped (r.big
// changes size): the resident batch goes with them, a staged one stays.
static int set_blinding(plonk_prover* p, bool on) {
    plonk_prover::Circuit& c = p->circuit;
    plonk_prover::Blinding& bl = p->blinding_src;
    if (on) {
        PLONK_REQUIRE(c.n >= 8, PLONK_ERR_ARG, "blinding: the quotient has 3n + 6 coefficients and four cosets hold 4n: group_order %zu is below 8", c.n);
        const plonk_srs* mono = c.srs->parent ? c.srs->parent : c.srs;  // a Lagrange view (plonk_srs_lagrange) takes the powers from its monomial parent
        PLONK_REQUIRE(mono->bases, PLONK_ERR_ARG, "blinding: the prover's SRS holds no monomial powers; the blinded commitments need tau^%zu .. tau^%zu",
                      c.n, c.n + BLIND_TAIL - 1);
        PLONK_REQUIRE(mono->n_points >= c.n + BLIND_TAIL, PLONK_ERR_ARG, "blinding: group_order %zu needs %zu powers of tau, the SRS has %zu", c.n,
                      c.n + BLIND_TAIL, mono->n_points);
        if (!bl.htab) {
            PLONK_TRY(dev_alloc((void**)&bl.htab, BLIND_TAIL * BLIND_WINDOWS * sizeof(G1Affine)));
            PLONK_LAUNCH(blind_h_kernel, dim3(2), dim3(64), 0, c.ctx->stream, (const G1Affine*)mono->bases, c.n, bl.htab);
            PLONK_CHECK_HIP(hipGetLastError());
        }
    }
    PLONK_CHECK_HIP(hipStreamSynchronize(c.ctx->stream));
    free_batch(p);
    c.qcosets = on ? QCOSETS_BLINDED : QCOSETS;
    PLONK_TRY(coset_tables(p));
    p->blinding = on;
    return PLONK_OK;
}

static int prover_init(plonk_prover* p, plonk_ctx* ctx, plonk_srs* srs, unsigned log_n, unsigned K, const uint8_t* selectors_le32,
                       const size_t* n_public_of) {
    const size_t n = (size_t)1 << log_n;
    plonk_prover::Circuit& c = p->circuit;
    c.ctx = ctx;
    c.srs = srs;
    c.log_n = log_n;
    c.n = n;
    c.n_circuits = K;
    c.n_public_of = (size_t*)malloc(K * sizeof(size_t));
    PLONK_REQUIRE(c.n_public_of, PLONK_ERR_NOMEM, "out of host memory");
    size_t n_public = 0;  // l_max: the public rows, sparse PI and li_big are sized by the widest circuit, zeros beyond a circuit's own
    for (unsigned k = 0; k < K; k++) {
        c.n_public_of[k] = n_public_of[k];
        if (n_public_of[k] > n_public) n_public = n_public_of[k];
    }
    c.n_public = n_public;
    c.chal = challenge_consts();
    c.g = host_fr_u64(5);  // multiplicative generator (curve.py:5): g^(4n) != 1, so Z_H != 0 on the coset
    c.w = host_root_of_unity(log_n, false);
    c.n_inv = host_fp_inv_pow2<FrParams>(log_n);
    c.half = fp_inv(host_fr_u64(2));
    const size_t e = sizeof(Fr);
    PLONK_TRY(dev_alloc((void**)&c.fixed_lag, K * 8 * n * e));
    PLONK_TRY(dev_alloc((void**)&c.fixed_coef, K * 8 * n * e));
    PLONK_TRY(plonk_fr_upload(ctx, c.fixed_lag, selectors_le32, K * 8 * n));
    PLONK_TRY(intake_init(p, selectors_le32));
    PLONK_TRY(ntt_get_roots(ctx, log_n, false, &c.roots));
    // coefficient forms of the 8 circuit polynomials
    PLONK_TRY(ntt_run(ctx, ntt_inverse(c.fixed_lag, c.fixed_coef, log_n, 8 * K)));
    // Z_H on coset r is the constant (g mu^r)^n - 1 = g^n i^r - 1, i = mu^n            prover.py:178
    const Fr one = fp_one<FrParams>();
    Fr gn = c.g;
    for (unsigned i = 0; i < log_n; i++) gn = fp_sqr(gn);
    Fr i4 = host_root_of_unity(2, false), cur = gn;
    for (int k = 0; k < 4; k++) {
        c.zh[k] = fp_sub(cur, one);
        c.zh_inv[k] = fp_inv(c.zh[k]);
        cur = fp_mul(cur, i4);
    }
    c.comb_i = i4;
    c.comb_g1 = fp_inv(gn);
    c.comb_g2 = fp_mul(fp_sqr(c.comb_g1), c.half);
    c.sparse_pi = n_public <= PI_SPARSE_MAX;
    if (c.sparse_pi && n_public) PLONK_TRY(ntt_get_roots(ctx, log_n, true, &c.roots_inv));
    c.qcosets = QCOSETS;
    PLONK_TRY(coset_tables(p));
    return PLONK_OK;  // (the MSM tables are built by the first commitment: lookup table or bucket-method window table)
}

extern "C" {

int plonk_prover_set_options(plonk_prover* p, unsigned flags) {
    PLONK_REQUIRE(p && !(flags & ~(PLONK_PROVER_LAGRANGE_COMMITS | PLONK_PROVER_SEGMENTS_MASK | PLONK_PROVER_SOLVE_FORM_MASK | PLONK_PROVER_BLINDING)),
                  PLONK_ERR_ARG, "unknown prover option bits %#x", flags);
    PLONK_ENTER(p->circuit.ctx);
    const unsigned seg = (flags & PLONK_PROVER_SEGMENTS_MASK) >> 8;  // k + 1, 0 = automatic
    PLONK_REQUIRE(seg <= 9 && (!seg || (p->circuit.n >> (seg - 1)) >= 16), PLONK_ERR_ARG,
                  "2^%u segments: at most 256, of at least 16 rows each (group_order %zu)", seg ? seg - 1 : 0, p->circuit.n);
    const unsigned form = (flags & PLONK_PROVER_SOLVE_FORM_MASK) >> 16;  // 0 = automatic
    PLONK_REQUIRE(form <= PLONK_PROVER_SOLVE_LEVELS, PLONK_ERR_ARG, "solve form %u: 0 (automatic), 1 (one lane per proof) or 2 (levels)", form);
    const bool blinding = (flags & PLONK_PROVER_BLINDING) != 0;
    if (blinding != p->blinding) PLONK_TRY(set_blinding(p, blinding));
    p->seg_forced = seg;
    p->solve_forced = form;  // from the next input upload on
    p->lag_srs = nullptr;
    if (flags & PLONK_PROVER_LAGRANGE_COMMITS) PLONK_TRY(msm_lagrange_srs(p->circuit.ctx, p->circuit.srs, p->circuit.log_n, &p->lag_srs));
    return PLONK_OK;
}

int plonk_prover_destroy(plonk_prover* p) {
    if (!p) return PLONK_OK;
    plonk_prover::Circuit& c = p->circuit;
    if (c.ctx) {
        plonk_use_device(c.ctx->device);
        hipStreamSynchronize(c.ctx->stream);
        if (c.ctx->copy_stream) hipStreamSynchronize(c.ctx->copy_stream);  // a batch that is still staged: its solve reads the circuit and the plan
    }
    free_batch(p);
    free_coset_tables(c);
    dev_free_all({(void**)&c.fixed_lag, (void**)&c.fixed_coef, (void**)&p->blinding_src.htab, (void**)&p->blinding_src.explicit_b});
    intake_destroy(p);
    free(c.n_public_of);
    delete p;
    return PLONK_OK;
}

// Enqueue all five rounds for the B resident witnesses.  Asynchronous.
int plonk_prover_run(plonk_prover* p, size_t B) {
    PLONK_REQUIRE(p && B, PLONK_ERR_ARG, "bad argument");
    // every buffer is laid out [k][B][n] with the B of the upload: another B would read the wrong strides
    PLONK_REQUIRE(B == p->intake.resident_b, PLONK_ERR_STATE, "run: batch %zu, but %zu witnesses are resident", B, p->intake.resident_b);
    const plonk_prover::Circuit& c = p->circuit;
    const plonk_prover::Rounds& r = p->rounds;
    PLONK_ENTER(c.ctx);
    plonk_ctx* ctx = c.ctx;
    const size_t n = c.n, n4 = 4 * n;
    const unsigned log_n = c.log_n;
    hipStream_t s = ctx->stream;
    const Fr* pub = p->intake.pub;
    ProofState* state = p->results.state;
    PLONK_REQUIRE(B <= 65535, PLONK_ERR_ARG, "batch %zu exceeds 65535 (the proofs are a grid's second dimension)", B);
    PLONK_TRY(ensure_segments(p, B));  // (the options may have changed since the upload)
    const unsigned S = prover_segments(p, B);  // of the three scans (prover_scans.h); 1: one workgroup per proof
    const bool blind = p->blinding;            // every `if (blind)` below is a correction of prover_blind.h behind the step it follows
    BlindState* bs = r.blind;
    if (blind) PLONK_TRY(blinders_for_run(p, B));
    const uint32_t* cid = c.n_circuits > 1 ? p->labels.dev : nullptr;  // the proofs' circuits (a table of one: circuit 0, no array)

    transcript_round(p, B, 0);
    // ---- round 1: coefficient forms of A, B, C, PI; commit A, B, C            prover.py:86-119
    PLONK_LAUNCH(gate_check_kernel, grid1(B * n), dim3(256), 0, s, (const Fr*)r.wit_lag, pub, c.n_public,
                 c.sparse_pi ? (const Fr*)nullptr : (const Fr*)(r.wit_lag + 3 * B * n), (const Fr*)c.fixed_lag, cid, n, B, r.closes + B);  // prover.py:108-116
    if (c.sparse_pi) {
        PLONK_TRY(ntt_run(ctx, ntt_inverse(r.wit_lag, r.coef, log_n, 3 * B)));
        if (c.n_public) PLONK_LAUNCH(pi_coeffs_kernel, grid1(B * n), dim3(256), 0, s, pub, c.n_public, c.roots_inv, n, B, c.n_inv, r.coef + 3 * B * n);
        else PLONK_CHECK_HIP(hipMemsetAsync(r.coef + 3 * B * n, 0, B * n * sizeof(Fr), s));
    } else {
        PLONK_TRY(ntt_run(ctx, ntt_inverse(r.wit_lag, r.coef, log_n, 4 * B)));
    }
    PLONK_TRY(commit(p, B, r.wit_lag, r.coef, 3, 0));
    if (blind) blind_commit(p, B, 0, 3);
    transcript_round(p, B, 1);
    // ---- round 2: grand product Z, commit                                      prover.py:121-152
    GrandProductIn gp = {};
    for (int k = 0; k < 3; k++) {
        gp.abc[k] = r.wit_lag + (size_t)k * B * n;
        gp.sig[k] = c.fixed_lag + (FX_S1 + k) * n;
    }
    gp.cid = cid;
    gp.sig_stride = FX_COUNT * n;
    // (the three scan families are instrumented for plonk_profile_read: tools/prover_scale.py)
    PLONK_TRY(prof_begin(ctx, "prover_grand_product", 11.0 * 32.0 * (double)n * (double)B));
    PLONK_TRY(scan_grand_product(s, S, gp, c.roots, state, RoundChallenges{}, n, B, r.z_lag, r.closes, r.num, r.wz, r.seg));  // num / wz: scratch until round 5
    PLONK_TRY(prof_end(ctx));
    PLONK_TRY(ntt_run(ctx, ntt_inverse(r.z_lag, r.coef + 4 * B * n, log_n, B)));
    PLONK_TRY(commit(p, B, r.z_lag, r.coef + 4 * B * n, 1, 3));
    if (blind) blind_commit(p, B, 3, 1);
    transcript_round(p, B, 2);
    // ---- round 3: coset extensions, fused quotient, back to coefficients, commit T1..T3   prover.py:154-226
    // deg t < 3n: three cosets g mu^r H of the n-th roots of unity determine the quotient, so A, B, C, Z are evaluated on 3n
    // points — per coset a size-n transform of c_i (g mu^r)^i, on the 2^log_n kernel — instead of the reference's 4n, the
    // fused pass runs over 3n points, and three size-n inverse transforms + quotient_combine_kernel give T1, T2, T3.
    // Blinded, deg t = 3n + 5: the same on all four cosets (n3 = 4n), the tails' values added to the coset forms in between, and
    // blind_combine_kernel in quotient_combine_kernel's place.
    const size_t n3 = c.qcosets * n;
    if (c.sparse_pi) {  // A, B, C and Z through the transform, PI from the Lagrange basis on the coset
        PLONK_TRY(ntt_run(ctx, coset_call(c, r.coef, r.big, 3 * B)));
        PLONK_TRY(ntt_run(ctx, coset_call(c, r.coef + 4 * B * n, r.big + 4 * B * n3, B)));
        if (c.n_public) PLONK_LAUNCH(pi_coset_kernel, grid1(B * n3), dim3(256), 0, s, pub, c.n_public, (const Fr*)c.li_big, n3, B, r.big + 3 * B * n3);
        else PLONK_CHECK_HIP(hipMemsetAsync(r.big + 3 * B * n3, 0, B * n3 * sizeof(Fr), s));
    } else {
        PLONK_TRY(ntt_run(ctx, coset_call(c, r.coef, r.big, 5 * B)));
    }
    if (blind) {
        BlindZh bz;
        for (int k = 0; k < 4; k++) bz.v[k] = c.zh[k];
        PLONK_LAUNCH(blind_coset_kernel, grid1(B * n3), dim3(256), 0, s, (const BlindState*)bs, (const Fr*)c.x_big, bz, log_n, B, r.big);
    }
    ZhInv zh;
    for (int k = 0; k < 4; k++) zh.v[k] = c.zh_inv[k < (int)c.qcosets ? k : 0];
    QuotientIn qi = {};
    for (int k = 0; k < 5; k++) qi.wit[k] = r.big + (size_t)k * B * n3;
    for (int k = 0; k < FX_COUNT; k++) qi.fixed[k] = c.fixed_big + (size_t)k * n3;
    qi.l0 = c.l0_big;
    qi.xs = c.x_big;
    qi.cid = cid;
    qi.fixed_stride = (unsigned)(FX_COUNT * n3);
    PLONK_LAUNCH(quotient_kernel, dim3((unsigned)((n3 + 255) / 256), (unsigned)B), dim3(256), 0, s, qi, zh, (const ProofState*)state, RoundChallenges{},
                 (unsigned)n3, r.quot, log_n, (unsigned)n4);
    NttCall back{r.quot, r.quot, log_n, true, B};  // (1/n rides in ginv_pow)
    back.in_bstride = back.out_bstride = n4;
    back.out_scale = c.ginv_pow;
    back.fan = NttFan{c.qcosets, (unsigned)n, (unsigned)n, (unsigned)n};  // the three coset slices of every quotient row, in place
    PLONK_TRY(ntt_run(ctx, back));
    if (blind) {
        const BlindCombine bc = {c.comb_i, c.half, fp_mul(c.comb_g1, c.half), c.comb_g2, fp_mul(c.comb_g2, c.comb_g1)};
        PLONK_LAUNCH(blind_combine_kernel, grid1(B * n), dim3(256), 0, s, r.quot, n, n4, B, bc, bs);
    } else {
        PLONK_LAUNCH(quotient_combine_kernel, grid1(B * n), dim3(256), 0, s, r.quot, n, n4, B, c.comb_i, c.comb_g1, c.comb_g2, c.half);
    }
    // T1..T3 = the three n-coefficient slices of each quotient row, one batched call (MSM k*B + b = slice k of proof b)
    PLONK_TRY(msm_run_device(ctx, c.srs, r.quot, n, 3 * B, n4, p->results.commit_xy + 2 * 4 * B, p->results.commit_flags + 4 * B, B, n));
    if (blind) blind_commit(p, B, 4, 3);
    transcript_round(p, B, 3);
    // ---- round 4: evaluations                                                  prover.py:228-239
    PLONK_TRY(prof_begin(ctx, "prover_evaluations", 7.0 * 32.0 * (double)n * (double)B));
    PLONK_TRY(scan_evaluations(s, S, r.coef, c.fixed_coef, cid, c.w, state, n, B, r.seg));
    PLONK_TRY(prof_end(ctx));
    if (blind) PLONK_LAUNCH(blind_evals_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, (const BlindState*)bs, state, c.w, log_n, B);
    transcript_round(p, B, 4);
    // ---- round 5: opening polynomials in coefficient form, commit              prover.py:241-306
    PLONK_LAUNCH(linearisation_weights_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, (const ProofState*)state, log_n, c.n_inv, B, r.lin_w);
    PLONK_LAUNCH(linearisation_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, s, (const Fr*)r.coef, (const Fr*)c.fixed_coef,
                 cid, (const Fr*)r.quot, (const LinWeights*)r.lin_w, log_n, B, r.num);
    if (blind) PLONK_LAUNCH(blind_openings_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, bs, (const ProofState*)state, (const Fr*)r.lin_w, c.w, B);
    PLONK_TRY(prof_begin(ctx, "prover_divisions", 2.0 * 3.0 * 32.0 * (double)n * (double)B));
    const DivideIn dv = {{r.num, r.coef + 4 * B * n}, {r.wz, r.wz + B * n}};  // W_z's numerator by X - zeta, Z by X - zeta w
    PLONK_TRY(scan_divisions(s, S, dv, c.w, state, n, B, r.seg));
    PLONK_TRY(prof_end(ctx));
    if (blind)
        PLONK_LAUNCH(blind_division_kernel, dim3((unsigned)((n + 256 * BLIND_ROWS_PER_LANE - 1) / (256 * BLIND_ROWS_PER_LANE)), (unsigned)B, 2), dim3(256), 0, s,
                     (const BlindState*)bs, (const ProofState*)state, c.w, n, B, r.wz);
    PLONK_TRY(msm_run_device(ctx, c.srs, r.wz, n, 2 * B, n, p->results.commit_xy + 2 * 7 * B, p->results.commit_flags + 7 * B));
    if (blind) blind_commit(p, B, 7, 2);
    PLONK_CHECK_HIP(hipGetLastError());
    return PLONK_OK;
}

// The blinders of the next blinded run of `batch` proofs, [batch][11] canonical LE: b[0..10] of prover_blind.h's table.
int plonk_prover_set_blinders(plonk_prover* p, const uint8_t* blinders_le32, size_t batch) {
    PLONK_REQUIRE(p && blinders_le32 && batch, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(p->circuit.ctx);
    plonk_prover::Blinding& bl = p->blinding_src;
    const size_t count = batch * BLIND_COUNT;
    for (size_t i = 0; i < count; i++)
        PLONK_REQUIRE(le32_below_modulus(blinders_le32 + 32 * i, false), PLONK_ERR_ARG, "blinder %zu of proof %zu is not below r", i % BLIND_COUNT,
                      i / BLIND_COUNT);
    hipStream_t s = p->circuit.ctx->stream;
    PLONK_TRY(dev_grow(s, &bl.explicit_cap, batch, {{(void**)&bl.explicit_b, count * sizeof(Fr)}}));
    std::vector<Fr> mont(count);
    for (size_t i = 0; i < count; i++) mont[i] = fr_from_le32(blinders_le32 + 32 * i);
    PLONK_CHECK_HIP(hipMemcpyAsync(bl.explicit_b, mont.data(), count * sizeof(Fr), hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipStreamSynchronize(s));  // `mont` goes out of scope
    bl.explicit_batch = batch;
    return PLONK_OK;
}

// The device draws every later run's blinders from `seed`, the number of blinded runs since this call and the proof's index.
int plonk_prover_seed_blinders(plonk_prover* p, const uint8_t seed[32]) {
    PLONK_REQUIRE(p && seed, PLONK_ERR_ARG, "bad argument");
    memcpy(p->blinding_src.seed, seed, 32);
    p->blinding_src.seeded = true;
    p->blinding_src.runs = 0;
    return PLONK_OK;
}

// Synchronise and fetch: the proof records (prover.h) and status[B] (0 ok, else PROVER_ST_* bits; with Z_OPEN clear, GATE is exactly
// the condition of the reference's quotient-degree assert, prover.py:205-208).
static int prover_download(plonk_prover* p, size_t B, uint8_t* out_proofs, uint8_t* out_status, bool compressed) {
    PLONK_REQUIRE(p && B && out_proofs && out_status, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(B == p->intake.resident_b, PLONK_ERR_STATE, "download: batch %zu, but %zu witnesses are resident", B, p->intake.resident_b);
    PLONK_ENTER(p->circuit.ctx);
    plonk_ctx* ctx = p->circuit.ctx;
    void* packed;
    PLONK_TRY(ctx_scratch(ctx, 2, B * (proof_bytes(compressed) + 1), &packed));
    uint8_t *d_proofs = (uint8_t*)packed, *d_status = d_proofs + B * proof_bytes(compressed);
    PLONK_TRY(prover_pack_device(p, B, compressed, d_proofs, d_status, nullptr));
    PLONK_CHECK_HIP(hipMemcpyAsync(out_proofs, d_proofs, B * proof_bytes(compressed), hipMemcpyDeviceToHost, ctx->stream));
    PLONK_CHECK_HIP(hipMemcpyAsync(out_status, d_status, B, hipMemcpyDeviceToHost, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return PLONK_OK;
}
int plonk_prover_download(plonk_prover* p, size_t B, uint8_t* out_proofs, uint8_t* out_status) {
    return prover_download(p, B, out_proofs, out_status, false);
}
// the same proofs as compressed records (g1_codec.h)
int plonk_prover_download_compressed(plonk_prover* p, size_t B, uint8_t* out_proofs, uint8_t* out_status) {
    return prover_download(p, B, out_proofs, out_status, true);
}

// Debug / test access: the six challenges of proof b, canonical LE (beta, gamma, alpha, fft_cofactor, zeta, v)
int plonk_prover_challenges(plonk_prover* p, size_t b, uint8_t out_le32[6 * 32]) {
    PLONK_REQUIRE(p && b < p->intake.resident_b && out_le32, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(p->circuit.ctx);
    ProofState st;
    PLONK_CHECK_HIP(hipStreamSynchronize(p->circuit.ctx->stream));
    PLONK_CHECK_HIP(hipMemcpy(&st, p->results.state + b, sizeof st, hipMemcpyDeviceToHost));
    const Fr* ch[6] = {&st.beta, &st.gamma, &st.alpha, &st.fft_cofactor, &st.zeta, &st.v};
    for (int i = 0; i < 6; i++) {
        Fr c = fp_from_mont(*ch[i]);
        memcpy(out_le32 + 32 * i, c.v, 32);
    }
    return PLONK_OK;
}

// DIAGNOSTICS: the automatic number of segments for `batch` proofs of 2^log_n rows on ctx's device
int plonk_prover_plan_segments(plonk_ctx* ctx, unsigned log_n, size_t batch, unsigned* out_segments) {
    PLONK_REQUIRE(ctx && out_segments && batch && log_n >= 1 && log_n <= PROVER_MAX_LOG_N, PLONK_ERR_ARG, "bad argument");
    *out_segments = prover_plan_segments(device_cus(ctx->device), log_n, batch);
    return PLONK_OK;
}

}  // extern "C"

// ---- the fused round kernels on their own: what Prover.round_2 / round_3 of the reference-shaped API call
extern "C" {

// prover.py:121-146: Z_0 = 1, Z_{i+1} = Z_i * num_i / den_i from the wire values and the permutation polynomials
int plonk_fr_grand_product(plonk_ctx* ctx, const void* d_a, const void* d_b, const void* d_c, const void* d_s1, const void* d_s2,
                           const void* d_s3, unsigned log_n, const uint8_t beta_le32[32], const uint8_t gamma_le32[32], void* d_z_out,
                           int* out_closes) {
    PLONK_REQUIRE(ctx && d_a && d_b && d_c && d_s1 && d_s2 && d_s3 && beta_le32 && gamma_le32 && d_z_out && out_closes, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(ctx);
    PLONK_REQUIRE(log_n <= PLONK_FR_TWO_ADICITY, PLONK_ERR_ARG, "size 2^%u exceeds the 2-adicity of Fr", log_n);
    PLONK_REQUIRE(le32_below_modulus(beta_le32, false) && le32_below_modulus(gamma_le32, false), PLONK_ERR_ARG, "challenge is not a canonical Fr value");
    const size_t n = (size_t)1 << log_n;
    const Fr* roots;
    PLONK_TRY(ntt_get_roots(ctx, log_n, false, &roots));
    void* scratch;
    const unsigned S = prover_plan_segments(device_cus(ctx->device), log_n, 1);
    PLONK_TRY(ctx_scratch(ctx, 2, (2 * n + 2 + scan_scratch_elems(1, S)) * sizeof(Fr), &scratch));  // num, den, the closes flag, the segments' carries
    Fr* num = (Fr*)scratch;
    uint32_t* closes = reinterpret_cast<uint32_t*>(num + 2 * n);
    GrandProductIn gp = {{(const Fr*)d_a, (const Fr*)d_b, (const Fr*)d_c}, {(const Fr*)d_s1, (const Fr*)d_s2, (const Fr*)d_s3}};
    RoundChallenges ch;
    ch.beta = fr_from_le32(beta_le32);
    ch.gamma = fr_from_le32(gamma_le32);
    ch.alpha = fp_zero<FrParams>();
    PLONK_TRY(scan_grand_product(ctx->stream, S, gp, roots, nullptr, ch, n, 1, (Fr*)d_z_out, closes, num, num + n, num + 2 * n + 2));
    PLONK_CHECK_HIP(hipGetLastError());
    uint32_t c = 0;
    PLONK_CHECK_HIP(hipMemcpyAsync(&c, closes, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *out_closes = (int)c;
    return PLONK_OK;
}

// prover.py:188-203: QUOT_big = (gate + alpha * permutation + alpha^2 * (Z - 1) L0) / Z_H on the 4n-point coset
// offset * mu^k.  d_evals = the coset extensions (fft_expand, 4n values each) of A, B, C, PI, Z, QL, QR, QM, QO, QC, S1,
// S2, S3, L0 in that order; X_big and 1 / Z_H (four distinct values) are derived from the offset here.
int plonk_fr_quotient(plonk_ctx* ctx, unsigned log_n, const void* const d_evals[14], const uint8_t offset_le32[32],
                      const uint8_t alpha_le32[32], const uint8_t beta_le32[32], const uint8_t gamma_le32[32], void* d_out) {
    PLONK_REQUIRE(ctx && d_evals && offset_le32 && alpha_le32 && beta_le32 && gamma_le32 && d_out, PLONK_ERR_ARG, "bad argument");
    for (int k = 0; k < 14; k++) PLONK_REQUIRE(d_evals[k], PLONK_ERR_ARG, "d_evals[%d] is NULL", k);
    PLONK_ENTER(ctx);
    PLONK_REQUIRE(log_n + 2 <= PLONK_FR_TWO_ADICITY, PLONK_ERR_ARG, "size 2^%u exceeds the 2-adicity of Fr", log_n + 2);
    PLONK_REQUIRE(le32_below_modulus(offset_le32, false) && le32_below_modulus(alpha_le32, false) && le32_below_modulus(beta_le32, false) &&
                      le32_below_modulus(gamma_le32, false), PLONK_ERR_ARG, "offset / challenge is not a canonical Fr value");
    const size_t n4 = (size_t)4 << log_n;
    const Fr off = fr_from_le32(offset_le32), one = fp_one<FrParams>();
    QuotientIn qi = {};  // no circuit labels: the fourteen vectors are the caller's
    for (int k = 0; k < 5; k++) qi.wit[k] = (const Fr*)d_evals[k];
    qi.fixed[FX_QL] = (const Fr*)d_evals[5];
    qi.fixed[FX_QR] = (const Fr*)d_evals[6];
    qi.fixed[FX_QM] = (const Fr*)d_evals[7];
    qi.fixed[FX_QO] = (const Fr*)d_evals[8];
    qi.fixed[FX_QC] = (const Fr*)d_evals[9];
    qi.fixed[FX_S1] = (const Fr*)d_evals[10];
    qi.fixed[FX_S2] = (const Fr*)d_evals[11];
    qi.fixed[FX_S3] = (const Fr*)d_evals[12];
    qi.l0 = (const Fr*)d_evals[13];
    PLONK_TRY(get_power_table(ctx, host_root_of_unity(log_n + 2, false), off, n4, &qi.xs));  // X_big[k] = offset * mu^k
    // Z_H(x_k) = (offset mu^k)^n - 1 = offset^n i^k - 1, i = mu^n: four values (prover.py:178); 1 / 0 == 0 as py_ecc
    Fr on = off;
    for (unsigned i = 0; i < log_n; i++) on = fp_sqr(on);
    const Fr i4 = host_root_of_unity(2, false);
    ZhInv zh;
    Fr cur = on;
    for (int k = 0; k < 4; k++) {
        zh.v[k] = fp_inv(fp_sub(cur, one));
        cur = fp_mul(cur, i4);
    }
    RoundChallenges ch;
    ch.alpha = fr_from_le32(alpha_le32);
    ch.beta = fr_from_le32(beta_le32);
    ch.gamma = fr_from_le32(gamma_le32);
    PLONK_LAUNCH(quotient_kernel, dim3((unsigned)((n4 + 255) / 256), 1), dim3(256), 0, ctx->stream, qi, zh, (const ProofState*)nullptr, ch, (unsigned)n4,
                 (Fr*)d_out, 0u, (unsigned)n4);
    PLONK_CHECK_HIP(hipGetLastError());
    return PLONK_OK;
}

}  // extern "C"

// Packs the resident batch's proof records (plain or compressed) and status bytes into DEVICE memory on the prover's own stream
// and records `done` there, if given: plonk_prover_download, the verifier's load and the send side of plonk_gather_proofs_device.
int prover_pack_device(plonk_prover* p, size_t B, int compressed, uint8_t* d_proofs, uint8_t* d_status, hipEvent_t done) {
    PLONK_REQUIRE(p && B && d_proofs && d_status, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(B == p->intake.resident_b, PLONK_ERR_STATE, "pack: batch %zu, but %zu witnesses are resident", B, p->intake.resident_b);
    plonk_ctx* ctx = p->circuit.ctx;
    const unsigned tb = (unsigned)((B + 63) / 64);
    PLONK_LAUNCH(pack_proofs_kernel, dim3(tb), dim3(64), 0, ctx->stream, (const Fq*)p->results.commit_xy, (const ProofState*)p->results.state, B, d_proofs,
                 compressed ? 1 : 0);
    PLONK_LAUNCH(pack_status_kernel, dim3(tb), dim3(64), 0, ctx->stream, (const ProofState*)p->results.state, (const uint32_t*)p->rounds.closes,
                 (const uint8_t*)p->results.commit_flags, (const unsigned long long*)p->intake.bad_input, p->intake.bad_stride,
                 p->solver.valid ? (const uint32_t*)p->solver.bad : (const uint32_t*)nullptr, B, d_status);
    PLONK_CHECK_HIP(hipGetLastError());
    if (done) PLONK_CHECK_HIP(hipEventRecord(done, ctx->stream));
    return PLONK_OK;
}

plonk_ctx* prover_ctx(plonk_prover* p) { return p->circuit.ctx; }
size_t prover_record_bytes(int compressed) { return proof_bytes(compressed != 0); }

// tests/emu/Makefile compiles verifier.hip as a unit of its own and says so (PLONK_EMU_VERIFIER_UNIT).  A tests/ tree from before
// that unit existed lists the units without it; laid over these sources it must still build the whole library, so there, and only
// there, the verifier is compiled here as it used to be.
#if defined(PLONK_EMU) && !defined(PLONK_EMU_VERIFIER_UNIT)
#include "verifier.hip"
#endif
