// pairing_device.h — many independent BN254 pairing checks over two FIXED G2 points, one lane per check
// (plonk_pairing_check_many, plonk_verifier_check_each).  Included by verifier.hip alone, like prover.h: kernels and their host side.
//
// The batch verifier needs one pairing product per batch and leaves it on the host (pairing.hip).  Naming the bad proofs of a batch
// that failed is another matter: bisection pays a fold launch and a host pairing per probe, in series, and whoever slips bad proofs
// into a batch sets that cost.  Every proof's own check is e(L_i, [x]_2) == e(R_i, [1]_2) with both G2 points fixed, so the lines of
// the ate loop over them are computed ONCE on the host (affine steps as in pairing.hip: slope L and c = L xR - yR per line, 195 lines
// of 128 B per point) and check i evaluates them at its own two G1 points:
//     f = 1;  per loop bit: f = f^2, f *= line0(A_i), f *= line1(B_i)  (and the two addition lines on a set bit)
//     f = f^((p^6 - 1)(p^2 + 1)): conj(f) / f, then frob2(f) f;   f = f^H, H = (p^4 - p^2 + 1) / r, plain square-and-multiply
//     ok[i] = (f == 1)
// The same Miller functions and the same exponent (p^12 - 1) / r as the host's, split into its three factors.  Every lane reads the
// same table entry at the same step; the loop bounds are uniform, only the identity tests diverge.  An Fq12 is 96 words and a product
// needs three of them and more: the kernel runs one wave per SIMD and spills what does not fit to scratch
// (profiles/verify_kernel_resource_usage.txt).
#pragma once
#include <string.h>

#include <vector>

#include "plonk_internal.h"
#include "pairing_tower.h"

// One line of the ate loop over a fixed Q: the slope at the running point R and c = lambda xR - yR (Montgomery form).  At
// P = (xP, yP) the line is  yP - (lambda xP) w + c w^3.
struct PairingLine { Fq2 lambda, c; };

// f *= the line `ln` of the fixed point at the lane's P = (x, y); nx = -x
PLONK_DEV void pairing_line_step(Fq12& f, const Fq& y, const Fq& nx, const PairingLine* ln) {
    const Fq2 lam = Fq2{fp_load(&ln->lambda.c0), fp_load(&ln->lambda.c1)};
    const Fq2 c = Fq2{fp_load(&ln->c.c0), fp_load(&ln->c.c1)};
    f = f12_mul_line(f, y, f2_mul_fq(lam, nx), c);
}

// ok[i] = 1 iff e(A_i, Q0) e(B_i, Q1) == 1.  pts[2 i] = A_i, pts[2 i + 1] = B_i: affine, Montgomery form, (0, 0) = the identity,
// which contributes nothing (e(O, .) = 1).  lines[0 .. 195) of Q0, lines[195 .. 390) of Q1.  skip (optional): ok[i] = 0 and no
// pairing where skip[i] != 0.
__global__ void __launch_bounds__(64) pairing_check_fixed_kernel(const G1Affine* pts, const PairingLine* lines, const uint8_t* skip, size_t count,
                                                                 uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (skip && skip[i]) {
        ok[i] = 0;
        return;
    }
    G1Affine A, B;
    A.x = fp_load(&pts[2 * i].x);
    A.y = fp_load(&pts[2 * i].y);
    B.x = fp_load(&pts[2 * i + 1].x);
    B.y = fp_load(&pts[2 * i + 1].y);
    const bool has_a = !g1_affine_is_identity(A), has_b = !g1_affine_is_identity(B);
    const Fq nxa = fp_neg(A.x), nxb = fp_neg(B.x);
    Fq12 f = f12_one();
    unsigned e = 0;  // the line of the step; PAIRING_ATE_LINES after the loop
#pragma unroll 1
    for (int bit = 125; bit >= 0; bit--) {  // T has 127 bits: the loop starts below its top bit
        f = f12_sqr(f);
        const unsigned steps = 1 + ((pairing_ate_t(bit >> 5) >> (bit & 31)) & 1);  // the doubling's line, and the addition's on a set bit
#pragma unroll 1
        for (unsigned s = 0; s < steps; s++, e++) {
            if (has_a) pairing_line_step(f, A.y, nxa, lines + e);
            if (has_b) pairing_line_step(f, B.y, nxb, lines + PAIRING_ATE_LINES + e);
        }
    }
    // easy part: f^(p^6 - 1) = conj(f) / f, then ^(p^2 + 1)
    Fq12 t = f12_mul(f12_conj(f), f12_inv(f));
    t = f12_mul(f12_frob2(t), t);
    // hard part: t^H, H's top bit taken by the start value
    f = t;
#pragma unroll 1
    for (int bit = PAIRING_HARD_EXP_BITS - 2; bit >= 0; bit--) {
        f = f12_sqr(f);
        if ((pairing_hard_exp(bit >> 5) >> (bit & 31)) & 1) f = f12_mul(f, t);
    }
    ok[i] = f12_is_one(f) ? 1 : 0;
}

// ================================================================================================
// host side
static_assert(sizeof(PairingLine) == 128, "a line is two Fq2");

static Fq2 pairing_g2_generator_x() {
    Fq2 x;
    for (int i = 0; i < 8; i++) {
        x.c0.v[i] = pairing_g2_gen_x_c0(i);
        x.c1.v[i] = pairing_g2_gen_x_c1(i);
    }
    return x;
}
static Fq2 pairing_g2_generator_y() {
    Fq2 y;
    for (int i = 0; i < 8; i++) {
        y.c0.v[i] = pairing_g2_gen_y_c0(i);
        y.c1.v[i] = pairing_g2_gen_y_c1(i);
    }
    return y;
}

// canonical x.c0 || x.c1 || y.c0 || y.c1 LE -> Montgomery form; the point must lie on the twist y^2 = x^3 + 3 / xi and not be the
// identity (all zero), which has no line table
// PLONK_ERR_ARG: a coordinate >= q, off the twist, the identity
static int pairing_g2_decode(const uint8_t g2_le[128], Fq2* x, Fq2* y) {
    Fq c[4];
    for (int k = 0; k < 4; k++) {
        PLONK_REQUIRE(le32_below_modulus(g2_le + 32 * k, true), PLONK_ERR_ARG, "G2 coordinate %d is >= q", k);
        memcpy(c[k].v, g2_le + 32 * k, 32);
        c[k] = fp_to_mont(c[k]);
    }
    *x = Fq2{c[0], c[1]};
    *y = Fq2{c[2], c[3]};
    PLONK_REQUIRE(!(f2_is_zero(*x) && f2_is_zero(*y)), PLONK_ERR_ARG, "the G2 point is the identity: a fixed line table needs a point");
    const Fq2 b2 = f2_mul(Fq2{fq_small(3), fq_zero()}, f2_inv(Fq2{fq_small(9), fq_one()}));
    PLONK_REQUIRE(f2_eq(f2_sqr(*y), f2_add(f2_mul(f2_sqr(*x), *x), b2)), PLONK_ERR_ARG, "the G2 point is not on the twist");
    return PLONK_OK;
}

// The lines of the ate loop over Q = (qx, qy) in loop order: pairing.hip's miller_loop without the evaluation
static void pairing_line_table(const Fq2& qx, const Fq2& qy, PairingLine* out) {
    Fq2 rx = qx, ry = qy;
    const Fq three = fq_small(3);
    unsigned e = 0;
    for (int bit = 125; bit >= 0; bit--) {
        const Fq2 L = f2_mul(f2_mul_fq(f2_sqr(rx), three), f2_inv(f2_dbl(ry)));
        out[e++] = PairingLine{L, f2_sub(f2_mul(L, rx), ry)};
        const Fq2 nx = f2_sub(f2_sub(f2_sqr(L), rx), rx);
        ry = f2_sub(f2_mul(L, f2_sub(rx, nx)), ry);
        rx = nx;
        if ((pairing_ate_t(bit >> 5) >> (bit & 31)) & 1) {
            const Fq2 La = f2_mul(f2_sub(qy, ry), f2_inv(f2_sub(qx, rx)));
            out[e++] = PairingLine{La, f2_sub(f2_mul(La, rx), ry)};
            const Fq2 ax = f2_sub(f2_sub(f2_sqr(La), rx), qx);
            ry = f2_sub(f2_mul(La, f2_sub(rx, ax)), ry);
            rx = ax;
        }
    }
}

// enqueue: d_ok[i] = (e(pts[2 i], Q0) e(pts[2 i + 1], Q1) == 1), i < count; d_lines = the tables of Q0 and Q1 one after the other;
// d_skip may be null
static int pairing_check_fixed_launch(hipStream_t s, const G1Affine* d_pts, const PairingLine* d_lines, const uint8_t* d_skip, size_t count, uint8_t* d_ok) {
    PLONK_LAUNCH(pairing_check_fixed_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, d_pts, d_lines, d_skip, count, d_ok);
    PLONK_CHECK_HIP(hipGetLastError());
    return PLONK_OK;
}

extern "C" {

int plonk_pairing_check_many(plonk_ctx* ctx, const uint8_t g2_le[2][128], const uint8_t* g1_xy_le, const uint8_t* g1_is_identity, size_t count,
                             uint8_t* out_ok) {
    PLONK_REQUIRE(ctx && g2_le && g1_xy_le && g1_is_identity && out_ok && count, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(count <= ((size_t)1 << 31), PLONK_ERR_ARG, "%zu checks: at most 2^31 per call", count);
    PLONK_ENTER(ctx);
    std::vector<PairingLine> lines(2 * PAIRING_ATE_LINES);
    for (int k = 0; k < 2; k++) {
        Fq2 x, y;
        PLONK_TRY(pairing_g2_decode(g2_le[k], &x, &y));
        pairing_line_table(x, y, lines.data() + k * PAIRING_ATE_LINES);
    }
    const Fq three = fq_small(3);
    std::vector<G1Affine> pts(2 * count);
    for (size_t j = 0; j < 2 * count; j++) {
        const uint8_t* p = g1_xy_le + 64 * j;
        PLONK_REQUIRE(le32_below_modulus(p, true) && le32_below_modulus(p + 32, true), PLONK_ERR_ARG, "G1 point %zu.%zu: a coordinate is >= q", j / 2, j % 2);
        if (g1_is_identity[j]) {
            pts[j] = g1_affine_identity();
            continue;
        }
        Fq x, y;
        memcpy(x.v, p, 32);
        memcpy(y.v, p + 32, 32);
        pts[j].x = fp_to_mont(x);
        pts[j].y = fp_to_mont(y);
        PLONK_REQUIRE(fp_eq(fp_sqr(pts[j].y), fp_add(fp_mul(fp_sqr(pts[j].x), pts[j].x), three)), PLONK_ERR_ARG, "G1 point %zu.%zu is not on the curve", j / 2,
                      j % 2);
    }
    const size_t line_bytes = lines.size() * sizeof(PairingLine), pt_bytes = pts.size() * sizeof(G1Affine);
    void* buf;
    PLONK_TRY(ctx_scratch(ctx, 3, line_bytes + pt_bytes + count, &buf));
    PairingLine* d_lines = (PairingLine*)buf;
    G1Affine* d_pts = (G1Affine*)(d_lines + lines.size());
    uint8_t* d_ok = (uint8_t*)(d_pts + pts.size());
    hipStream_t s = ctx->stream;
    PLONK_CHECK_HIP(hipMemcpyAsync(d_lines, lines.data(), line_bytes, hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipMemcpyAsync(d_pts, pts.data(), pt_bytes, hipMemcpyHostToDevice, s));
    int rc = pairing_check_fixed_launch(s, d_pts, d_lines, nullptr, count, d_ok);
    if (rc == PLONK_OK && hipMemcpyAsync(out_ok, d_ok, count, hipMemcpyDeviceToHost, s) != hipSuccess) {
        plonk_set_error("copying %zu verdicts back failed", count);
        rc = PLONK_ERR_HIP;
    }
    // the staging vectors are the sources of asynchronous copies: wait before they go, whatever happened
    const hipError_t e = hipStreamSynchronize(s);
    if (rc != PLONK_OK) return rc;
    PLONK_CHECK_HIP(e);
    return PLONK_OK;
}

}  // extern "C"
