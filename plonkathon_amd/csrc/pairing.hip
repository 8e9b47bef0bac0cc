// pairing.hip — BN254 pairing-product check on the HOST, for the verifier (first half).
//
// Reference behaviour replaced: the `b.pairing(...)` calls of the verifier,
// /root/reference/TESTING_verifier_DO_NOT_OPEN.py:148-160 (one check e(A, [x]_2) == e(B, [1]_2)) and
// :237-262 (two such checks) — i.e. py_ecc.bn128.pairing, a third-party dependency that is not under
// /root/reference.  A verifier only ever asks whether a PRODUCT of pairings is the identity, which is the same
// question for every bilinear non-degenerate pairing on G1 x G2, so this file implements the simplest one:
//     ate pairing      a(Q, P) = f_{T,Q}(P) ^ ((p^12 - 1) / r),     T = t - 1 = 6u^2   (127 bits),
// instead of py_ecc's optimal-ate loop with its two Frobenius steps: no Frobenius maps and no Fq12 inversion are
// needed anywhere.  Tower: Fq2 = Fq[i]/(i^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), xi = 9 + i, Fq12 = Fq6[w]/(w^2 - v);
// G2 lives on the D-type twist y^2 = x^3 + 3/xi over Fq2 and maps to E(Fq12) by (x, y) -> (x w^2, y w^3).  The
// Miller loop runs on affine twist coordinates (one Fq2 inversion per step: this is host code, off the prover
// hot path, ~0.1 s per check) and the line through R with twist slope L evaluated at P = (xP, yP) is
//     yP - (L xP) w + (L xR - yR) w^3         (vertical lines vanish under the final exponentiation).
// The final exponentiation is a plain square-and-multiply by the 2790-bit constant of pairing_constants.h.
// Runs on the CPU by design ("Verifier + pairing on CPU"); it shares fp.h with the kernels
// (the field templates are __host__ __device__) and the tower of pairing_tower.h with the per-lane checks of pairing_device.h,
// and nothing with oracle/.
#include <string.h>

#include "pairing_constants.h"
#include "plonk_internal.h"
#include "pairing_tower.h"

namespace {

struct G2Aff { Fq2 x, y; bool inf; };

// line through R (slope L on the twist) at P:  yP - (L xP) w + (L xR - yR) w^3,   w^3 = w v
inline Fq12 line_value(const Fq2& L, const G2Aff& R, const Fq& xP, const Fq& yP) {
    Fq12 l;
    l.c0 = Fq6{Fq2{yP, fq_zero()}, f2_zero(), f2_zero()};
    l.c1 = Fq6{f2_neg(f2_mul_fq(L, xP)), f2_sub(f2_mul(L, R.x), R.y), f2_zero()};
    return l;
}

// f_{T,Q}(P) for the 127-bit T = t - 1; Q on the twist (not the identity), P = (xP, yP) in G1 (not the identity)
Fq12 miller_loop(const G2Aff& Q, const Fq& xP, const Fq& yP) {
    Fq12 f = f12_one();
    G2Aff R = Q;
    const Fq three = fq_small(3);
    for (int bit = (int)PAIRING_ATE_T_BITS - 2; bit >= 0; bit--) {
        // doubling step: slope 3 xR^2 / (2 yR); a point of odd prime order never has yR == 0
        const Fq2 L = f2_mul(f2_mul_fq(f2_mul(R.x, R.x), three), f2_inv(f2_add(R.y, R.y)));
        f = f12_mul(f12_mul(f, f), line_value(L, R, xP, yP));
        const Fq2 nx = f2_sub(f2_sub(f2_mul(L, L), R.x), R.x);
        R.y = f2_sub(f2_mul(L, f2_sub(R.x, nx)), R.y);
        R.x = nx;
        if ((PAIRING_ATE_T[bit >> 5] >> (bit & 31)) & 1) {
            // addition step R + Q (R != +-Q inside the loop for points of order r, T < r)
            const Fq2 La = f2_mul(f2_sub(Q.y, R.y), f2_inv(f2_sub(Q.x, R.x)));
            f = f12_mul(f, line_value(La, R, xP, yP));
            const Fq2 ax = f2_sub(f2_sub(f2_mul(La, La), R.x), Q.x);
            R.y = f2_sub(f2_mul(La, f2_sub(R.x, ax)), R.y);
            R.x = ax;
        }
    }
    return f;
}

Fq12 final_exponentiation(const Fq12& f) {
    Fq12 r = f12_one();
    for (int bit = (int)PAIRING_FINAL_EXP_BITS - 1; bit >= 0; bit--) {
        r = f12_mul(r, r);
        if ((PAIRING_FINAL_EXP[bit >> 5] >> (bit & 31)) & 1) r = f12_mul(r, f);
    }
    return r;
}

bool le32_lt_q(const uint8_t* b) {
    uint32_t v[8];
    memcpy(v, b, 32);
    for (int i = 7; i >= 0; i--) {
        if (v[i] < FqParams::mod(i)) return true;
        if (v[i] > FqParams::mod(i)) return false;
    }
    return false;
}
Fq fq_from_le32(const uint8_t* b) {
    Fq a;
    memcpy(a.v, b, 32);
    return fp_to_mont(a);
}

}  // namespace

extern "C" {

// out_ok = 1 iff  prod_i e(P_i, Q_i) == 1.  P_i: affine canonical x||y LE (64 B) + identity flag; Q_i: affine canonical
// x.c0 || x.c1 || y.c0 || y.c1 LE (128 B, py_ecc FQ2 coefficient order), all-zero = the identity.  Points are checked
// to lie on their curves (PLONK_ERR_ARG otherwise); subgroup membership of Q is the caller's business (verification
// keys come from the SRS).
int plonk_pairing_check(const uint8_t* g1_xy_le, const uint8_t* g1_is_identity, const uint8_t* g2_le, size_t k, int* out_ok) {
    PLONK_REQUIRE(g1_xy_le && g1_is_identity && g2_le && out_ok && k, PLONK_ERR_ARG, "bad argument");
    const Fq three = fq_small(3);
    // b' = 3 / xi on the twist
    const Fq2 b2 = f2_mul(Fq2{three, fq_zero()}, f2_inv(Fq2{fq_small(9), fq_one()}));
    Fq12 acc = f12_one();
    for (size_t i = 0; i < k; i++) {
        for (int c = 0; c < 2; c++)
            PLONK_REQUIRE(le32_lt_q(g1_xy_le + 64 * i + 32 * c), PLONK_ERR_ARG, "G1 coordinate %zu.%d is >= q", i, c);
        for (int c = 0; c < 4; c++)
            PLONK_REQUIRE(le32_lt_q(g2_le + 128 * i + 32 * c), PLONK_ERR_ARG, "G2 coordinate %zu.%d is >= q", i, c);
        G2Aff Q;
        Q.x = Fq2{fq_from_le32(g2_le + 128 * i), fq_from_le32(g2_le + 128 * i + 32)};
        Q.y = Fq2{fq_from_le32(g2_le + 128 * i + 64), fq_from_le32(g2_le + 128 * i + 96)};
        Q.inf = f2_is_zero(Q.x) && f2_is_zero(Q.y);
        if (g1_is_identity[i] || Q.inf) continue;  // e(O, Q) = e(P, O) = 1
        const Fq xP = fq_from_le32(g1_xy_le + 64 * i), yP = fq_from_le32(g1_xy_le + 64 * i + 32);
        PLONK_REQUIRE(fp_eq(fp_sqr(yP), fp_add(fp_mul(fp_sqr(xP), xP), three)), PLONK_ERR_ARG, "G1 point %zu is not on the curve", i);
        PLONK_REQUIRE(f2_eq(f2_mul(Q.y, Q.y), f2_add(f2_mul(f2_mul(Q.x, Q.x), Q.x), b2)), PLONK_ERR_ARG,
                      "G2 point %zu is not on the twist", i);
        acc = f12_mul(acc, miller_loop(Q, xP, yP));
    }
    *out_ok = f12_is_one(final_exponentiation(acc)) ? 1 : 0;
    return PLONK_OK;
}

}  // extern "C"
