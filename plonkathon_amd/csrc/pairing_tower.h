// pairing_tower.h — the extension tower of the BN254 pairing, for host and device code alike.
//
//   Fq2 = Fq[i] / (i^2 + 1),   Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + i,   Fq12 = Fq6[w] / (w^2 - v)     (so w^6 = xi)
// An Fq12 element c0 + c1 w holds the coefficients of w^0 .. w^5 as c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2.
// Used by the host pairing product (pairing.hip) and by the per-lane checks on the device (pairing_device.h).  Coefficients are
// named struct members, never arrays indexed at run time: an Fq12 is 96 words and lives in registers or in a lane's scratch as
// the compiler sees fit, but nothing forces it there.  On the device a 254-bit multiplication is ~330 instructions, so the
// products from Fq2 upwards are calls (PLONK_HD_NOINLINE): inlined, one Fq12 product alone would be larger than the instruction cache.
#pragma once
#include "fp.h"
#include "pairing_device_constants.h"

struct Fq2 { Fq c0, c1; };
struct Fq6 { Fq2 c0, c1, c2; };
struct Fq12 { Fq6 c0, c1; };

PLONK_HD Fq fq_zero() { return fp_zero<FqParams>(); }
PLONK_HD Fq fq_one() { return fp_one<FqParams>(); }
inline Fq fq_small(uint32_t k) {  // host: a small integer in Montgomery form
    Fq a = fq_zero();
    a.v[0] = k;
    return fp_to_mont(a);
}

PLONK_HD Fq2 f2_zero() { return Fq2{fq_zero(), fq_zero()}; }
PLONK_HD Fq2 f2_one() { return Fq2{fq_one(), fq_zero()}; }
PLONK_HD bool f2_is_zero(const Fq2& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
PLONK_HD bool f2_eq(const Fq2& a, const Fq2& b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }
PLONK_HD Fq2 f2_add(const Fq2& a, const Fq2& b) { return Fq2{fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
PLONK_HD Fq2 f2_sub(const Fq2& a, const Fq2& b) { return Fq2{fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)}; }
PLONK_HD Fq2 f2_neg(const Fq2& a) { return Fq2{fp_neg(a.c0), fp_neg(a.c1)}; }
PLONK_HD Fq2 f2_dbl(const Fq2& a) { return Fq2{fp_dbl(a.c0), fp_dbl(a.c1)}; }
PLONK_HD_NOINLINE Fq2 f2_mul(const Fq2 a, const Fq2 b) {  // (a0 + a1 i)(b0 + b1 i), i^2 = -1
    const Fq t0 = fp_mul(a.c0, b.c0), t1 = fp_mul(a.c1, b.c1);
    const Fq s = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
    return Fq2{fp_sub(t0, t1), fp_sub(fp_sub(s, t0), t1)};
}
PLONK_HD_NOINLINE Fq2 f2_sqr(const Fq2 a) {  // (a0 + a1)(a0 - a1) + 2 a0 a1 i
    const Fq m = fp_mul(a.c0, a.c1);
    return Fq2{fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1)), fp_dbl(m)};
}
PLONK_HD_NOINLINE Fq2 f2_mul_fq(const Fq2 a, const Fq k) { return Fq2{fp_mul(a.c0, k), fp_mul(a.c1, k)}; }
PLONK_HD Fq2 f2_mul_xi(const Fq2& a) {  // (9 + i)(a0 + a1 i) = (9 a0 - a1) + (9 a1 + a0) i, 9 x = 8 x + x by doublings
    const Fq n0 = fp_add(fp_dbl(fp_dbl(fp_dbl(a.c0))), a.c0), n1 = fp_add(fp_dbl(fp_dbl(fp_dbl(a.c1))), a.c1);
    return Fq2{fp_sub(n0, a.c1), fp_add(n1, a.c0)};
}
PLONK_HD Fq2 f2_inv(const Fq2& a) {  // conj(a) / (a0^2 + a1^2)
    const Fq n = fp_inv(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
    return Fq2{fp_mul(a.c0, n), fp_neg(fp_mul(a.c1, n))};
}

PLONK_HD Fq6 f6_zero() { return Fq6{f2_zero(), f2_zero(), f2_zero()}; }
PLONK_HD Fq6 f6_add(const Fq6& a, const Fq6& b) { return Fq6{f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
PLONK_HD Fq6 f6_sub(const Fq6& a, const Fq6& b) { return Fq6{f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
PLONK_HD Fq6 f6_neg(const Fq6& a) { return Fq6{f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
PLONK_HD_NOINLINE Fq6 f6_mul(const Fq6& a, const Fq6& b) {  // v^3 = xi
    const Fq2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    const Fq2 m12 = f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), t1), t2);  // a1 b2 + a2 b1
    const Fq2 m01 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), t0), t1);  // a0 b1 + a1 b0
    const Fq2 m02 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), t0), t2);  // a0 b2 + a2 b0
    return Fq6{f2_add(t0, f2_mul_xi(m12)), f2_add(m01, f2_mul_xi(t2)), f2_add(m02, t1)};
}
// a (b0 + b1 v): the product with an element whose v^2 coefficient is zero (five Fq2 products for six)
PLONK_HD_NOINLINE Fq6 f6_mul_sparse(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 t0 = f2_mul(a.c0, b0), t1 = f2_mul(a.c1, b1);
    const Fq2 m01 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b0, b1)), t0), t1);  // a0 b1 + a1 b0
    return Fq6{f2_add(t0, f2_mul_xi(f2_mul(a.c2, b1))), m01, f2_add(f2_mul(a.c2, b0), t1)};
}
PLONK_HD Fq6 f6_mul_fq(const Fq6& a, const Fq& k) { return Fq6{f2_mul_fq(a.c0, k), f2_mul_fq(a.c1, k), f2_mul_fq(a.c2, k)}; }
PLONK_HD Fq6 f6_mul_v(const Fq6& a) { return Fq6{f2_mul_xi(a.c2), a.c0, a.c1}; }
// 1 / (c0 + c1 v + c2 v^2) = (A + B v + C v^2) / F:  A = c0^2 - xi c1 c2,  B = xi c2^2 - c0 c1,  C = c1^2 - c0 c2,
// F = c0 A + xi (c2 B + c1 C) in Fq2
PLONK_HD_NOINLINE Fq6 f6_inv(const Fq6& a) {
    const Fq2 A = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2 B = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    const Fq2 C = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    const Fq2 F = f2_add(f2_mul(a.c0, A), f2_mul_xi(f2_add(f2_mul(a.c2, B), f2_mul(a.c1, C))));
    const Fq2 Fi = f2_inv(F);
    return Fq6{f2_mul(A, Fi), f2_mul(B, Fi), f2_mul(C, Fi)};
}

PLONK_HD Fq12 f12_one() { return Fq12{Fq6{f2_one(), f2_zero(), f2_zero()}, f6_zero()}; }
PLONK_HD_NOINLINE Fq12 f12_mul(const Fq12& a, const Fq12& b) {  // w^2 = v
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    const Fq6 m = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1);
    return Fq12{f6_add(t0, f6_mul_v(t1)), m};
}
// complex squaring over Fq6: (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - t - v t + 2 t w,  t = a0 a1
PLONK_HD_NOINLINE Fq12 f12_sqr(const Fq12& a) {
    const Fq6 t = f6_mul(a.c0, a.c1);
    const Fq6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return Fq12{f6_sub(f6_sub(s, t), f6_mul_v(t)), f6_add(t, t)};
}
// a (y + b0 w + b1 w^3), y in Fq: the product with the line  yP - (L xP) w + (L xR - yR) w^3  of a Miller step.  As an Fq12
// the line is (y, 0, 0) + (b0, b1, 0) w.
PLONK_HD_NOINLINE Fq12 f12_mul_line(const Fq12& a, const Fq& y, const Fq2& b0, const Fq2& b1) {
    const Fq6 t0 = f6_mul_fq(a.c0, y), t1 = f6_mul_sparse(a.c1, b0, b1);
    const Fq6 m = f6_sub(f6_sub(f6_mul_sparse(f6_add(a.c0, a.c1), Fq2{fp_add(b0.c0, y), b0.c1}, b1), t0), t1);
    return Fq12{f6_add(t0, f6_mul_v(t1)), m};
}
PLONK_HD Fq12 f12_conj(const Fq12& a) { return Fq12{a.c0, f6_neg(a.c1)}; }  // the p^6-power Frobenius: w -> -w
// 1 / (a0 + a1 w) = (a0 - a1 w) / (a0^2 - v a1^2): one inversion in Fq all told (f6_inv -> f2_inv -> fp_inv)
PLONK_HD_NOINLINE Fq12 f12_inv(const Fq12& a) {
    const Fq6 d = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return Fq12{f6_mul(a.c0, d), f6_neg(f6_mul(a.c1, d))};
}
// The p^2-power Frobenius: the coefficient of w^k times gamma^k; gamma^3 = -1, so 1, g, g^2, -1, -g, -g^2 for k = 0 .. 5
PLONK_HD_NOINLINE Fq12 f12_frob2(const Fq12& a) {
    Fq g, g2;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        g.v[i] = pairing_frob2_gamma(i);
        g2.v[i] = pairing_frob2_gamma2(i);
    }
    Fq12 r;
    r.c0.c0 = a.c0.c0;                          // w^0
    r.c1.c0 = f2_mul_fq(a.c1.c0, g);            // w^1
    r.c0.c1 = f2_mul_fq(a.c0.c1, g2);           // w^2
    r.c1.c1 = f2_neg(a.c1.c1);                  // w^3
    r.c0.c2 = f2_neg(f2_mul_fq(a.c0.c2, g));    // w^4
    r.c1.c2 = f2_neg(f2_mul_fq(a.c1.c2, g2));   // w^5
    return r;
}
PLONK_HD bool f12_is_one(const Fq12& a) {
    return fp_eq(a.c0.c0.c0, fq_one()) && fp_is_zero(a.c0.c0.c1) && f2_is_zero(a.c0.c1) && f2_is_zero(a.c0.c2) && f2_is_zero(a.c1.c0) &&
           f2_is_zero(a.c1.c1) && f2_is_zero(a.c1.c2);
}
PLONK_HD bool f12_eq(const Fq12& a, const Fq12& b) {
    return f2_eq(a.c0.c0, b.c0.c0) && f2_eq(a.c0.c1, b.c0.c1) && f2_eq(a.c0.c2, b.c0.c2) && f2_eq(a.c1.c0, b.c1.c0) && f2_eq(a.c1.c1, b.c1.c1) &&
           f2_eq(a.c1.c2, b.c1.c2);
}
