// Host-side probe of the pairing tower (pairing_tower.h compiled with g++ via PLONK_EMU) and of the generated constants.
// TEST INFRASTRUCTURE ONLY: lets tests/test_emu_pairing_device.py compare them with Python integers.
// An Fq12 element travels as 12 canonical values of 8 words: the Fq2 coefficient of w^k at [2 k] (real part) and [2 k + 1].
#include <string.h>

#include "fp.h"
#include "pairing_tower.h"

static Fq ld(const uint32_t* p) {
    Fq a;
    memcpy(a.v, p, 32);
    return fp_to_mont(a);
}
static void st(uint32_t* p, const Fq& a) {
    const Fq c = fp_from_mont(a);
    memcpy(p, c.v, 32);
}
static Fq2 ld2(const uint32_t* p) { return Fq2{ld(p), ld(p + 8)}; }
static void st2(uint32_t* p, const Fq2& a) {
    st(p, a.c0);
    st(p + 8, a.c1);
}
static Fq12 ld12(const uint32_t* p) {
    Fq12 a;
    a.c0.c0 = ld2(p);
    a.c1.c0 = ld2(p + 16);
    a.c0.c1 = ld2(p + 32);
    a.c1.c1 = ld2(p + 48);
    a.c0.c2 = ld2(p + 64);
    a.c1.c2 = ld2(p + 80);
    return a;
}
static void st12(uint32_t* p, const Fq12& a) {
    st2(p, a.c0.c0);
    st2(p + 16, a.c1.c0);
    st2(p + 32, a.c0.c1);
    st2(p + 48, a.c1.c1);
    st2(p + 64, a.c0.c2);
    st2(p + 80, a.c1.c2);
}

// op 5: b is the line y + b0 w + b1 w^3 as an Fq12 element (y real, the other coefficients zero)
extern "C" void probe_f12(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const Fq12 x = ld12(a);
    Fq12 r = f12_one();
    switch (op) {
        case 0: r = f12_mul(x, ld12(b)); break;
        case 1: r = f12_sqr(x); break;
        case 2: r = f12_inv(x); break;
        case 3: r = f12_frob2(x); break;
        case 4: r = f12_conj(x); break;
        case 5: r = f12_mul_line(x, ld(b), ld2(b + 16), ld2(b + 48)); break;
    }
    st12(out, r);
}

// gamma[8], gamma2[8], g2[32] canonical; hard_exp[PAIRING_HARD_EXP_WORDS], ate_t[4]; sizes[3] = lines, hard-exponent bits and words
extern "C" void probe_pairing_constants(uint32_t* gamma, uint32_t* gamma2, uint32_t* hard_exp, uint32_t* ate_t, uint32_t* g2, uint32_t* sizes) {
    Fq g, gg, q[4];
    for (int i = 0; i < 8; i++) {
        g.v[i] = pairing_frob2_gamma(i);
        gg.v[i] = pairing_frob2_gamma2(i);
        q[0].v[i] = pairing_g2_gen_x_c0(i);
        q[1].v[i] = pairing_g2_gen_x_c1(i);
        q[2].v[i] = pairing_g2_gen_y_c0(i);
        q[3].v[i] = pairing_g2_gen_y_c1(i);
    }
    st(gamma, g);
    st(gamma2, gg);
    for (int k = 0; k < 4; k++) st(g2 + 8 * k, q[k]);
    for (int i = 0; i < PAIRING_HARD_EXP_WORDS; i++) hard_exp[i] = pairing_hard_exp(i);
    for (int i = 0; i < 4; i++) ate_t[i] = pairing_ate_t(i);
    sizes[0] = PAIRING_ATE_LINES;
    sizes[1] = PAIRING_HARD_EXP_BITS;
    sizes[2] = PAIRING_HARD_EXP_WORDS;
}
