// Host-side probe of fpl_from_fp_signed (csrc/fpl.h, compiled with g++ via PLONK_EMU: the range checks are on).
// TEST INFRASTRUCTURE ONLY: lets tests/test_emu_fpl_signed.py compare the signed unpack with Python ints.
#include "fp.h"
#include "g1.h"

// limbs[9] of s ? -y : y (s = 0 or ~0), and (+-y) z R^-1 mod m through fpl_mul against the normalised z — the one product the
// signed limbs enter in the mixed addition (S2 = Y2 ZZZ1), with fpl_dbg_check_product's bounds asserted on the way
extern "C" void probe_fpl_signed(const uint32_t* y, uint32_t s, const uint32_t* z, int32_t* limbs, uint32_t* prod) {
    Fq a, b;
    memcpy(a.v, y, 32);
    memcpy(b.v, z, 32);
    const FqL l = fpl_from_fp_signed(a, s);
    for (int i = 0; i < 9; i++) limbs[i] = l.l[i];
    const Fq p = fpl_to_fp(fpl_mul(l, fpl_from_fp(b)));
    memcpy(prod, p.v, 32);
}
