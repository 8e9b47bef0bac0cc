// Stand-alone sanitizer check of the per-lane pairing checks (csrc/pairing_device.h, csrc/pairing_tower.h) on the emulated
// kernels: plonk_pairing_check_many on checks e(a G, [7]_2) e(-(7 a + d) G, [1]_2) == 1, d = 0 (true) and d = 1 (false) in turn,
// a = 1, r - 1 and small multipliers, both sides the identity, one side the identity; counts 1, 2, 7 and 66 (a second workgroup);
// every verdict against the host's plonk_pairing_check on the same four points; the refused arguments.
//   make -C tests/emu -f pairing_sanitize.mk pairing-sanitize      (AddressSanitizer + UBSan, its own main, nothing loaded into Python)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "plonk_hip.h"

#define CHECK(call)                                                                          \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0) {                                                                      \
            fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, plonk_last_error()); \
            exit(1);                                                                         \
        }                                                                                    \
    } while (0)
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// [7]_2 and the generator [1]_2: x.c0 || x.c1 || y.c0 || y.c1, canonical little-endian
static const uint8_t Q7[128] = {
    0x08, 0xb3, 0x28, 0xaa, 0x2a, 0x14, 0x90, 0xc3, 0x89, 0x2a, 0xe3, 0x75, 0xba, 0x53, 0xa2, 0x57, 0x16, 0x2f, 0x1c, 0xde, 0x01, 0x2e, 0x70, 0xed, 0xf8, 0xfc, 0x27, 0x43, 0x5d, 0xdc, 0x4b, 0x22,
    0x55, 0x24, 0x36, 0x46, 0xba, 0xde, 0x3e, 0x59, 0x6d, 0xee, 0x46, 0x6e, 0x51, 0xd4, 0x0f, 0xbe, 0x63, 0x1e, 0x55, 0x84, 0x1e, 0x08, 0x5d, 0x6a, 0xe2, 0xbd, 0x9a, 0x5a, 0x01, 0xba, 0x03, 0x29,
    0x3f, 0x23, 0x14, 0x41, 0x05, 0xe8, 0x21, 0x2e, 0xd8, 0xdf, 0x28, 0xca, 0x0e, 0x80, 0x31, 0xd4, 0x7b, 0x7a, 0x7d, 0xe3, 0x72, 0xb3, 0xcc, 0xee, 0x17, 0x50, 0x26, 0x2a, 0xf5, 0xff, 0x92, 0x1d,
    0xd8, 0xe0, 0x35, 0x03, 0xbe, 0x1e, 0xed, 0xba, 0xad, 0xf7, 0xe6, 0xc4, 0xa1, 0xbe, 0x36, 0x70, 0xd1, 0x4a, 0x46, 0xda, 0x5f, 0xaf, 0xee, 0x7a, 0xdb, 0xde, 0xb2, 0xa6, 0xcd, 0xb7, 0xc8, 0x03,
};
static const uint8_t G2[128] = {
    0xed, 0xf6, 0x92, 0xd9, 0x5c, 0xbd, 0xde, 0x46, 0xdd, 0xda, 0x5e, 0xf7, 0xd4, 0x22, 0x43, 0x67, 0x79, 0x44, 0x5c, 0x5e, 0x66, 0x00, 0x6a, 0x42, 0x76, 0x1e, 0x1f, 0x12, 0xef, 0xde, 0x00, 0x18,
    0xc2, 0x12, 0xf3, 0xae, 0xb7, 0x85, 0xe4, 0x97, 0x12, 0xe7, 0xa9, 0x35, 0x33, 0x49, 0xaa, 0xf1, 0x25, 0x5d, 0xfb, 0x31, 0xb7, 0xbf, 0x60, 0x72, 0x3a, 0x48, 0x0d, 0x92, 0x93, 0x93, 0x8e, 0x19,
    0xaa, 0x7d, 0xfa, 0x66, 0x01, 0xcc, 0xe6, 0x4c, 0x7b, 0xd3, 0x43, 0x0c, 0x69, 0xe7, 0xd1, 0xe3, 0x8f, 0x40, 0xcb, 0x8d, 0x80, 0x71, 0xab, 0x4a, 0xeb, 0x6d, 0x8c, 0xdb, 0xa5, 0x5e, 0xc8, 0x12,
    0x5b, 0x97, 0x22, 0xd1, 0xdc, 0xda, 0xac, 0x55, 0xf3, 0x8e, 0xb3, 0x70, 0x33, 0x31, 0x4b, 0xbc, 0x95, 0x33, 0x0c, 0x69, 0xad, 0x99, 0x9e, 0xec, 0x75, 0xf0, 0x5f, 0x58, 0xd0, 0x89, 0x06, 0x09,
};
// r, little-endian
static const uint8_t R_MOD[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                  0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

// out = +v or r - v (v small and non-zero), canonical little-endian
static void scalar(uint8_t out[32], uint64_t v, bool negative) {
    memset(out, 0, 32);
    memcpy(out, &v, 8);
    if (!negative) return;
    unsigned borrow = 0;
    for (int i = 0; i < 32; i++) {
        const int d = (int)R_MOD[i] - (int)out[i] - (int)borrow;
        borrow = d < 0;
        out[i] = (uint8_t)(d + (borrow ? 256 : 0));
    }
}

int main() {
    plonk_ctx* ctx = nullptr;
    CHECK(plonk_ctx_create(0, &ctx));
    const size_t POOL = 11;
    // check j: a_j, the false ones off by one generator; 8 = both sides the identity, 9 and 10 = one side
    const uint64_t a[POOL] = {1, 1, 1, 1, 2, 3, 5, 1000003, 4, 6, 9};
    const bool a_neg[POOL] = {false, false, true, true, false, false, true, false, false, false, false};  // 2, 3: a = r - 1
    std::vector<uint8_t> gen(2 * POOL * 64, 0), ks(2 * POOL * 32), xy(2 * POOL * 64), ident(2 * POOL);
    for (size_t j = 0; j < 2 * POOL; j++) {
        gen[64 * j] = 1;
        gen[64 * j + 32] = 2;  // G1 = (1, 2)
    }
    for (size_t j = 0; j < POOL; j++) {
        scalar(&ks[32 * (2 * j)], a[j], a_neg[j]);
        // B = -(7 a + d) G: the scalar 7 a + d with the opposite sign; a = r - 1 gives 7 a = r - 7, so -(7 a + d) = 7 - d
        scalar(&ks[32 * (2 * j + 1)], a_neg[j] ? 7 * a[j] - (j % 2) : 7 * a[j] + (j % 2), !a_neg[j]);
    }
    CHECK(plonk_g1_mul_many(ctx, gen.data(), ks.data(), 2 * POOL, xy.data(), ident.data()));
    for (size_t j = 0; j < 2 * POOL; j++) EXPECT(!ident[j]);
    ident[2 * 8] = ident[2 * 8 + 1] = 1;
    ident[2 * 9 + 1] = 1;
    ident[2 * 10] = 1;
    // the host's verdicts
    uint8_t want[POOL];
    for (size_t j = 0; j < POOL; j++) {
        uint8_t g2[256];
        memcpy(g2, Q7, 128);
        memcpy(g2 + 128, G2, 128);
        int ok = -1;
        CHECK(plonk_pairing_check(&xy[64 * 2 * j], &ident[2 * j], g2, 2, &ok));
        want[j] = (uint8_t)ok;
        EXPECT(ok == (j < 9 ? (j % 2 == 0) : 0));
    }
    uint8_t g2[2][128];
    memcpy(g2[0], Q7, 128);
    memcpy(g2[1], G2, 128);
    const size_t counts[4] = {1, 2, 7, 66};
    for (size_t c = 0; c < 4; c++) {
        const size_t n = counts[c];
        std::vector<uint8_t> pts(n * 128), fl(n * 2), got(n, 7);
        for (size_t i = 0; i < n; i++) {
            const size_t j = n == 66 ? (i % 8 == 7 ? 8 + (i / 8) % 3 : i % 2) : (i + 2 * c) % POOL;  // 66: mostly the two cheapest to tell apart
            memcpy(&pts[128 * i], &xy[128 * j], 128);
            memcpy(&fl[2 * i], &ident[2 * j], 2);
            got[i] = want[j] ? 0 : 1;  // the opposite: the call must write every verdict
        }
        CHECK(plonk_pairing_check_many(ctx, g2, pts.data(), fl.data(), n, got.data()));
        for (size_t i = 0; i < n; i++) {
            const size_t j = n == 66 ? (i % 8 == 7 ? 8 + (i / 8) % 3 : i % 2) : (i + 2 * c) % POOL;
            EXPECT(got[i] == want[j]);
        }
    }
    // refused arguments
    uint8_t one[1], bad[2][128], fl0[2] = {0, 0};
    memcpy(bad, g2, 256);
    bad[0][64] ^= 1;  // y.c0 of Q0: off the twist
    EXPECT(plonk_pairing_check_many(ctx, bad, xy.data(), fl0, 1, one) == PLONK_ERR_ARG);
    memcpy(bad, g2, 256);
    memset(bad[1], 0, 128);  // Q1 the identity
    EXPECT(plonk_pairing_check_many(ctx, bad, xy.data(), fl0, 1, one) == PLONK_ERR_ARG);
    EXPECT(plonk_pairing_check_many(ctx, g2, xy.data(), fl0, 0, one) == PLONK_ERR_ARG);
    std::vector<uint8_t> off(xy.begin(), xy.begin() + 128);
    off[32] ^= 1;  // A.y: off the curve
    EXPECT(plonk_pairing_check_many(ctx, g2, off.data(), fl0, 1, one) == PLONK_ERR_ARG);
    memset(&off[0], 0xff, 32);  // A.x >= p
    EXPECT(plonk_pairing_check_many(ctx, g2, off.data(), fl0, 1, one) == PLONK_ERR_ARG);
    CHECK(plonk_ctx_destroy(ctx));
    printf("pairing_sanitize: ok\n");
    return 0;
}
