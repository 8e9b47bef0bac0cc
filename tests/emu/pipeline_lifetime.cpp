// Stand-alone sanitizer check of the two-slot intake (csrc/prover_intake.h: plonk_prover_stage_inputs / _stage_variables /
// _advance) on the emulated kernels: who owns which of the two sets of intake buffers, and which event, while batches are staged,
// advanced, re-staged larger, crossed by a plain upload, re-planned, and while a prover is destroyed with a batch staged.
//   make -C tests/emu -f pipeline_sanitize.mk pipeline-sanitize   (AddressSanitizer + UBSan, its own main, nothing loaded into Python)
// The circuit: 16 rows, x_{i+1} <== x_i + x_i for i < 8, nine variables, the input x0.
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

static const size_t N = 16, ROWS = 8, V = 9, MAXB = 7;
static void put_u64(uint8_t* le32, uint64_t v) {
    memset(le32, 0, 32);
    memcpy(le32, &v, 8);
}
// r - 1, little-endian
static const uint8_t R_MINUS_1[32] = {0x00, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                      0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

static plonk_prover* make_prover(plonk_ctx* ctx, plonk_srs* srs) {
    std::vector<uint8_t> sel(8 * N * 32, 0);  // QM, QL, QR, QO, QC, S1, S2, S3
    for (size_t i = 0; i < ROWS; i++) {
        put_u64(&sel[(1 * N + i) * 32], 1);
        put_u64(&sel[(2 * N + i) * 32], 1);
        memcpy(&sel[(3 * N + i) * 32], R_MINUS_1, 32);
    }
    plonk_prover* p = nullptr;
    CHECK(plonk_prover_create(ctx, srs, 4, sel.data(), 0, &p));
    std::vector<uint32_t> cell(3 * N, (uint32_t)V);
    for (size_t i = 0; i < ROWS; i++) {
        cell[i] = cell[N + i] = (uint32_t)i;
        cell[2 * N + i] = (uint32_t)i + 1;
    }
    CHECK(plonk_prover_set_wiring(p, cell.data(), nullptr, V));
    return p;
}

// batch `salt` of B proofs: x0 = 3 + 5 b + 100 salt, every other variable the doubled one
static uint64_t value(size_t salt, size_t b, size_t var) { return (uint64_t)(3 + 5 * b + 100 * salt) << var; }
static void fill(size_t salt, size_t B, uint8_t* in, uint8_t* vars) {
    for (size_t b = 0; b < B; b++) {
        put_u64(in + b * 32, value(salt, b, 0));
        for (size_t v = 0; v < V; v++) put_u64(vars + (b * V + v) * 32, value(salt, b, v));
    }
}

// the resident batch is batch `salt` of B: its variables, its verdicts, and its rounds run and download
static void expect_resident(plonk_prover* p, size_t salt, size_t B, bool prove) {
    std::vector<uint8_t> in(B * 32), want(B * V * 32), got(B * V * 32), proofs(B * 768), status(B);
    std::vector<uint32_t> rows(B, 99);
    fill(salt, B, in.data(), want.data());
    CHECK(plonk_prover_download_variables(p, B, nullptr, 0, got.data()));
    EXPECT(!memcmp(got.data(), want.data(), want.size()));
    CHECK(plonk_prover_solve_failures(p, B, rows.data()));
    for (size_t b = 0; b < B; b++) EXPECT(rows[b] == 0);
    if (!prove) return;
    CHECK(plonk_prover_run(p, B));
    CHECK(plonk_prover_download(p, B, proofs.data(), status.data()));
    for (size_t b = 0; b < B; b++) EXPECT(!(status[b] & (8 | 16)));  // (this circuit has no permutation: the other bits are not its subject)
}

int main() {
    plonk_ctx* ctx;
    CHECK(plonk_ctx_create(0, &ctx));
    std::vector<uint8_t> bases(N * 64, 0);  // the generator (1, 2), sixteen times
    for (size_t i = 0; i < N; i++) {
        bases[64 * i] = 1;
        bases[64 * i + 32] = 2;
    }
    plonk_srs* srs;
    CHECK(plonk_srs_load_affine(ctx, bases.data(), N, &srs));
    void *pin_in[2], *pin_vars[2];
    for (int i = 0; i < 2; i++) {
        CHECK(plonk_host_alloc(ctx, MAXB * 32, &pin_in[i]));
        CHECK(plonk_host_alloc(ctx, MAXB * V * 32, &pin_vars[i]));
    }
    const uint32_t input = 0;
    uint32_t missing = 0;
    size_t staged = 99, B = 0;

    plonk_prover* p = make_prover(ctx, srs);
    EXPECT(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[0], 1) == PLONK_ERR_STATE);  // no plan
    CHECK(plonk_prover_set_inputs(p, &input, 1, &missing));
    EXPECT(plonk_prover_advance(p, &B) == PLONK_ERR_STATE);
    CHECK(plonk_prover_staged(p, &staged));
    EXPECT(staged == 0);
    // the first batch through the second slot; then alternately from inputs and from packed variables, smaller and larger
    const size_t sizes[6] = {2, 5, 1, 5, 7, 2};
    fill(0, sizes[0], (uint8_t*)pin_in[0], (uint8_t*)pin_vars[0]);
    CHECK(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[0], sizes[0]));
    CHECK(plonk_prover_advance(p, &B));
    EXPECT(B == sizes[0]);
    for (size_t k = 0; k < 6; k++) {
        const bool prove = sizes[k] <= 2;  // the rounds are what costs time on the emulated kernels: the small batches run them
        if (prove) CHECK(plonk_prover_run(p, sizes[k]));
        if (k + 1 < 6) {
            const size_t nb = sizes[k + 1], slot = (k + 1) & 1;
            fill(k + 1, nb, (uint8_t*)pin_in[slot], (uint8_t*)pin_vars[slot]);
            if (k & 1) CHECK(plonk_prover_stage_variables(p, (const uint8_t*)pin_vars[slot], nb));
            else CHECK(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[slot], nb));
            CHECK(plonk_prover_staged(p, &staged));
            EXPECT(staged == nb);
            EXPECT(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[slot], nb) == PLONK_ERR_STATE);  // one staged batch at a time
            EXPECT(plonk_prover_set_inputs(p, &input, 1, &missing) == PLONK_ERR_STATE);
        }
        expect_resident(p, k, sizes[k], prove);  // still batch k, with k + 1 staged
        if (k + 1 < 6) {
            CHECK(plonk_prover_advance(p, &B));
            EXPECT(B == sizes[k + 1]);
        }
    }
    // a plain upload, larger than anything before, between stage and advance: it reallocates the resident set and the rounds' buffers
    fill(20, 3, (uint8_t*)pin_in[0], (uint8_t*)pin_vars[0]);
    CHECK(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[0], 3));
    std::vector<uint8_t> in(MAXB * 2 * 32), vars(MAXB * 2 * V * 32);
    fill(21, 2 * MAXB, in.data(), vars.data());
    CHECK(plonk_prover_upload_inputs(p, in.data(), 2 * MAXB));
    expect_resident(p, 21, 2 * MAXB, false);
    CHECK(plonk_prover_advance(p, &B));
    EXPECT(B == 3);
    expect_resident(p, 20, 3, true);
    // a new plan with nothing staged: the inputs' buffers of BOTH sets go; then the pipeline again, advance before any download
    CHECK(plonk_prover_set_inputs(p, &input, 1, &missing));
    fill(30, 1, (uint8_t*)pin_in[0], (uint8_t*)pin_vars[0]);
    CHECK(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[0], 1));
    CHECK(plonk_prover_advance(p, &B));
    CHECK(plonk_prover_run(p, 1));
    fill(31, 4, (uint8_t*)pin_in[1], (uint8_t*)pin_vars[1]);
    CHECK(plonk_prover_stage_inputs(p, (const uint8_t*)pin_in[1], 4));
    CHECK(plonk_prover_advance(p, &B));  // gives up batch 30's results
    expect_resident(p, 31, 4, false);
    // destroyed with a batch staged and never advanced
    fill(32, 6, (uint8_t*)pin_in[0], (uint8_t*)pin_vars[0]);
    CHECK(plonk_prover_stage_variables(p, (const uint8_t*)pin_vars[0], 6));
    CHECK(plonk_prover_destroy(p));

    plonk_prover* only_staged = make_prover(ctx, srs);  // a batch staged into a prover that never had a resident one
    CHECK(plonk_prover_set_inputs(only_staged, &input, 1, &missing));
    fill(40, 2, (uint8_t*)pin_in[0], (uint8_t*)pin_vars[0]);
    CHECK(plonk_prover_stage_inputs(only_staged, (const uint8_t*)pin_in[0], 2));
    CHECK(plonk_prover_destroy(only_staged));

    for (int i = 0; i < 2; i++) {
        CHECK(plonk_host_free(ctx, pin_in[i]));
        CHECK(plonk_host_free(ctx, pin_vars[i]));
    }
    CHECK(plonk_srs_free(ctx, srs));
    CHECK(plonk_ctx_destroy(ctx));
    printf("pipeline_lifetime ok\n");
    return 0;
}
