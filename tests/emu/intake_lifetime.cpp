// Stand-alone sanitizer check of the prover's intake (csrc/prover_intake.h) on the emulated kernels: who owns which device buffer
// and which event, across growing and shrinking batches, a second plan, and a prover that never sees an upload.
//   make -C tests/emu intake-sanitize      (sanitize.mk: AddressSanitizer + UBSan, its own main, nothing loaded into Python)
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

static const size_t N = 16, ROWS = 8, V = 9;
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
    return p;
}

static uint64_t value(size_t b, size_t var) { return (uint64_t)(3 + 5 * b) << var; }

int main() {
    plonk_ctx* ctx;
    CHECK(plonk_ctx_create(0, &ctx));
    std::vector<uint8_t> bases(N * 64, 0);  // the generator (1, 2), sixteen times: nothing is committed here
    for (size_t i = 0; i < N; i++) {
        bases[64 * i] = 1;
        bases[64 * i + 32] = 2;
    }
    plonk_srs* srs;
    CHECK(plonk_srs_load_affine(ctx, bases.data(), N, &srs));

    plonk_prover* p = make_prover(ctx, srs);
    std::vector<uint32_t> cell(3 * N, (uint32_t)V);
    for (size_t i = 0; i < ROWS; i++) {
        cell[i] = cell[N + i] = (uint32_t)i;
        cell[2 * N + i] = (uint32_t)i + 1;
    }
    CHECK(plonk_prover_set_wiring(p, cell.data(), nullptr, V));
    const uint32_t input = 0;
    uint32_t missing = 0;
    CHECK(plonk_prover_set_inputs(p, &input, 1, &missing));

    const size_t MAXB = 5;
    void *pin_in, *pin_vars;
    CHECK(plonk_host_alloc(ctx, MAXB * 32, &pin_in));
    CHECK(plonk_host_alloc(ctx, MAXB * V * 32, &pin_vars));
    std::vector<uint8_t> got(MAXB * V * 32);
    std::vector<uint32_t> rows(MAXB);
    const size_t sizes[3] = {2, 5, 1};
    for (int pass = 0; pass < 2; pass++) {
        for (size_t B : sizes) {
            std::vector<uint8_t> in(B * 32), vars(B * V * 32), abc(3 * B * N * 32, 0);
            for (size_t b = 0; b < B; b++) {
                put_u64(&in[b * 32], value(b, 0));
                for (size_t v = 0; v < V; v++) put_u64(&vars[(b * V + v) * 32], value(b, v));
                for (size_t k = 0; k < 3 * N; k++)
                    if (cell[k] < V) put_u64(&abc[((k / N * B + b) * N + k % N) * 32], value(b, cell[k]));
            }
            // inputs: the solver's values are the doubled ones
            CHECK(plonk_prover_upload_inputs(p, in.data(), B));
            CHECK(plonk_prover_download_variables(p, B, nullptr, 0, got.data()));
            if (memcmp(got.data(), vars.data(), vars.size())) {
                fprintf(stderr, "solved values differ (B = %zu)\n", B);
                return 1;
            }
            CHECK(plonk_prover_solve_failures(p, B, rows.data()));
            memcpy(pin_in, in.data(), in.size());
            CHECK(plonk_prover_upload_inputs_async(p, (const uint8_t*)pin_in, B));
            // variables
            CHECK(plonk_prover_upload_variables(p, vars.data(), B));
            memcpy(pin_vars, vars.data(), vars.size());
            CHECK(plonk_prover_upload_variables_async(p, (const uint8_t*)pin_vars, B));
            CHECK(plonk_prover_download_variables(p, B, nullptr, 0, got.data()));
            if (memcmp(got.data(), vars.data(), vars.size())) {
                fprintf(stderr, "uploaded values differ (B = %zu)\n", B);
                return 1;
            }
            // wire columns: no variable values afterwards
            CHECK(plonk_prover_upload_witness(p, abc.data(), nullptr, B));
            if (plonk_prover_download_variables(p, B, nullptr, 0, got.data()) != PLONK_ERR_STATE) {
                fprintf(stderr, "download_variables after a column upload was not refused\n");
                return 1;
            }
            CHECK(plonk_prover_solve_failures(p, B, rows.data()));
        }
        if (pass == 0) CHECK(plonk_prover_set_inputs(p, &input, 1, &missing));  // a second plan: the staging of the first goes
    }
    CHECK(plonk_prover_destroy(p));

    plonk_prover* idle = make_prover(ctx, srs);  // never uploads: owns no staging buffer and no event
    CHECK(plonk_prover_destroy(idle));

    CHECK(plonk_host_free(ctx, pin_in));
    CHECK(plonk_host_free(ctx, pin_vars));
    CHECK(plonk_srs_free(ctx, srs));
    CHECK(plonk_ctx_destroy(ctx));
    printf("intake_lifetime ok\n");
    return 0;
}
