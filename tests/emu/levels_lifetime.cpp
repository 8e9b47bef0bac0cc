// Stand-alone sanitizer check of the witness solver's plan (csrc/witness_solve.h, csrc/prover_intake.h) on the emulated kernels:
// who owns the descriptors and the levelised form's schedule (order, level_start) across a plan, a second plan with other
// inputs, a new wiring, uploads under both forms, and a prover that is destroyed with a plan and no upload.
//   make -C tests/emu -f levels_sanitize.mk levels-sanitize      (AddressSanitizer + UBSan, its own main, nothing loaded into Python)
// The circuit: 16 rows, two chains side by side, x_{i+1} <== x_i + x_i and y_{i+1} <== y_i + y_i for i < 4: ten variables
// (x0 .. x4, y0 .. y4), eight active rows in four levels of width two.
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

static const size_t N = 16, ROWS = 8, V = 10;
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

// rows 2 i and 2 i + 1 double x_i and y_i (interleaved = true), or rows i and 4 + i do (the second wiring)
static std::vector<uint32_t> wiring(bool interleaved) {
    std::vector<uint32_t> cell(3 * N, (uint32_t)V);
    for (size_t i = 0; i < 4; i++)
        for (size_t c = 0; c < 2; c++) {
            const size_t row = interleaved ? 2 * i + c : 4 * c + i;
            cell[row] = cell[N + row] = (uint32_t)(5 * c + i);
            cell[2 * N + row] = (uint32_t)(5 * c + i + 1);
        }
    return cell;
}

static uint64_t value(size_t b, size_t var) { return (uint64_t)(3 + 5 * b + 7 * (var / 5)) << (var % 5); }

// one batch of B from the inputs x0, y0 (and x4 where with_x4: its row is then a check) under `form`: every variable is the doubled one
static void solve_and_compare(plonk_prover* p, unsigned form, size_t B, bool with_x4) {
    CHECK(plonk_prover_set_options(p, PLONK_PROVER_SOLVE_FORM(form)));
    const size_t K = with_x4 ? 3 : 2;
    std::vector<uint8_t> in(B * K * 32), want(B * V * 32), got(B * V * 32);
    for (size_t b = 0; b < B; b++) {
        put_u64(&in[(b * K + 0) * 32], value(b, 0));
        put_u64(&in[(b * K + 1) * 32], value(b, 5));
        if (with_x4) put_u64(&in[(b * K + 2) * 32], value(b, 4));
        for (size_t v = 0; v < V; v++) put_u64(&want[(b * V + v) * 32], value(b, v));
    }
    CHECK(plonk_prover_upload_inputs(p, in.data(), B));
    CHECK(plonk_prover_download_variables(p, B, nullptr, 0, got.data()));
    if (memcmp(got.data(), want.data(), want.size())) {
        fprintf(stderr, "solved values differ (form %u, B = %zu)\n", form, B);
        exit(1);
    }
    std::vector<uint32_t> rows(B, 99);
    CHECK(plonk_prover_solve_failures(p, B, rows.data()));
    for (size_t b = 0; b < B; b++) EXPECT(rows[b] == 0);
}

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
    uint32_t plan[7], missing = 0;
    EXPECT(plonk_prover_solve_plan(p, 1, plan) == PLONK_ERR_STATE);  // no wiring, no plan
    CHECK(plonk_prover_set_wiring(p, wiring(true).data(), nullptr, V));
    EXPECT(plonk_prover_solve_plan(p, 1, plan) == PLONK_ERR_STATE);
    const uint32_t two[2] = {0, 5}, three[3] = {0, 5, 4};
    CHECK(plonk_prover_set_inputs(p, two, 2, &missing));
    CHECK(plonk_prover_solve_plan(p, 1, plan));
    EXPECT(plan[0] == 8 && plan[1] == 8 && plan[2] == 4 && plan[3] == 2 && plan[4] == 64 && plan[6] == 4);
    for (unsigned form : {PLONK_PROVER_SOLVE_LEVELS, PLONK_PROVER_SOLVE_LANES, 0u})
        for (size_t B : {2, 5, 1}) solve_and_compare(p, form, B, false);
    // a second plan with other inputs: x4's row becomes a check, on the level it had
    CHECK(plonk_prover_set_inputs(p, three, 3, &missing));
    CHECK(plonk_prover_solve_plan(p, 3, plan));
    EXPECT(plan[1] == 8 && plan[2] == 4 && plan[3] == 2);
    for (unsigned form : {PLONK_PROVER_SOLVE_LANES, PLONK_PROVER_SOLVE_LEVELS})
        for (size_t B : {5, 2}) solve_and_compare(p, form, B, true);
    // a refused plan (x0 alone: y0 is read and never given) leaves the one in force
    const uint32_t one = 0;
    EXPECT(plonk_prover_set_inputs(p, &one, 1, &missing) == PLONK_ERR_ARG && missing == 5);
    solve_and_compare(p, PLONK_PROVER_SOLVE_LEVELS, 3, true);
    // a new wiring drops the plan with its schedule; the next plan is built from the new rows
    CHECK(plonk_prover_set_wiring(p, wiring(false).data(), nullptr, V));
    EXPECT(plonk_prover_solve_plan(p, 1, plan) == PLONK_ERR_STATE);
    std::vector<uint8_t> in(3 * 32, 0);
    EXPECT(plonk_prover_upload_inputs(p, in.data(), 1) == PLONK_ERR_STATE);
    CHECK(plonk_prover_set_inputs(p, two, 2, &missing));
    CHECK(plonk_prover_solve_plan(p, 1, plan));
    EXPECT(plan[1] == 8 && plan[2] == 4 && plan[3] == 2);
    for (unsigned form : {PLONK_PROVER_SOLVE_LEVELS, PLONK_PROVER_SOLVE_LANES}) solve_and_compare(p, form, 4, false);
    EXPECT(plonk_prover_set_options(p, PLONK_PROVER_SOLVE_FORM(3)) == PLONK_ERR_ARG);
    CHECK(plonk_prover_destroy(p));

    plonk_prover* planned = make_prover(ctx, srs);  // a plan and no upload: owns the schedule, no staging buffer, no event
    CHECK(plonk_prover_set_wiring(planned, wiring(true).data(), nullptr, V));
    CHECK(plonk_prover_set_inputs(planned, two, 2, &missing));
    CHECK(plonk_prover_destroy(planned));

    CHECK(plonk_srs_free(ctx, srs));
    CHECK(plonk_ctx_destroy(ctx));
    printf("levels_lifetime ok\n");
    return 0;
}
