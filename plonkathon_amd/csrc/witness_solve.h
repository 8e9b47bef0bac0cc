// witness_solve.h — the witness solver of the lock-step prover (internal, included by prover.hip): the variables of every proof
// of a batch from the circuit's input values, on the device.
//
// Reference behaviour replaced: Program.fill_variable_assignments (compiler/program.py:161-192), which solves the gate identity
// for the output wire row by row wherever QO = +-1:   c = -(QL a + QR b + QM a b + QC) / QO.
// The selectors are the prover's fixed_lag, the variable of every wire cell its cell_index: nothing else describes the circuit.
// The PLAN (solve_plan_build, once per set of inputs) replays the rows on the host with a "known" bit per variable and leaves one
// descriptor word per row, and the rows sorted into dependency levels.  Once per batch one of two KERNELS runs (solve_plan_form
// chooses): witness_solve_kernel walks the rows in program order with one lane per proof; witness_solve_levels_kernel gives a
// proof a workgroup, whose lanes take the rows of one level at a time.  Same values, same verdicts.
#pragma once
#include <algorithm>
#include <vector>

#include "prover.h"

// A row's descriptor: its kind, the sign of QO and the class of each of QL, QR, QM, QC.
#define SOLVE_SKIP 0u    // the O cell is empty or QO is not +-1 (public rows, padding): nothing to do
#define SOLVE_ASSIGN 1u  // O is not yet known: it is written
#define SOLVE_CHECK 2u   // O is already known: it is compared, a mismatch is the reference's "Failed assertion"
#define SOLVE_KIND_MASK 3u
#define SOLVE_QO_MINUS 4u  // QO = r - 1 (a negated output, "-d <== ...")
enum { SOLVE_CLS_ZERO = 0, SOLVE_CLS_ONE = 1, SOLVE_CLS_MINUS_ONE = 2, SOLVE_CLS_GENERAL = 3 };
#define SOLVE_SHIFT_QL 4
#define SOLVE_SHIFT_QR 6
#define SOLVE_SHIFT_QM 8
#define SOLVE_SHIFT_QC 10
#define SOLVE_NO_VARIABLE 0xffffffffu  // *out_missing_var of plonk_prover_set_inputs where the refusal names no variable

// sum + q x for a selector q of class `cls`: classes 0 and +-1 cost no multiplication, only "general" loads the selector (one
// address for the whole wave)
PLONK_DEV Fr solve_term(const Fr& sum, const Fr& x, unsigned cls, const Fr* sel) {
    if (cls == SOLVE_CLS_ONE) return fp_add(sum, x);
    if (cls == SOLVE_CLS_MINUS_ONE) return fp_sub(sum, x);
    if (cls == SOLVE_CLS_GENERAL) return fp_add(sum, fp_mul(x, fp_load(sel)));
    return sum;
}

// The row step of both kernels: -(QL a + QR b + QM a b + QC) / QO of row `row` with descriptor d and the L and R cells il, ir,
// from the proof's variables v.  A cell index V (empty cell) reads as zero WITHOUT a load: v + V is the next proof's slot 0, and
// past the buffer for the last proof.
PLONK_DEV Fr solve_row_value(const Fr* v, uint32_t d, uint32_t row, uint32_t il, uint32_t ir, const Fr* fixed_lag, size_t V, size_t n) {
    const Fr a = il < V ? fp_load(v + il) : fp_zero<FrParams>();
    const Fr bb = ir < V ? fp_load(v + ir) : fp_zero<FrParams>();
    const unsigned cm = (d >> SOLVE_SHIFT_QM) & 3u, cc = (d >> SOLVE_SHIFT_QC) & 3u;
    Fr sum = fp_zero<FrParams>();
    if (cm) sum = solve_term(sum, fp_mul(a, bb), cm, fixed_lag + FX_QM * n + row);
    sum = solve_term(sum, a, (d >> SOLVE_SHIFT_QL) & 3u, fixed_lag + FX_QL * n + row);
    sum = solve_term(sum, bb, (d >> SOLVE_SHIFT_QR) & 3u, fixed_lag + FX_QR * n + row);
    if (cc == SOLVE_CLS_GENERAL) sum = fp_add(sum, fp_load(fixed_lag + FX_QC * n + row));
    else if (cc) sum = solve_term(sum, fp_one<FrParams>(), cc, nullptr);
    return (d & SOLVE_QO_MINUS) ? sum : fp_neg(sum);  // -sum / QO
}

// One lane per proof, in place on vars [B][V] (Montgomery).  Every lane walks the rows 0 .. n_rows - 1 in program order, so
// every branch on a descriptor or a cell index is wave-uniform.  An assign or check row's O cell is never empty
// (solve_plan_build), and the plan guarantees that a slot is written (by the seed or an earlier row) before it is read.
// bad[b] = 0, or 1 + the first row whose check failed.
__global__ void __launch_bounds__(64) witness_solve_kernel(Fr* __restrict__ vars, const uint32_t* __restrict__ desc,
                                                           const uint32_t* __restrict__ cell, const Fr* __restrict__ fixed_lag, size_t V, size_t n,
                                                           uint32_t n_rows, size_t B, uint32_t* __restrict__ bad) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    Fr* v = vars + b * V;
    uint32_t first_bad = 0;
    for (uint32_t row = 0; row < n_rows; row++) {
        const uint32_t d = desc[row], kind = d & SOLVE_KIND_MASK;
        if (kind == SOLVE_SKIP) continue;
        const uint32_t il = cell[row], ir = cell[n + row], io = cell[2 * n + row];
        const Fr out = solve_row_value(v, d, row, il, ir, fixed_lag, V, n);
        if (kind == SOLVE_ASSIGN) fp_store(v + io, out);
        else if (!first_bad && !fp_eq(fp_load(v + io), out)) first_bad = row + 1;
    }
    bad[b] = first_bad;
}

// The levelised form: one workgroup per proof (grid B, block T = 64 or 256: solve_plan_build), in place on the same vars.  The
// rows of dependency level l are order[level_start[l] .. level_start[l + 1]): they read only variables that the seed or a row of
// an earlier level wrote, so the lanes take them T at a time in any order, and a workgroup barrier closes the level.  The values
// travel between levels through `vars` in global memory, ordered by the barrier's workgroup-scope fence: `vars` is not
// __restrict__ here and nothing read from it lives across a barrier.  Every lane runs every level and every barrier (no early
// return; the inner loop's trip count alone differs between lanes).  A failed check leaves its row in one LDS word by atomicMin:
// bad[b] = 0, or 1 + the SMALLEST failing row, which is the first one the walk in program order meets.
#define SOLVE_LEVELS_MAX_THREADS 256
__global__ void __launch_bounds__(SOLVE_LEVELS_MAX_THREADS) witness_solve_levels_kernel(Fr* vars, const uint32_t* __restrict__ desc,
                                                                                       const uint32_t* __restrict__ order,
                                                                                       const uint32_t* __restrict__ level_start,
                                                                                       const uint32_t* __restrict__ cell,
                                                                                       const Fr* __restrict__ fixed_lag, size_t V, size_t n,
                                                                                       uint32_t levels, uint32_t* __restrict__ bad) {
    __shared__ uint32_t first_bad;
    Fr* v = vars + (size_t)blockIdx.x * V;
    if (threadIdx.x == 0) first_bad = 0xffffffffu;
    __syncthreads();
    uint32_t begin = level_start[0];
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t end = level_start[l + 1];
        for (uint32_t k = begin + threadIdx.x; k < end; k += blockDim.x) {
            const uint32_t row = order[k], d = desc[row], il = cell[row], ir = cell[n + row], io = cell[2 * n + row];
            const Fr out = solve_row_value(v, d, row, il, ir, fixed_lag, V, n);
            if ((d & SOLVE_KIND_MASK) == SOLVE_ASSIGN) fp_store(v + io, out);
            else if (!fp_eq(fp_load(v + io), out)) atomicMin(&first_bad, row);
        }
        __syncthreads();
        begin = end;
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = first_bad == 0xffffffffu ? 0u : first_bad + 1;
}

// The inputs of a batch, in [B][K] canonical little-endian: range-checked and converted as fr_to_mont_checked_kernel does (*bad =
// the flat index of the first value that is not below r, so the owning proof is *bad / K), and written to their variables' slots.
__global__ void witness_seed_kernel(const Fr* in, const uint32_t* input_index, size_t K, size_t V, size_t B, Fr* vars, unsigned long long* bad,
                                    uint32_t* solve_bad) {
    const size_t total = B * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / K, k = i - b * K;
        const Fr a = fp_load(in + i);
        uint32_t br = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) (void)fp_sbb(a.v[q], FrParams::mod(q), br);  // a - r borrows  <=>  a < r
        if (!br) atomicMin(bad, (unsigned long long)i);
        fp_store(vars + b * V + input_index[k], fp_to_mont(a));
        if (k == 0) solve_bad[b] = 0;
    }
}

// plonk_prover_download_variables: out[b][j] = the canonical value of variable index[j] (index == null: j) of proof b
__global__ void variable_gather_kernel(const Fr* vars, const uint32_t* index, size_t V, size_t k, size_t B, Fr* out) {
    const size_t total = B * k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / k, j = i - b * k;
        fp_store(out + i, fp_from_mont(fp_load(vars + b * V + (index ? index[j] : (uint32_t)j))));
    }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// class of a canonical little-endian selector value: 0, 1, r - 1 or anything else
static inline unsigned solve_class(const uint8_t* le32) {
    uint32_t v[8], rest = 0;
    memcpy(v, le32, 32);
    for (int k = 1; k < 8; k++) rest |= v[k];
    if (!rest && v[0] == 0) return SOLVE_CLS_ZERO;
    if (!rest && v[0] == 1) return SOLVE_CLS_ONE;
    bool minus_one = v[0] == FrParams::mod(0) - 1;  // r is odd: r - 1 differs from r in limb 0 only
    for (int k = 1; k < 8; k++) minus_one = minus_one && v[k] == FrParams::mod(k);
    return minus_one ? SOLVE_CLS_MINUS_ONE : SOLVE_CLS_GENERAL;
}

// What solve_plan_build leaves: the descriptors that both kernels read, and the levelised form's schedule.
struct SolvePlan {
    std::vector<uint32_t> desc;         // [rows walked] one descriptor per row, up to the last row that is not skipped
    std::vector<uint32_t> order;        // [active] the rows that are not skipped, by level, then by descriptor word, then by row
    std::vector<uint32_t> level_start;  // [levels + 1] level l is order[level_start[l] .. level_start[l + 1])
    uint32_t widest;                    // rows of the widest level
    uint32_t threads;                   // T, the levelised kernel's block: one wave where no level is wider than one
    uint32_t steps;                     // sum over the levels of ceil(width / T): what the levelised form walks instead of `active` rows
};

// Replays the rows in program order (compiler/program.py:161-192) with a "known" bit per variable, the inputs known from the
// start.  gates = the columns QM, QL, QR, QO, QC (FX_* order) as [5][n] canonical LE, cell = cell_index [3][n].  Leaves one
// descriptor per row up to the last row that is not skipped, and every such row's dependency LEVEL: 1 + the largest level among
// the rows that assigned its L and R variables — and O, for a check — with the inputs at level 0.  A variable is assigned exactly
// once (a later row with the same output is a check), so read-after-write is the only hazard and rows of one level are independent.
// PLONK_ERR_ARG with *missing = the variable where a row reads one
// that is not yet known (the reference's KeyError at out[in_L]) or where one is still unknown after the last row (the reference
// fails later, at witness[wire]); with *missing = SOLVE_NO_VARIABLE for an input index out of range or given twice.
static int solve_plan_build(const uint8_t* gates, const uint32_t* cell, size_t n, size_t V, const uint32_t* input_index, size_t n_inputs,
                            SolvePlan& plan, uint32_t* missing) {
    *missing = SOLVE_NO_VARIABLE;
    std::vector<uint8_t> known(V, 0);
    for (size_t k = 0; k < n_inputs; k++) {
        PLONK_REQUIRE(input_index[k] < V, PLONK_ERR_ARG, "input %zu names variable %u of %zu", k, input_index[k], V);
        PLONK_REQUIRE(!known[input_index[k]], PLONK_ERR_ARG, "input %zu names variable %u a second time", k, input_index[k]);
        known[input_index[k]] = 1;
    }
    std::vector<uint32_t>& desc = plan.desc;
    desc.assign(n, SOLVE_SKIP);
    std::vector<uint32_t> var_level(V, 0), row_level(n, 0);  // the level of the row that assigned a variable; of a row (0: skipped)
    uint32_t levels = 0;
    size_t n_rows = 0;
    for (size_t row = 0; row < n; row++) {
        const uint32_t il = cell[row], ir = cell[n + row], io = cell[2 * n + row];
        const unsigned qo = solve_class(gates + 32 * (FX_QO * n + row));
        if (io >= V || (qo != SOLVE_CLS_ONE && qo != SOLVE_CLS_MINUS_ONE)) continue;
        for (const uint32_t in : {il, ir})
            if (in < V && !known[in]) {
                *missing = in;
                PLONK_REQUIRE(false, PLONK_ERR_ARG, "row %zu reads variable %u, which is neither an input nor assigned by an earlier row", row, in);
            }
        uint32_t d = known[io] ? SOLVE_CHECK : SOLVE_ASSIGN;
        if (qo == SOLVE_CLS_MINUS_ONE) d |= SOLVE_QO_MINUS;
        d |= solve_class(gates + 32 * (FX_QL * n + row)) << SOLVE_SHIFT_QL;
        d |= solve_class(gates + 32 * (FX_QR * n + row)) << SOLVE_SHIFT_QR;
        d |= solve_class(gates + 32 * (FX_QM * n + row)) << SOLVE_SHIFT_QM;
        d |= solve_class(gates + 32 * (FX_QC * n + row)) << SOLVE_SHIFT_QC;
        desc[row] = d;
        uint32_t level = known[io] ? var_level[io] : 0;
        for (const uint32_t in : {il, ir})
            if (in < V && var_level[in] > level) level = var_level[in];
        row_level[row] = ++level;
        if (!known[io]) var_level[io] = level;
        if (level > levels) levels = level;
        known[io] = 1;
        n_rows = row + 1;
    }
    for (size_t v = 0; v < V; v++)
        if (!known[v]) {
            *missing = (uint32_t)v;
            PLONK_REQUIRE(false, PLONK_ERR_ARG, "variable %zu is neither an input nor assigned by any row", v);
        }
    desc.resize(n_rows);  // rows beyond the last one that is not skipped are not walked
    // the schedule: a counting sort by level, then each level by descriptor word (a wave then mostly sees one selector class), then by row
    plan.level_start.assign(levels + 1, 0);
    for (size_t row = 0; row < n_rows; row++)
        if (row_level[row]) plan.level_start[row_level[row]]++;
    plan.widest = 0;
    for (uint32_t l = 1; l <= levels; l++) {
        plan.widest = std::max(plan.widest, plan.level_start[l]);
        plan.level_start[l] += plan.level_start[l - 1];
    }
    plan.order.assign(plan.level_start[levels], 0);
    std::vector<uint32_t> fill(plan.level_start.begin(), plan.level_start.end() - 1);
    for (size_t row = 0; row < n_rows; row++)
        if (row_level[row]) plan.order[fill[row_level[row] - 1]++] = (uint32_t)row;
    plan.threads = plan.widest <= 64 ? 64 : SOLVE_LEVELS_MAX_THREADS;
    plan.steps = 0;
    for (uint32_t l = 0; l < levels; l++) {
        std::sort(plan.order.begin() + plan.level_start[l], plan.order.begin() + plan.level_start[l + 1],
                  [&desc](uint32_t a, uint32_t b) { return desc[a] != desc[b] ? desc[a] < desc[b] : a < b; });
        plan.steps += (plan.level_start[l + 1] - plan.level_start[l] + plan.threads - 1) / plan.threads;
    }
    return PLONK_OK;
}
