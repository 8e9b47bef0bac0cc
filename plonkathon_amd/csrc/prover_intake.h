// prover_intake.h — how a batch gets into the lock-step prover (internal, included by prover.hip): everything between "bytes from
// the caller" and "wit_lag, pub, the PI column and resident_b are in place".  The wiring and the solver's plan, the three kinds
// of upload (wire columns, per-variable values, input values), and what reads the resident variables back.
// Blinding (prover_blind.h) is not intake: the blinders belong to a RUN, not to a slot — plonk_prover_run draws or copies them for
// the batch it proves — so staging and advance are the same for a blinded prover.
//
// Stream order of an upload.  C = the context's compute stream, H = its copy stream; "sync" and "async" are the two entry points
// of a kind.  Growing a buffer waits for C first (dev_grow).
//   wire columns (sync only)   C: memset bad_input (if allocated) · plonk_fr_upload wit_lag [H2D, checked conversion, wait]
//                                 · plonk_fr_upload pub [the same] · PI column · wait
//   variables, sync            C: memset bad_input · plonk_fr_upload vars [H2D, checked conversion, wait] · GATHER · wait
//   variables, async           H: wait vars.read (if pending) · H2D vars · record ev_copied
//                              C: wait ev_copied · checked conversion in place [memset bad_input, kernel] · GATHER
//   inputs, sync               C: H2D inputs · SOLVE · GATHER · D2H bad_input · wait
//   inputs, async              H: wait inputs.read (if pending) · H2D inputs · record ev_copied
//                              C: wait ev_copied · SOLVE · GATHER
//   SOLVE  = memset bad_input · witness_seed_kernel · record inputs.read · [prof] witness_solve_kernel [prof]
//            (the levelised form, solve_form_of: witness_solve_levels_kernel in that kernel's place)
//   GATHER = witness_scatter_kernel · public_gather_kernel (if n_public) · PI column · record vars.read
//   PI column = memset (n_public == 0) | pi_fill_kernel (dense PI) | nothing (sparse PI: round 1 builds it from pub)
// A prover over a table of circuits (plonk_prover_create_multi): every upload above first takes the labels plonk_prover_set_labels left
// for it — C: H2D labels (behind an event: the host copy is not rewritten under it) — and the gathers index the wiring tables with them.
// The solver writes `vars` in place: on C it is behind the previous batch's gathers, the only readers, so only the staging buffer
// that H writes needs its `read` event.  An async path's canonical-range verdict comes back as PROVER_ST_BAD_INPUT of the download.
//
// The second slot (StagedSlot, prover.h).  A prover that stages owns a second wit_lag, pub, vars, inputs, bad_input and solver.bad.  The
// uploads above fill the RESIDENT set on C; a stage fills the STAGED set on H alone, where copy, seed, solve and gathers are in order
// without an event between them, and touches nothing of the resident batch:
//   stage inputs               H: wait released (if pending) · H2D inputs · SOLVE (no record, no prof) · GATHER (no record) · record ready
//   stage variables            H: wait released (if pending) · H2D vars · checked conversion in place [memset bad_input, kernel]
//                                 · GATHER (no record) · record ready
//   advance                    C: wait ready · [host: the two sets change places by pointer] · record released
// `released` stands behind everything C was given while the buffers that are now the staged set were resident — the rounds that read
// wit_lag and pub, the download that reads the two verdicts — so it is all the next stage waits for.  Growing a staged buffer waits on
// the host for H and for `released`, never for C; growing the rounds' buffers for a staged batch larger than any before is left to
// advance, which gives up the resident batch anyway.
#pragma once
#include <string.h>

#include <utility>

#include "witness_solve.h"  // prover.h; the plan, the solver's kernels

static int ensure_batch(plonk_prover* p, size_t B);   // prover.hip: the per-batch buffers of B proofs, the resident set's among them
static int ensure_rounds(plonk_prover* p, size_t B);  // prover.hip: the same without the resident set's (advance brings its own)
#define STAGED_N_VECTORS 4  // n-vectors per proof of a set (wit_lag); BATCH_N_VECTORS counts them for the resident one

// witness upload helper: PI[b][i] = -public[b][i] for i < n_public, 0 otherwise (prover.py:57-62)
__global__ void pi_fill_kernel(const Fr* pub, size_t n_public, size_t n, size_t B, Fr* pi) {
    const size_t total = B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / n, i = gI - b * n;
        Fr v = fp_zero<FrParams>();
        if (i < n_public) v = fp_neg(fp_load(pub + b * n_public + i));
        fp_store(pi + gI, v);
    }
}

// prover.py:94-103 on the device: A[i], B[i], C[i] = witness[wires[i].L / R / O], witness[None] = 0, zero padded to n.
// vars = [B][V] variable values; cell[K][3][n] = variable index of each wire cell (V: empty); out = wit_lag [3][B][n].  Proof b is
// wired as circuit cid[b] (cid == null: circuit 0), its variables numbered in that circuit's order.
__global__ void witness_scatter_kernel(const Fr* vars, const uint32_t* cell, const uint32_t* cid, size_t V, size_t n, size_t B, Fr* out) {
    const size_t total = 3 * B * n;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t j = gI / (B * n), r = gI - j * B * n, b = r / n, i = r - b * n;
        const uint32_t idx = cell[(cid ? (size_t)cid[b] * 3 * n : 0) + j * n + i];
        fp_store(out + gI, idx < V ? fp_load(vars + b * V + idx) : fp_zero<FrParams>());
    }
}
// pub_index[K][l]; an entry V pads the row of a circuit with fewer than l public inputs: the value is 0
__global__ void public_gather_kernel(const Fr* vars, const uint32_t* pub_index, const uint32_t* cid, size_t V, size_t l, size_t B, Fr* pub) {
    const size_t total = B * l;
    for (size_t gI = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gI < total; gI += (size_t)gridDim.x * blockDim.x) {
        const size_t b = gI / l, k = gI - b * l;
        const uint32_t idx = pub_index[(cid ? (size_t)cid[b] * l : 0) + k];
        fp_store(pub + gI, idx < V ? fp_load(vars + b * V + idx) : fp_zero<FrParams>());
    }
}

// the wiring's, the solver's and the staging's share of plonk_prover_create and plonk_prover_destroy
static int intake_init(plonk_prover* p, const uint8_t* selectors_le32) {
    p->solver.gates_host = (uint8_t*)malloc(5 * p->circuit.n * 32);  // QM .. QC as given: what plonk_prover_set_inputs classifies
    PLONK_REQUIRE(p->solver.gates_host, PLONK_ERR_NOMEM, "out of host memory");
    memcpy(p->solver.gates_host, selectors_le32, 5 * p->circuit.n * 32);
    return PLONK_OK;
}
static void intake_destroy(plonk_prover* p) {
    dev_free_all({(void**)&p->intake.vars.buf, (void**)&p->intake.inputs.buf, (void**)&p->intake.bad_input, (void**)&p->wiring.cell_index,
                  (void**)&p->wiring.pub_index, (void**)&p->solver.desc, (void**)&p->solver.order, (void**)&p->solver.level_start,
                  (void**)&p->solver.input_index, (void**)&p->solver.bad, (void**)&p->labels.dev});
    free(p->labels.pending);
    free(p->labels.host);
    if (p->labels.copied) hipEventDestroy(p->labels.copied);
    StagedSlot& sl = p->staged;  // a batch still staged goes with its buffers (plonk_prover_destroy has waited for both streams)
    dev_free_all({(void**)&sl.wit_lag, (void**)&sl.pub, (void**)&sl.vars.buf, (void**)&sl.inputs.buf, (void**)&sl.bad_input, (void**)&sl.solve_bad});
    for (hipEvent_t ev : {p->intake.vars.read, p->intake.inputs.read, p->intake.ev_copied, sl.vars.read, sl.inputs.read, sl.ready, sl.released})
        if (ev) hipEventDestroy(ev);  // each exists only if an upload or a stage created it
    free(p->solver.gates_host);
    free(p->wiring.cell_host);
}

// The caller's bytes into a staging buffer.  async: on the copy stream, behind the previous batch's last read of the buffer; the
// compute stream goes on behind the copy.  Otherwise on the compute stream.
static int staging_copy(plonk_prover* p, Staging* st, const uint8_t* src, size_t bytes, bool async) {
    plonk_ctx* ctx = p->circuit.ctx;
    if (!async) {
        PLONK_CHECK_HIP(hipMemcpyAsync(st->buf, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return PLONK_OK;
    }
    PLONK_TRY(ctx_copy_stream(ctx));
    if (st->read_pending) PLONK_CHECK_HIP(hipStreamWaitEvent(ctx->copy_stream, st->read, 0));
    PLONK_CHECK_HIP(hipMemcpyAsync(st->buf, src, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    PLONK_CHECK_HIP(hipEventRecord(p->intake.ev_copied, ctx->copy_stream));
    PLONK_CHECK_HIP(hipStreamWaitEvent(ctx->stream, p->intake.ev_copied, 0));
    return PLONK_OK;
}

// What a prover over a table of K > 1 circuits does not do yet: the solver's plan and the staged slot are per circuit.
#define PLONK_REQUIRE_ONE_CIRCUIT(p, what) \
    PLONK_REQUIRE((p)->circuit.n_circuits == 1, PLONK_ERR_STATE, what ": not on a prover over a table of %u circuits", (p)->circuit.n_circuits)

// The labels an upload of B proofs will take (plonk_prover_set_labels).  labels_check changes nothing; labels_commit makes them the
// resident batch's: the host copy, and for a table of more than one circuit the device array behind everything on stream s.
static int labels_check(const plonk_prover* p, size_t B) {
    const plonk_prover::Labels& lb = p->labels;
    PLONK_REQUIRE(!lb.pending_batch || lb.pending_batch == B, PLONK_ERR_STATE, "upload: batch %zu, but the labels were set for a batch of %zu", B,
                  lb.pending_batch);
    PLONK_REQUIRE(lb.pending_batch || p->circuit.n_circuits == 1, PLONK_ERR_STATE,
                  "upload: a table of %u circuits, and plonk_prover_set_labels has not named the circuit of each of the %zu proofs", p->circuit.n_circuits, B);
    return PLONK_OK;
}
static int labels_commit(plonk_prover* p, size_t B, hipStream_t s, bool take_pending = true) {
    plonk_prover::Labels& lb = p->labels;
    if (lb.copy_pending) PLONK_CHECK_HIP(hipEventSynchronize(lb.copied));  // the previous batch's copy still reads `host`
    lb.copy_pending = false;
    if (B > lb.host_cap) {
        free(lb.host);
        lb.host_cap = 0;
        lb.host = (uint32_t*)malloc(B * sizeof(uint32_t));
        PLONK_REQUIRE(lb.host, PLONK_ERR_NOMEM, "out of host memory");
        lb.host_cap = B;
    }
    if (take_pending && lb.pending_batch) {  // (labels_check: they are of B proofs)
        memcpy(lb.host, lb.pending, B * sizeof(uint32_t));
        lb.pending_batch = 0;
    } else {
        memset(lb.host, 0, B * sizeof(uint32_t));
    }
    if (p->circuit.n_circuits == 1) return PLONK_OK;  // every kernel is given a null array
    PLONK_TRY(dev_grow(s, &lb.cap, B, {{(void**)&lb.dev, B * sizeof(uint32_t)}}));
    if (!lb.copied) PLONK_CHECK_HIP(hipEventCreate(&lb.copied));
    PLONK_CHECK_HIP(hipMemcpyAsync(lb.dev, lb.host, B * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    PLONK_CHECK_HIP(hipEventRecord(lb.copied, s));
    lb.copy_pending = true;
    return PLONK_OK;
}

// the PI column of B witnesses, wit_lag[3]: -public inputs, then zeros (the sparse form is built from `pub` in round 1)
static int fill_pi_column(plonk_prover* p, Fr* wit_lag, const Fr* pub, size_t B, hipStream_t s) {
    const size_t n = p->circuit.n, l = p->circuit.n_public;
    Fr* pi = wit_lag + 3 * B * n;
    if (!l) PLONK_CHECK_HIP(hipMemsetAsync(pi, 0, B * n * sizeof(Fr), s));
    else if (!p->circuit.sparse_pi) PLONK_LAUNCH(pi_fill_kernel, grid1(B * n), dim3(256), 0, s, pub, l, n, B, pi);
    PLONK_CHECK_HIP(hipGetLastError());
    return PLONK_OK;
}

// the form of the solve of B proofs: PLONK_PROVER_SOLVE_FORM where it was set, the automatic rule otherwise
static unsigned solve_form_of(const plonk_prover* p, size_t B) {
    const plonk_prover::Solver& sv = p->solver;
    return p->solve_forced ? p->solve_forced : solve_plan_form(device_cus(p->circuit.ctx->device), sv.active, sv.steps, sv.threads, B);
}

// One batch's own buffers, wherever they live: the resident set or the staged one.
struct BatchSet { Fr *wit_lag, *pub, *vars, *inputs; unsigned long long* bad_input; uint32_t* solve_bad; };
static BatchSet resident_set(plonk_prover* p) {
    return {p->rounds.wit_lag, p->intake.pub, p->intake.vars.buf, p->intake.inputs.buf, p->intake.bad_input, p->solver.bad};
}
static BatchSet staged_set(plonk_prover* p) {
    const StagedSlot& sl = p->staged;
    return {sl.wit_lag, sl.pub, sl.vars.buf, sl.inputs.buf, sl.bad_input, sl.solve_bad};
}

// The three steps that SOLVE and GATHER (the head of this file) are made of, for B proofs of the set `bs` on stream s.
static void enqueue_seed(plonk_prover* p, const BatchSet& bs, size_t B, hipStream_t s) {
    const size_t V = p->wiring.n_vars, K = p->solver.n_inputs;
    PLONK_LAUNCH(witness_seed_kernel, grid1(B * K), dim3(256), 0, s, (const Fr*)bs.inputs, (const uint32_t*)p->solver.input_index, K, V, B, bs.vars,
                 bs.bad_input, bs.solve_bad);
}
static void enqueue_solve(plonk_prover* p, const BatchSet& bs, size_t B, hipStream_t s) {
    const size_t n = p->circuit.n, V = p->wiring.n_vars;
    if (solve_form_of(p, B) == PLONK_PROVER_SOLVE_LEVELS)
        PLONK_LAUNCH(witness_solve_levels_kernel, dim3((unsigned)B), dim3(p->solver.threads), 0, s, bs.vars, (const uint32_t*)p->solver.desc,
                     (const uint32_t*)p->solver.order, (const uint32_t*)p->solver.level_start, (const uint32_t*)p->wiring.cell_index,
                     (const Fr*)p->circuit.fixed_lag, V, n, p->solver.levels, bs.solve_bad);
    else
        PLONK_LAUNCH(witness_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, bs.vars, (const uint32_t*)p->solver.desc,
                     (const uint32_t*)p->wiring.cell_index, (const Fr*)p->circuit.fixed_lag, V, n, p->solver.rows, B, bs.solve_bad);
}
static int enqueue_gather(plonk_prover* p, const BatchSet& bs, size_t B, hipStream_t s) {
    const size_t n = p->circuit.n, l = p->circuit.n_public, V = p->wiring.n_vars;
    const uint32_t* cid = p->circuit.n_circuits > 1 ? p->labels.dev : nullptr;  // (a staged set is a one-circuit prover's)
    PLONK_LAUNCH(witness_scatter_kernel, grid1(3 * B * n), dim3(256), 0, s, (const Fr*)bs.vars, (const uint32_t*)p->wiring.cell_index, cid, V, n, B, bs.wit_lag);
    if (l) PLONK_LAUNCH(public_gather_kernel, grid1(B * l), dim3(256), 0, s, (const Fr*)bs.vars, (const uint32_t*)p->wiring.pub_index, cid, V, l, B, bs.pub);
    return fill_pi_column(p, bs.wit_lag, bs.pub, B, s);
}

// Per-variable values of a batch, uploaded ([B][n_vars] canonical LE, n_vars * 32 bytes per proof instead of 3 * n * 32) or, from_inputs,
// solved from [B][n_inputs] input values; the wire columns and the public inputs are gathered from them on the device (prover.py:94-103,
// 57-62).  async (order: the head of this file): nothing waits on the host, the copy overlaps whatever the compute stream is running; the
// caller keeps src_le32 alive, in pinned memory (plonk_host_alloc) for a copy that really is asynchronous, until the batch is downloaded.
static int prover_upload(plonk_prover* p, const uint8_t* src_le32, size_t B, bool from_inputs, bool async) {
    // begin: the checks, every buffer and event the batch needs, and no batch resident (a failed upload leaves none to run)
    PLONK_REQUIRE(p && src_le32 && B, PLONK_ERR_ARG, "bad argument");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    PLONK_REQUIRE(p->wiring.n_vars, PLONK_ERR_STATE, "plonk_prover_set_wiring has not been called");
    if (from_inputs) PLONK_REQUIRE_ONE_CIRCUIT(p, "upload_inputs");
    PLONK_REQUIRE(p->solver.n_inputs || !from_inputs, PLONK_ERR_STATE, "plonk_prover_set_inputs has not been called");
    PLONK_TRY(labels_check(p, B));
    PLONK_TRY(ensure_batch(p, B));
    plonk_prover::Intake& in = p->intake;
    hipStream_t s = ctx->stream;
    const size_t V = p->wiring.n_vars, K = p->solver.n_inputs;
    PLONK_TRY(dev_grow(s, &in.vars.cap, B * V, {{(void**)&in.vars.buf, B * V * sizeof(Fr)}}));
    if (from_inputs) PLONK_TRY(dev_grow(s, &in.inputs.cap, B, {{(void**)&in.inputs.buf, B * K * sizeof(Fr)}, {(void**)&p->solver.bad, B * sizeof(uint32_t)}}));
    if (!in.bad_input) PLONK_TRY(dev_alloc((void**)&in.bad_input, sizeof(unsigned long long)));
    if (!in.ev_copied) PLONK_CHECK_HIP(hipEventCreate(&in.ev_copied));
    if (!in.vars.read) PLONK_CHECK_HIP(hipEventCreate(&in.vars.read));
    if (from_inputs && !in.inputs.read) PLONK_CHECK_HIP(hipEventCreate(&in.inputs.read));
    in.resident_b = 0;
    in.vars_valid = p->solver.valid = false;
    in.bad_stride = from_inputs ? K : V;
    PLONK_TRY(labels_commit(p, B, s));
    // convert: `vars` of the batch in Montgomery form, and the verdict on the uploaded values in *bad_input
    if (from_inputs) {
        PLONK_TRY(staging_copy(p, &in.inputs, src_le32, B * K * sizeof(Fr), async));
        PLONK_CHECK_HIP(hipMemsetAsync(in.bad_input, 0xff, sizeof(unsigned long long), s));
        enqueue_seed(p, resident_set(p), B, s);
        PLONK_CHECK_HIP(hipEventRecord(in.inputs.read, s));
        in.inputs.read_pending = true;
        PLONK_TRY(prof_begin(ctx, "witness_solve", 32.0 * (double)V * (double)B));
        enqueue_solve(p, resident_set(p), B, s);
        PLONK_TRY(prof_end(ctx));
    } else if (async) {
        PLONK_TRY(staging_copy(p, &in.vars, src_le32, B * V * sizeof(Fr), true));
        PLONK_TRY(k_fr_to_mont_checked(ctx, in.vars.buf, B * V, in.bad_input));
    } else {
        PLONK_CHECK_HIP(hipMemsetAsync(in.bad_input, 0xff, sizeof(unsigned long long), s));
        PLONK_TRY(plonk_fr_upload(ctx, in.vars.buf, src_le32, B * V));  // waits, and reports a non-canonical value as PLONK_ERR_ARG
    }
    // finish: the wire columns, the public inputs and the PI column from `vars` (vars.read marks its last read); sync: the host waits,
    // and inputs that were only enqueued for their check get their verdict read back
    PLONK_TRY(enqueue_gather(p, resident_set(p), B, s));
    PLONK_CHECK_HIP(hipEventRecord(in.vars.read, s));
    in.vars.read_pending = true;
    unsigned long long first_bad = ~0ull;
    if (!async && from_inputs) PLONK_CHECK_HIP(hipMemcpyAsync(&first_bad, in.bad_input, sizeof first_bad, hipMemcpyDeviceToHost, s));
    if (!async) PLONK_CHECK_HIP(hipStreamSynchronize(s));
    PLONK_REQUIRE(first_bad == ~0ull, PLONK_ERR_ARG, "input %llu of proof %llu is not a canonical Fr value (>= r)", first_bad % K, first_bad / K);
    in.resident_b = B;
    in.vars_valid = true;
    p->solver.valid = from_inputs;
    return PLONK_OK;
}

// The staged set's buffers for B proofs.  One that is short is freed and allocated anew, after a host wait for H (the previous stage
// into it) and for `released` (the last reader on C of what is now the staged set) — never for C itself.
static int staged_grow(plonk_prover* p, size_t B, bool from_inputs) {
    StagedSlot& sl = p->staged;
    hipStream_t h = p->circuit.ctx->copy_stream;
    const size_t n = p->circuit.n, l = p->circuit.n_public, V = p->wiring.n_vars, K = p->solver.n_inputs;
    if (B > sl.cap_b || B * V > sl.vars.cap || (from_inputs && B > sl.inputs.cap)) {
        PLONK_CHECK_HIP(hipStreamSynchronize(h));
        if (sl.released_pending) PLONK_CHECK_HIP(hipEventSynchronize(sl.released));
        sl.released_pending = false;
    }
    int rc = dev_grow(h, &sl.cap_b, B, {{(void**)&sl.wit_lag, 4 * B * n * sizeof(Fr)}, {(void**)&sl.pub, (B * l + 1) * sizeof(Fr)}});
    if (rc == PLONK_OK) rc = dev_grow(h, &sl.vars.cap, B * V, {{(void**)&sl.vars.buf, B * V * sizeof(Fr)}});
    if (rc == PLONK_OK && from_inputs)
        rc = dev_grow(h, &sl.inputs.cap, B, {{(void**)&sl.inputs.buf, B * K * sizeof(Fr)}, {(void**)&sl.solve_bad, B * sizeof(uint32_t)}});
    if (rc == PLONK_ERR_NOMEM)
        plonk_set_error("staging a batch of %zu proofs of group_order %zu needs %zu bytes of device memory beside the resident batch's", B, n,
                        B * (STAGED_N_VECTORS * n + V) * sizeof(Fr));
    return rc;
}

// A batch into the staged set while the resident one proves (order: the head of this file): from [B][n_inputs] input values, solved, or
// from [B][n_vars] values, converted and range-checked; wire columns, public inputs and the PI column gathered.  Everything on H, nothing
// waits on the host unless a buffer has to grow, nothing of the resident batch is read or written.
static int prover_stage(plonk_prover* p, const uint8_t* src_le32, size_t B, bool from_inputs) {
    PLONK_REQUIRE(p && src_le32 && B, PLONK_ERR_ARG, "bad argument");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    StagedSlot& sl = p->staged;
    PLONK_REQUIRE_ONE_CIRCUIT(p, "stage");
    PLONK_REQUIRE(p->wiring.n_vars, PLONK_ERR_STATE, "plonk_prover_set_wiring has not been called");
    PLONK_REQUIRE(p->solver.n_inputs || !from_inputs, PLONK_ERR_STATE, "plonk_prover_set_inputs has not been called");
    PLONK_REQUIRE(!sl.batch, PLONK_ERR_STATE, "stage: a batch of %zu is already staged (plonk_prover_advance takes it)", sl.batch);
    PLONK_TRY(ctx_copy_stream(ctx));
    hipStream_t h = ctx->copy_stream;
    PLONK_TRY(staged_grow(p, B, from_inputs));
    if (!sl.bad_input) PLONK_TRY(dev_alloc((void**)&sl.bad_input, sizeof(unsigned long long)));
    if (!sl.ready) PLONK_CHECK_HIP(hipEventCreate(&sl.ready));
    if (!sl.released) PLONK_CHECK_HIP(hipEventCreate(&sl.released));
    const size_t V = p->wiring.n_vars, K = p->solver.n_inputs;
    if (sl.released_pending) PLONK_CHECK_HIP(hipStreamWaitEvent(h, sl.released, 0));
    sl.released_pending = false;  // H is in order: what it waited for once, every later stage is behind
    const BatchSet bs = staged_set(p);
    if (from_inputs) {
        PLONK_CHECK_HIP(hipMemcpyAsync(bs.inputs, src_le32, B * K * sizeof(Fr), hipMemcpyHostToDevice, h));
        PLONK_CHECK_HIP(hipMemsetAsync(bs.bad_input, 0xff, sizeof(unsigned long long), h));
        enqueue_seed(p, bs, B, h);
        enqueue_solve(p, bs, B, h);
    } else {
        PLONK_CHECK_HIP(hipMemcpyAsync(bs.vars, src_le32, B * V * sizeof(Fr), hipMemcpyHostToDevice, h));
        PLONK_TRY(k_fr_to_mont_checked_on(h, bs.vars, B * V, bs.bad_input));
    }
    PLONK_TRY(enqueue_gather(p, bs, B, h));
    PLONK_CHECK_HIP(hipEventRecord(sl.ready, h));
    sl.bad_stride = from_inputs ? K : V;
    sl.solved = from_inputs;
    sl.batch = B;
    return PLONK_OK;
}

extern "C" {

int plonk_prover_stage_inputs(plonk_prover* p, const uint8_t* inputs_le32, size_t B) { return prover_stage(p, inputs_le32, B, true); }
int plonk_prover_stage_variables(plonk_prover* p, const uint8_t* vars_le32, size_t B) { return prover_stage(p, vars_le32, B, false); }

// the batch that is staged, 0: none
int plonk_prover_staged(const plonk_prover* p, size_t* out_batch) {
    PLONK_REQUIRE(p && out_batch, PLONK_ERR_ARG, "bad argument");
    *out_batch = p->staged.batch;
    return PLONK_OK;
}

// The staged batch becomes the resident one: C waits for the stage, the two sets change places by pointer, and what C has been given
// so far — the outgoing batch's rounds and download, if the caller asked for them — is what the next stage will wait for.
int plonk_prover_advance(plonk_prover* p, size_t* out_batch) {
    PLONK_REQUIRE(p && out_batch, PLONK_ERR_ARG, "bad argument");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    StagedSlot& sl = p->staged;
    plonk_prover::Intake& in = p->intake;
    PLONK_REQUIRE_ONE_CIRCUIT(p, "advance");
    PLONK_REQUIRE(sl.batch, PLONK_ERR_STATE, "advance: no batch is staged");
    PLONK_TRY(labels_commit(p, sl.batch, ctx->stream, false));  // a staged batch takes no labels: circuit 0 (pending ones wait for an upload)
    const size_t B = sl.batch;
    PLONK_TRY(ensure_rounds(p, B));  // a staged batch larger than any before: the rounds' own buffers grow here, behind the outgoing batch
    PLONK_CHECK_HIP(hipStreamWaitEvent(ctx->stream, sl.ready, 0));
    std::swap(p->rounds.wit_lag, sl.wit_lag);
    std::swap(in.pub, sl.pub);
    std::swap(in.cap_b, sl.cap_b);
    std::swap(in.vars, sl.vars);
    std::swap(in.inputs, sl.inputs);
    std::swap(in.bad_input, sl.bad_input);
    std::swap(in.bad_stride, sl.bad_stride);
    std::swap(p->solver.bad, sl.solve_bad);
    in.vars_valid = true;
    p->solver.valid = sl.solved;
    in.resident_b = B;
    sl.batch = 0;
    PLONK_CHECK_HIP(hipEventRecord(sl.released, ctx->stream));
    sl.released_pending = true;
    *out_batch = B;
    return PLONK_OK;
}

// witness columns [3][B][n] (A, B, C) and public inputs [B][n_public], canonical LE
int plonk_prover_upload_witness(plonk_prover* p, const uint8_t* abc_le32, const uint8_t* public_le32, size_t B) {
    PLONK_REQUIRE(p && abc_le32 && B && (public_le32 || !p->circuit.n_public), PLONK_ERR_ARG, "bad argument");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    PLONK_TRY(labels_check(p, B));
    // a public row is [n_public] of the widest circuit: beyond its own circuit's count it must be zero, or PI would not be the circuit's
    const size_t l_max = p->circuit.n_public;
    for (size_t b = 0; b < B && p->labels.pending_batch; b++)
        for (size_t k = 32 * (b * l_max + p->circuit.n_public_of[p->labels.pending[b]]); k < 32 * (b + 1) * l_max; k++)
            PLONK_REQUIRE(!public_le32[k], PLONK_ERR_ARG, "proof %zu: public value %zu is not zero, and circuit %u has %zu public inputs", b,
                          k / 32 - b * l_max, p->labels.pending[b], p->circuit.n_public_of[p->labels.pending[b]]);
    PLONK_TRY(ensure_batch(p, B));
    p->intake.resident_b = 0;
    PLONK_TRY(labels_commit(p, B, ctx->stream));
    if (p->intake.bad_input) PLONK_CHECK_HIP(hipMemsetAsync(p->intake.bad_input, 0xff, sizeof(unsigned long long), ctx->stream));
    PLONK_TRY(plonk_fr_upload(ctx, p->rounds.wit_lag, abc_le32, 3 * B * p->circuit.n));
    if (p->circuit.n_public) PLONK_TRY(plonk_fr_upload(ctx, p->intake.pub, public_le32, B * p->circuit.n_public));
    PLONK_TRY(fill_pi_column(p, p->rounds.wit_lag, p->intake.pub, B, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    p->intake.resident_b = B;
    p->intake.vars_valid = p->solver.valid = false;
    return PLONK_OK;
}

// cell_index[3][n]: variable index carried by each wire cell (column L/R/O, row), n_vars for an empty cell or a
// padding row; public_index[n_public]: the public variables, in the order of the public rows (prover.py:57-62).
// plonk_prover_set_wiring_multi: the same for every circuit of the table, cell_index[K][3][n] and public_index[K][n_public] with
// n_public the widest circuit's: a circuit's row holds its own public variables, then n_vars as the padding entry.  One n_vars
// serves the table; every circuit's variables are numbered in its own order.
int plonk_prover_set_wiring_multi(plonk_prover* p, const uint32_t* cell_index, const uint32_t* public_index, size_t n_vars) {
    PLONK_REQUIRE(p && cell_index && n_vars && (public_index || !p->circuit.n_public), PLONK_ERR_ARG, "bad argument");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    PLONK_REQUIRE(!p->staged.batch, PLONK_ERR_STATE, "set_wiring: a batch of %zu is staged under the wiring in force", p->staged.batch);
    plonk_prover::Wiring& w = p->wiring;
    const size_t K = p->circuit.n_circuits, cells = K * 3 * p->circuit.n, l_max = p->circuit.n_public, l = K * l_max;
    for (size_t k = 0; k < cells; k++)
        PLONK_REQUIRE(cell_index[k] <= n_vars, PLONK_ERR_ARG, "wire cell %zu names variable %u of %zu", k, cell_index[k], n_vars);
    for (size_t k = 0; k < l; k++) {
        const bool own = k % l_max < p->circuit.n_public_of[k / l_max];
        PLONK_REQUIRE(!own || public_index[k] < n_vars, PLONK_ERR_ARG, "public input %zu names variable %u of %zu", k, public_index[k], n_vars);
        PLONK_REQUIRE(own || public_index[k] == n_vars, PLONK_ERR_ARG, "public entry %zu pads its circuit's row: %u is not the marker %zu", k,
                      public_index[k], n_vars);
    }
    if (!w.cell_index) PLONK_TRY(dev_alloc((void**)&w.cell_index, cells * sizeof(uint32_t)));
    if (!w.pub_index) PLONK_TRY(dev_alloc((void**)&w.pub_index, (l + 1) * sizeof(uint32_t)));
    PLONK_CHECK_HIP(hipMemcpyAsync(w.cell_index, cell_index, cells * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (l) PLONK_CHECK_HIP(hipMemcpyAsync(w.pub_index, public_index, l * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (!w.cell_host) w.cell_host = (uint32_t*)malloc(cells * sizeof(uint32_t));
    PLONK_REQUIRE(w.cell_host, PLONK_ERR_NOMEM, "out of host memory");
    memcpy(w.cell_host, cell_index, cells * sizeof(uint32_t));
    w.n_vars = n_vars;
    p->solver.n_inputs = 0;  // a plan belongs to the wiring it was built from: it goes, with its schedule
    dev_free_all({(void**)&p->solver.desc, (void**)&p->solver.order, (void**)&p->solver.level_start});
    p->intake.vars_valid = false;
    return PLONK_OK;
}

int plonk_prover_set_wiring(plonk_prover* p, const uint32_t* cell_index, const uint32_t* public_index, size_t n_vars) {
    PLONK_REQUIRE(p, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(p->circuit.n_circuits == 1, PLONK_ERR_STATE, "a prover over a table of %u circuits is wired with plonk_prover_set_wiring_multi",
                  p->circuit.n_circuits);
    return plonk_prover_set_wiring_multi(p, cell_index, public_index, n_vars);
}

// The circuit of each proof of the NEXT upload, which must be of `batch` proofs: circuit[b] < the table's K.  They serve that one
// upload, as plonk_prover_set_blinders serves the next run, and stay with the batch it makes resident.
int plonk_prover_set_labels(plonk_prover* p, const uint32_t* circuit, size_t batch) {
    PLONK_REQUIRE(p && circuit && batch, PLONK_ERR_ARG, "bad argument");
    for (size_t b = 0; b < batch; b++)
        PLONK_REQUIRE(circuit[b] < p->circuit.n_circuits, PLONK_ERR_ARG, "proof %zu: circuit %u of a table of %u", b, circuit[b], p->circuit.n_circuits);
    plonk_prover::Labels& lb = p->labels;
    uint32_t* mem = (uint32_t*)realloc(lb.pending, batch * sizeof(uint32_t));
    PLONK_REQUIRE(mem, PLONK_ERR_NOMEM, "out of host memory");
    lb.pending = mem;
    memcpy(lb.pending, circuit, batch * sizeof(uint32_t));
    lb.pending_batch = batch;
    return PLONK_OK;
}

int plonk_prover_upload_variables(plonk_prover* p, const uint8_t* vars_le32, size_t B) { return prover_upload(p, vars_le32, B, false, false); }
int plonk_prover_upload_variables_async(plonk_prover* p, const uint8_t* vars_le32, size_t B) { return prover_upload(p, vars_le32, B, false, true); }

// The circuit's inputs: the variables a batch will give values for.  Builds the solver's plan from the gate columns
// plonk_prover_create was given and the wiring; a refusal that names a variable (one that no row assigns before it is read, or
// at all) sets *out_missing_var to it, any other sets it to 0xffffffff.
int plonk_prover_set_inputs(plonk_prover* p, const uint32_t* input_index, size_t n_inputs, uint32_t* out_missing_var) {
    PLONK_REQUIRE(p && input_index && n_inputs && out_missing_var, PLONK_ERR_ARG, "bad argument");
    *out_missing_var = SOLVE_NO_VARIABLE;
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    PLONK_REQUIRE_ONE_CIRCUIT(p, "set_inputs");
    PLONK_REQUIRE(p->wiring.n_vars && p->wiring.cell_host, PLONK_ERR_STATE, "plonk_prover_set_wiring has not been called");
    PLONK_REQUIRE(!p->staged.batch, PLONK_ERR_STATE, "set_inputs: a batch of %zu is staged under the plan in force", p->staged.batch);
    plonk_prover::Solver& sv = p->solver;
    SolvePlan plan;
    PLONK_TRY(solve_plan_build(sv.gates_host, p->wiring.cell_host, p->circuit.n, p->wiring.n_vars, input_index, n_inputs, plan, out_missing_var));
    const std::vector<uint32_t>& desc = plan.desc;
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // a batch in flight still walks the old plan
    sv.n_inputs = 0;
    p->intake.resident_b = 0;
    dev_free_all({(void**)&sv.desc, (void**)&sv.order, (void**)&sv.level_start, (void**)&sv.input_index, (void**)&p->intake.inputs.buf, (void**)&sv.bad,
                  (void**)&p->staged.inputs.buf, (void**)&p->staged.solve_bad});  // (the staged set's: C has waited for the stage that used them)
    p->intake.inputs.cap = p->staged.inputs.cap = 0;
    PLONK_TRY(dev_alloc((void**)&sv.desc, desc.size() * sizeof(uint32_t)));
    PLONK_TRY(dev_alloc((void**)&sv.order, plan.order.size() * sizeof(uint32_t)));
    PLONK_TRY(dev_alloc((void**)&sv.level_start, plan.level_start.size() * sizeof(uint32_t)));
    PLONK_TRY(dev_alloc((void**)&sv.input_index, n_inputs * sizeof(uint32_t)));
    if (!plan.order.empty())
        PLONK_CHECK_HIP(hipMemcpyAsync(sv.order, plan.order.data(), plan.order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PLONK_CHECK_HIP(hipMemcpyAsync(sv.level_start, plan.level_start.data(), plan.level_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (!desc.empty()) PLONK_CHECK_HIP(hipMemcpyAsync(sv.desc, desc.data(), desc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PLONK_CHECK_HIP(hipMemcpyAsync(sv.input_index, input_index, n_inputs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    sv.rows = (uint32_t)desc.size();
    sv.active = (uint32_t)plan.order.size();
    sv.levels = (uint32_t)plan.level_start.size() - 1;
    sv.widest = plan.widest;
    sv.threads = plan.threads;
    sv.steps = plan.steps;
    sv.n_inputs = n_inputs;
    return PLONK_OK;
}

int plonk_prover_upload_inputs(plonk_prover* p, const uint8_t* inputs_le32, size_t B) { return prover_upload(p, inputs_le32, B, true, false); }
int plonk_prover_upload_inputs_async(plonk_prover* p, const uint8_t* inputs_le32, size_t B) { return prover_upload(p, inputs_le32, B, true, true); }

// [B][k] canonical LE values of the variables var_index[0 .. k) of the resident batch (var_index == NULL: all n_vars, k
// ignored), after either kind of variable upload: what the solver computed — a public input among it — for the verifier
int plonk_prover_download_variables(plonk_prover* p, size_t B, const uint32_t* var_index, size_t k, uint8_t* out_le32) {
    PLONK_REQUIRE(p && B && out_le32 && (k || !var_index), PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(B == p->intake.resident_b, PLONK_ERR_STATE, "download_variables: batch %zu, but %zu witnesses are resident", B, p->intake.resident_b);
    PLONK_REQUIRE(p->intake.vars_valid, PLONK_ERR_STATE, "the resident batch was uploaded as wire columns: it has no variable values");
    plonk_ctx* ctx = p->circuit.ctx;
    PLONK_ENTER(ctx);
    const size_t V = p->wiring.n_vars;
    if (!var_index) k = V;
    for (size_t j = 0; var_index && j < k; j++)
        PLONK_REQUIRE(var_index[j] < V, PLONK_ERR_ARG, "index %zu names variable %u of %zu", j, var_index[j], V);
    void* tmp;
    PLONK_TRY(ctx_scratch(ctx, 3, B * k * sizeof(Fr) + k * sizeof(uint32_t), &tmp));
    Fr* vals = (Fr*)tmp;
    uint32_t* d_index = nullptr;
    if (var_index) {
        d_index = reinterpret_cast<uint32_t*>(vals + B * k);
        PLONK_CHECK_HIP(hipMemcpyAsync(d_index, var_index, k * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    PLONK_LAUNCH(variable_gather_kernel, grid1(B * k), dim3(256), 0, ctx->stream, (const Fr*)p->intake.vars.buf, (const uint32_t*)d_index, V, k, B, vals);
    PLONK_CHECK_HIP(hipGetLastError());
    PLONK_CHECK_HIP(hipMemcpyAsync(out_le32, vals, B * k * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return PLONK_OK;
}

// per proof of the resident batch, 0 or 1 + the first row whose check failed (PROVER_ST_ASSERT); a batch that did not come
// through the solver has none
int plonk_prover_solve_failures(plonk_prover* p, size_t B, uint32_t* out_rows) {
    PLONK_REQUIRE(p && B && out_rows, PLONK_ERR_ARG, "bad argument");
    PLONK_REQUIRE(B == p->intake.resident_b, PLONK_ERR_STATE, "solve_failures: batch %zu, but %zu witnesses are resident", B, p->intake.resident_b);
    PLONK_ENTER(p->circuit.ctx);
    if (!p->solver.valid) {
        memset(out_rows, 0, B * sizeof(uint32_t));
        return PLONK_OK;
    }
    PLONK_CHECK_HIP(hipMemcpyAsync(out_rows, p->solver.bad, B * sizeof(uint32_t), hipMemcpyDeviceToHost, p->circuit.ctx->stream));
    PLONK_CHECK_HIP(hipStreamSynchronize(p->circuit.ctx->stream));
    return PLONK_OK;
}

// DIAGNOSTICS: the solver's plan and what the rule makes of it for `batch` proofs: out = rows walked, active rows, levels, the
// widest level, T (the levelised kernel's block), the form solve_plan_form picks (1 = one lane per proof, 2 = levels), and the
// levelised form's steps
int plonk_prover_solve_plan(plonk_prover* p, size_t batch, uint32_t out[7]) {
    PLONK_REQUIRE(p && batch && out, PLONK_ERR_ARG, "bad argument");
    PLONK_ENTER(p->circuit.ctx);
    const plonk_prover::Solver& sv = p->solver;
    PLONK_REQUIRE_ONE_CIRCUIT(p, "solve_plan");
    PLONK_REQUIRE(sv.n_inputs, PLONK_ERR_STATE, "plonk_prover_set_inputs has not been called");
    const uint32_t plan[7] = {sv.rows, sv.active, sv.levels, sv.widest, sv.threads,
                              solve_plan_form(device_cus(p->circuit.ctx->device), sv.active, sv.steps, sv.threads, batch), sv.steps};
    memcpy(out, plan, sizeof plan);
    return PLONK_OK;
}

}  // extern "C"
