// plonk_internal.h — context object and helpers shared by the C-ABI implementation files.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/plonk_hip.h"
#include "fp.h"
#include "g1.h"

void plonk_set_error(const char* fmt, ...);

#define PLONK_CHECK_HIP(expr)                                                                     \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            plonk_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PLONK_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)

// Allocation that may fail and be recovered from (the caller frees something and retries, or falls back to a smaller table):
// HIP parks the failure in its thread-local last-error slot, where the next `PLONK_CHECK_HIP(hipGetLastError())` after a kernel
// launch would find it and report a stale out-of-memory as PLONK_ERR_HIP.  The slot is emptied here, at the failing call.
template <class T> static inline bool plonk_dev_malloc(T** p, size_t bytes) {
    if (hipMalloc((void**)p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}
template <class T> static inline bool plonk_host_malloc(T** p, size_t bytes) {
    if (hipHostMalloc((void**)p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}

// an object's own device buffers (prover, verifier): allocation that reports, and the one way to release — every pointer
// that is set is freed and nulled
static inline int dev_alloc(void** p, size_t bytes) {
    if (plonk_dev_malloc(p, bytes ? bytes : 32)) return PLONK_OK;
    plonk_set_error("hipMalloc(%zu) failed", bytes);
    return PLONK_ERR_NOMEM;
}
static inline void dev_free_all(std::initializer_list<void**> ptrs) {
    for (void** q : ptrs) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
}
// Grow device buffers that share one capacity (in the caller's units): nothing while `need` fits; otherwise wait for the stream
// that may still be using them, free them, allocate each anew.  *cap is 0 while any of them is missing.
struct DevBuf { void** ptr; size_t bytes; };
static inline int dev_grow(hipStream_t stream, size_t* cap, size_t need, std::initializer_list<DevBuf> bufs) {
    if (need <= *cap) return PLONK_OK;
    PLONK_CHECK_HIP(hipStreamSynchronize(stream));
    for (const DevBuf& b : bufs) dev_free_all({b.ptr});
    *cap = 0;
    for (const DevBuf& b : bufs)
        if (int rc = dev_alloc(b.ptr, b.bytes)) return rc;
    *cap = need;
    return PLONK_OK;
}

// a small integer in Montgomery form, and 1 / 2^log_n (the inverse transform's factor): the host-side routines of every field
template <class P> static inline Fp<P> host_fp_u64(uint64_t x) {
    Fp<P> a = fp_zero<P>();
    a.v[0] = (uint32_t)x;
    a.v[1] = (uint32_t)(x >> 32);
    return fp_to_mont(a);
}
template <class P> static inline Fp<P> host_fp_inv_pow2(unsigned log_n) { return fp_inv(host_fp_u64<P>((uint64_t)1 << log_n)); }
static inline Fr host_fr_u64(uint64_t x) { return host_fp_u64<FrParams>(x); }

#define PLONK_REQUIRE(cond, code, ...)    \
    do {                                  \
        if (!(cond)) {                    \
            plonk_set_error(__VA_ARGS__); \
            return (code);                \
        }                                 \
    } while (0)

// HIP's current device is per thread; every entry point that touches a context makes its device current first
// (a process may hold contexts on several GPUs).
int plonk_use_device(int device);
#define PLONK_ENTER(ctx)                                                  \
    do {                                                                  \
        int rc_enter_ = plonk_use_device((ctx)->device);                  \
        if (rc_enter_ != PLONK_OK) return rc_enter_;                      \
    } while (0)

#define PLONK_TRY(expr)          \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != PLONK_OK) return rc_; \
    } while (0)

// Key of an entry in the transform engine's per-context caches (tables and launch plans): a cache names the fields its entries depend on,
// distinct fields give distinct keys.  SCALED: the table (or the plan's output) carries the inverse's 1/N; FULL, LATENCY, BIG: a plan's form (ntt_policy_form)
enum : unsigned { NTT_KEY_SCALED = 1, NTT_KEY_FULL = 2, NTT_KEY_LATENCY = 4, NTT_KEY_BIG = 8 };
static inline unsigned ntt_key(unsigned log_n, bool inverse, unsigned flags = 0, unsigned log_r1 = 0, unsigned log_e = 0) {
    return log_n | (inverse ? 64u : 0u) | (flags << 8) | (log_r1 << 16) | (log_e << 24);  // log_n <= 32, log_r1 <= 13, log_e <= 3
}

// device tables of the wave NTT kernels for one field, cached per context (the memory is in plonk_ctx::owned); keys: ntt_key
struct WaveTables {
    std::map<unsigned, int32_t*> prog;          // a kernel's twiddles in program order, per (size, direction, elements per thread as log_e)
    std::map<unsigned, int32_t*> lo, hi;        // the two-level inter-pass twiddles, per (size, direction); hi also SCALED
    std::map<unsigned, int32_t*> interpass;     // full inter-pass tables, per (size, direction, SCALED, log_r1, log_e of the column kernel)
    const int32_t* jm = nullptr;                // fpl_reduce_small's multiples of the modulus
    bool attr_set[4] = {false, false, false, false};   // hipFuncSetAttribute is per device: tracked per context (E = 4, E = 8, E = 4 column kernel, the 512-thread 2^12 kernel)
    std::map<unsigned, void*> packed[3];        // packed source tables (full, lo, hi) of a field that has no cache of its own (BLS12-381 Fr), per (size, direction)
    std::map<unsigned, std::shared_ptr<void>> plans;  // WavePlan<P> per (size, direction, SCALED, FULL, LATENCY, BIG): ntt_wave_host.h
    unsigned plan_epoch = 0;                    // plonk_ctx::ntt_cfg_epoch the plans were built under
};

struct NttTables {
    // per (size, direction)
    std::map<unsigned, Fr*> small;   // w_R^k, k < R/2              (per-pass LDS twiddles)
    std::map<unsigned, Fr*> lo, hi;  // w_N^e = lo[e & 1023] * hi[e >> 10]   (inter-pass twiddles)
    std::map<unsigned, Fr*> full;    // w_N^k, k < N                 (barycentric / permutation argument)
    WaveTables wave;                 // the wave NTT kernels' tables for BN254 Fr (ntt_wave_host.h)
};

#define MSM_TABLE_COMB 1
#define MSM_TABLE_WINDOWS 2
// One lookup table per (process, device, base set), shared by every plonk_srs / context / stream that
// loads the same bases (msm_tables.h keeps the registry; reference counted, freed with its last plonk_srs).
struct MsmLookupTable {
    int device = 0;
    uint64_t key = 0;        // FNV-1a of the host bytes the bases were loaded from
    size_t n_points = 0;
    unsigned kind = 0;       // MSM_TABLE_COMB (msm_comb.h: bits = teeth h, windows = columns a) or MSM_TABLE_WINDOWS (bits = c, windows = W)
    unsigned bits = 0, windows = 0;
    unsigned top_bits = 0, top_g = 0;  // comb with top tables (msm_comb.h: windows = floor(254 / bits)): R and the bases per group; 0, 0 = none
    G1Affine* data = nullptr;  // comb: data[(i << (h - 1)) + idx]; windows: data[((w * n_points + i) << (c - 1)) + d - 1]
    size_t bytes = 0;
    uint8_t* base_skip = nullptr;  // comb: base_skip[i] = 1 where base i is the identity — every entry of its block is, and its items are skipped (n_points bytes, device)
    double build_s = 0;      // wall time of the build (reported by bench.py)
    int refs = 0;
};

struct plonk_srs {
    int device = 0;
    uint64_t content_key = 0;   // FNV-1a of the loaded bytes: identifies the base set in the lookup-table registry
    size_t n_points = 0;
    G1Affine* bases = nullptr;  // device, Montgomery coordinates (.ptau layout)
    unsigned window_bits = 0;   // c of the current window table (0 = not built)
    unsigned n_windows = 0;
    G1Affine* table = nullptr;  // device: table[w * n_points + i] = 2^(c*w) * bases[i]
    // table MSM (msm_tables.h): multiples of the bases resident in HBM
    bool fixed = false;          // a reusable SRS (plonk_srs_load_ptau): worth a big table
    bool lookup_failed = false;  // an automatic build did not fit: do not retry on every call
    MsmLookupTable* shared = nullptr;  // the attached table (null = none)
    // Lagrange-basis SRS (setup.py:66-72 without the ifft): lagrange[log_n] = [L_i(tau)]_1, i < 2^log_n, built on
    // demand by an EC inverse NTT of the first 2^log_n bases (msm.hip); each is a plonk_srs of its own.
    std::map<unsigned, plonk_srs*> lagrange;
    plonk_srs* parent = nullptr;  // a Lagrange view's SRS (its table is charged against the parent's budget)
};

#define PLONK_SCRATCH_SLOTS 4
struct plonk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host-to-device staging that overlaps the compute stream (created on first use: ctx_copy_stream)
    NttTables tw;
    std::map<std::string, Fr*> power_tables;  // cached coset-offset power tables, keyed by (offset, n, kind)
    std::vector<void*> owned;                 // device allocations released with the context
    void* scratch[PLONK_SCRATCH_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t scratch_bytes[PLONK_SCRATCH_SLOTS] = {0, 0, 0, 0};
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    Fr host_tmp[16];                 // small host-side staging that must outlive an asynchronous copy (every user synchronises before returning)
    unsigned msm_window_bits = 0, msm_groups = 0;
    int msm_lookup_mode = 0;         // 0 auto (fixed SRS only), 1 off, 2 force msm_lookup_bits for every base set
    unsigned msm_lookup_bits = 0;    // 0 = the table with the fewest additions per base that fits the budget
    bool msm_lookup_top = false;     // with explicit msm_lookup_bits: the comb WITH top tables (plonk_msm_lookup_configure mode | 32)
    bool msm_comb_wide = false;      // test flag (plonk_msm_lookup_configure mode | 64): the comb kernel with the 64-bit entry index whatever the table's size
    unsigned msm_comb_walk = 0;      // test flags (plonk_msm_lookup_configure mode | 128, | 256): 1 the comb's row walk, 2 its column-lane kernel, whatever the rule says (0)
    // device: the recovery list of this context's last MSM call (msm_common.h; its first word counts the MSMs redone), read by
    // plonk_msm_recovery_count.  It points INTO scratch slot 1, which ctx_scratch may free and move: valid only because every user of slot 1
    // goes through msm_run_device, which clears it before the method's run takes the slot and sets it after enqueueing its kernels.
    uint32_t* msm_redo = nullptr;
    unsigned msm_lookup_kind = MSM_TABLE_COMB;  // layout of the tables this context builds (plonk_msm_lookup_configure: mode | 16 = window tables)
    size_t msm_lookup_budget = 0;    // bytes; 0 = default (PLONK_MSM_TABLE_GB if set, else min(device memory / 16, free memory / 4): msm_tables.h)
    bool ntt_attr_set = false, msm_attr_set = false;  // hipFuncSetAttribute is per device: tracked per context
    // per-kernel HIP-event profiling (bench.py roofline): one record per instrumented launch
    struct ProfRec { const char* name; hipEvent_t a, b; double algo_bytes; };
    bool profiling = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    unsigned ntt_tile_log = 12, ntt_single_log = 11, ntt_radix_log = 10;
    bool ntt_adaptive_tiles = true;
    WaveTables wave_bls;  // the same for the standalone BLS12-381 Fr transform (ntt_bls.hip)
    size_t ntt_table_budget = (size_t)4 << 30, ntt_tables_bytes = 0;  // full inter-pass twiddle tables (80 B per point and direction): plonk_ntt_set_table_budget
    unsigned char ntt_split[32] = {0};  // plonk_ntt_set_split: log2 R1 of the two-pass wave plan per log2 N (0 = default)
    unsigned ntt_cfg_epoch = 0;  // bumped by every plonk_ntt_* setter: cached launch plans are rebuilt
    unsigned ntt_kind = 0;  // an NttKind (ntt_wave_host.h, with the policy it selects): plonk_ntt_select_kernel
};

// grid of a grid-stride kernel over n items
static inline dim3 grid1(size_t n, unsigned block = 256, size_t cap = 4096) {
    size_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (!g) g = 1;
    return dim3((unsigned)g);
}

// scratch slot use: 0 = NTT inter-pass buffer, 1 = MSM digits/partials, 2-3 = API-level temporaries
int ctx_scratch(plonk_ctx* ctx, int slot, size_t bytes, void** out);
// a device table released with the context (plonk_ctx::owned); `entries` goes into the out-of-memory message (0: none — the caller has a fallback, or its own text)
int ctx_table_alloc(plonk_ctx* ctx, size_t bytes, size_t entries, void** out);
int ctx_copy_stream(plonk_ctx* ctx);
// bracket an instrumented launch: prof_begin before, prof_end after (no-ops unless profiling)
int prof_begin(plonk_ctx* ctx, const char* name, double algo_bytes);
int prof_end(plonk_ctx* ctx);

// ---- enqueue helpers shared between translation units (all on ctx->stream) ---------------------
// fr_ops.hip
int k_fr_to_mont(plonk_ctx*, const Fr* in, Fr* out, size_t n);
int k_fr_from_mont(plonk_ctx*, const Fr* in, Fr* out, size_t n);
int k_fr_to_mont_checked(plonk_ctx*, Fr* data, size_t n, unsigned long long* d_first_bad);
int k_fr_to_mont_checked_on(hipStream_t stream, Fr* data, size_t n, unsigned long long* d_first_bad);  // the same on a stream given (the copy stream: a staged batch)
int k_fr_pointwise(plonk_ctx*, int op, const Fr* a, const Fr* b, Fr* out, size_t n);
int k_fr_pointwise_scalar(plonk_ctx*, int op, const Fr* a, const Fr& s_mont, Fr* out, size_t n, size_t limit);
int k_fr_batch_inverse(plonk_ctx*, const Fr* in, Fr* out, size_t n);
int k_fr_powers(plonk_ctx*, const Fr& base_mont, const Fr& first_mont, Fr* out, size_t n);
int k_fr_rotate(plonk_ctx*, const Fr* in, Fr* out, size_t n, size_t shift, size_t batch);
int k_fr_barycentric(plonk_ctx*, const Fr* vals, const Fr* roots, unsigned log_n, const Fr* xs_dev, size_t x_stride,
                     const Fr& n_inv_mont, Fr* out_dev, size_t n_polys);
int k_fr_barycentric_ptrs(plonk_ctx*, const Fr* const* polys, const Fr* roots, unsigned log_n, const Fr* xs_dev, const Fr& n_inv_mont,
                          Fr* out_dev, size_t n_polys);  // <= 16 polynomials in separate buffers, one point each
int k_fr_lincomb(plonk_ctx*, const Fr* const* terms, const Fr* scalars_mont, unsigned n_terms, const Fr& constant_mont, Fr* out, size_t n);  // <= 20 terms
int k_fr_count_diff(plonk_ctx*, const Fr* a, const Fr* b_or_null, size_t n, unsigned long long* d_count);
// api.hip
Fr fr_from_le32(const uint8_t* b);                 // canonical little-endian bytes -> Montgomery form (host)
bool le32_below_modulus(const uint8_t* b, bool fq);
int get_power_table(plonk_ctx*, const Fr& base, const Fr& first, size_t n, const Fr** out);  // first * base^i, cached per context
unsigned device_cus(int device);                   // compute units, cached per device (the MSM's launch rounds, the prover's segments)
// ntt.hip
Fr host_root_of_unity(unsigned log_n, bool inverse);
// fan (optional): every batch entry is transformed `count` times — copy f reads in + f in_stride, writes out + f out_stride
// and takes its scaling vector at in_scale / out_scale + f scale_stride (elements): one launch on the wave kernels' single-pass
// sizes (the prover: a coefficient vector evaluated on three cosets), a loop of calls elsewhere
struct NttFan { unsigned count, in_stride, out_stride, scale_stride; };
// One call of the engine: `batch` transforms of 2^log_n points, entry b read at in + b in_bstride (its first in_len elements; the
// rest count as zero) and written at out + b out_bstride.  in_scale / out_scale: vectors multiplied in at the first load / last
// store; scale_by_n_inv: the output times 1/N.  A length or stride of 0 stands for N = 2^log_n (ntt_run and wave_run resolve it
// first thing; no caller means a zero-length input, so nothing is misread).  E: the field's element (BLS12-381 Fr: ntt_bls.hip).
template <class E> struct NttCallT {
    const E* in; E* out; unsigned log_n; bool inverse;
    size_t batch = 1;
    size_t in_len = 0, in_bstride = 0, out_bstride = 0;  // 0 = N
    const E* in_scale = nullptr; const E* out_scale = nullptr;
    bool scale_by_n_inv = false;
    NttFan fan = {};  // count <= 1: none
};
typedef NttCallT<Fr> NttCall;
// the common shapes: `batch` contiguous vectors, forward, or inverse with its 1/N
template <class E> static inline NttCallT<E> ntt_forward(const E* in, E* out, unsigned log_n, size_t batch) { return NttCallT<E>{in, out, log_n, false, batch}; }
template <class E> static inline NttCallT<E> ntt_inverse(const E* in, E* out, unsigned log_n, size_t batch) {
    NttCallT<E> t{in, out, log_n, true, batch};
    t.scale_by_n_inv = true;
    return t;
}
template <class E> static inline NttCallT<E> ntt_call_resolved(NttCallT<E> t) {
    const size_t N = (size_t)1 << t.log_n;
    if (!t.in_len) t.in_len = N;
    if (!t.in_bstride) t.in_bstride = N;
    if (!t.out_bstride) t.out_bstride = N;
    return t;
}
int ntt_run(plonk_ctx*, const NttCall&);
int ntt_get_roots(plonk_ctx*, unsigned log_n, bool inverse, const Fr** table_full);
int ntt_dist_plan(unsigned log_n, unsigned log_w, unsigned* log_r1, unsigned* log_r2);
bool ntt_wave_plan(const plonk_ctx* ctx /* null: the default splits */, unsigned log_n, bool latency, unsigned* log_r1, unsigned* log_r2);
int ntt_dist_columns(plonk_ctx*, const Fr* in, Fr* out, unsigned log_n, unsigned log_w, unsigned rank, bool inverse);
int ntt_dist_rows(plonk_ctx*, const Fr* in, Fr* out, unsigned log_n, unsigned log_w, unsigned rank, bool inverse);
// msm.hip
int msm_lagrange_srs(plonk_ctx*, plonk_srs*, unsigned log_n, plonk_srs** out);  // owned by (and freed with) the parent
void g1_batch_to_affine(plonk_ctx*, const G1Xyzz* in, G1Affine* out, size_t n, size_t max_groups = 65536);  // enqueue: XYZZ -> affine (Montgomery), identity -> (0, 0)
void msm_window_bases(plonk_ctx*, const G1Affine* bases, size_t n, unsigned c, unsigned W, G1Xyzz* out);  // enqueue: out[w * n + i] = 2^(c w) bases[i]
// g1_ntt.hip: the same Lagrange-basis points by an inverse DFT over the group (n log n group operations)
int g1_lagrange_by_ntt(plonk_ctx*, const plonk_srs*, unsigned log_n, G1Affine* d_bases_out);
// msm_tables.h
void msm_srs_release(plonk_srs*);  // drops the reference on the shared lookup table
int msm_lookup_info(const plonk_srs*, unsigned* bits, size_t* bytes, double* build_s, int* sharers);
int msm_lookup_layout(const plonk_srs*, unsigned* kind, unsigned* additions_per_base);
int msm_lookup_top(const plonk_srs*, unsigned* top_bits, unsigned* bases_per_group);
bool msm_comb_takes_top(unsigned teeth);  // msm_comb.h: a comb of this many teeth can take top tables
uint64_t plonk_fnv1a64(const void* data, size_t n);
// MSM m reads its scalars at d_scalars + (m % inner) * stride + (m / inner) * outer_stride (inner = 0: inner = M)
int msm_run_device(plonk_ctx*, plonk_srs*, const Fr* d_scalars, size_t n, size_t M, size_t stride, Fq* d_out_xy,
                   uint8_t* d_flags, size_t inner = 0, size_t outer_stride = 0);
// prover.hip
struct plonk_prover;
int prover_pack_device(plonk_prover* p, size_t B, int compressed, uint8_t* d_proofs, uint8_t* d_status, hipEvent_t done);
plonk_ctx* prover_ctx(plonk_prover* p);
size_t prover_record_bytes(int compressed);  // bytes of one packed proof record (prover.h)
