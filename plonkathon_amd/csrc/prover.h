// prover.h — what prover.hip and verifier.hip share (internal): the per-proof state, the resident batch, the status bits and the
// layout of a proof record.
#pragma once
#include <type_traits>

#include "plonk_internal.h"
#include "transcript_device.h"

#define NEVAL 7  // a, b, c, s1, s2, z_shifted, PI(zeta)

struct ProofState {
    Fr beta, gamma, alpha, fft_cofactor, zeta, v;
    Fr evals[NEVAL];
    MerlinState transcript;
    uint32_t error;  // 1: a commitment was the identity (the reference's append_point(None) raises)
    uint32_t pad_[3];
};

// The challenges of rounds 2 and 3 where a kernel runs outside a proof's transcript (st == null: plonk_fr_grand_product,
// plonk_fr_quotient); the lock-step prover's kernels read them from the ProofStates and pass an empty one.
struct RoundChallenges { Fr beta, gamma, alpha; };

// the prover's status byte (pack_status_kernel; 0 = the proof is good)
#define PROVER_ST_IDENTITY 1u   // a commitment was the identity
#define PROVER_ST_Z_OPEN 2u     // Z does not close to 1: the witness breaks the copy constraints (prover.py:132)
#define PROVER_ST_GATE 4u       // a gate constraint fails on some row (prover.py:108-116)
#define PROVER_ST_BAD_INPUT 8u  // an asynchronously uploaded value was not below r
#define PROVER_ST_ASSERT 16u    // the witness solver's check of a row whose output was already known failed (compiler/program.py:185-186)

// A proof record: nine commitments a_1, b_1, c_1, z_1, t_lo_1, t_mid_1, t_hi_1, W_z_1, W_zw_1, then the six evaluations a, b, c,
// s1, s2, z_shifted.  Plain: x || y and the evaluations as canonical little-endian words.  Compressed (g1_codec.h): 32 bytes per
// point, the evaluations big-endian.
#define PROOF_POINTS 9
#define PROOF_EVALS 6
#define PROOF_BYTES (64 * PROOF_POINTS + 32 * PROOF_EVALS)
#define PROOF_BYTES_COMPRESSED (32 * PROOF_POINTS + 32 * PROOF_EVALS)
#define PROOF_COMPRESSED_EVALS (32 * PROOF_POINTS)  // byte offset of the scalars in a compressed record
constexpr unsigned proof_point_word(unsigned k, unsigned h) { return 16 * k + 8 * h; }  // coordinate h (x, y) of point k, plain record
constexpr unsigned proof_eval_word(unsigned e) { return 16 * PROOF_POINTS + 8 * e; }
constexpr size_t proof_bytes(bool compressed) { return compressed ? PROOF_BYTES_COMPRESSED : PROOF_BYTES; }

#define PI_SPARSE_MAX 8
enum { FX_QM = 0, FX_QL, FX_QR, FX_QO, FX_QC, FX_S1, FX_S2, FX_S3, FX_COUNT };
#define PROVER_MAX_LOG_N 16  // the largest group order the lock-step prover accepts: what the suite checks (tests/test_gpu_prover_large.py)
#define QCOSETS 3  // cosets of size n the lock-step prover evaluates the quotient on (deg t < 3n)
#define QCOSETS_BLINDED 4  // under PLONK_PROVER_BLINDING (prover_blind.h): deg t = 3n + 5

// A device buffer that an upload fills on the copy stream while the previous batch may still be reading it.
struct Staging {
    Fr* buf;
    size_t cap;         // in the owner's units (below)
    hipEvent_t read;    // recorded behind the last kernel that reads buf (created with the buffer's first allocation)
    bool read_pending;  // `read` has been recorded: the next asynchronous copy into buf waits for it
};

// The second intake slot (prover_intake.h: stage, advance): everything a batch owns before the rounds run, for the ONE batch that is
// staged on the copy stream while the resident one proves.  plonk_prover_advance swaps these with the resident batch's (Rounds::wit_lag,
// the Intake fields of the same names, Solver::bad and Solver::valid).  All null until the first stage.
struct StagedSlot {
    size_t batch;              // the staged batch, 0: none
    size_t cap_b;              // proofs that wit_lag and pub hold
    Fr* wit_lag;               // [4][B][n]
    Fr* pub;                   // [B][n_public]
    Staging vars, inputs;      // as Intake's; their `read` events travel with the buffers
    unsigned long long* bad_input;
    size_t bad_stride;
    uint32_t* solve_bad;       // [B] (capacity: inputs.cap proofs, as Solver::bad)
    bool solved;               // the staged batch came through the solver
    hipEvent_t ready;          // recorded on the copy stream behind the stage's last kernel: advance makes the compute stream wait for it
    hipEvent_t released;       // recorded on the compute stream by advance, behind the last reader of the buffers that became this slot's
    bool released_pending;     // the next stage waits for `released` first
};

struct plonk_prover {
    // ---- the circuit: set by plonk_prover_create, constant afterwards
    struct Circuit {
        plonk_ctx* ctx;
        plonk_srs* srs;
        unsigned log_n;
        size_t n, n_public;  // n_public: of the widest circuit of the table (l_max); public rows are [n_public], zero beyond a circuit's own count
        // A prover over a table of K circuits of one group order (plonk_prover_create_multi): the three forms of the fixed polynomials,
        // the wiring's two index tables hold the circuits one after the other, and every kernel that reads them takes the proof's
        // circuit from Labels::dev.  K = 1 is plonk_prover_create's prover: its kernels get a null label array.
        unsigned n_circuits;   // K
        size_t* n_public_of;   // [K] host: each circuit's own number of public inputs
        Fr g;                // fixed coset offset (Montgomery)
        Fr w, n_inv, half;   // the n-th root of unity, 1 / n, 1 / 2
        // The quotient has degree < 3n, so THREE cosets of the n-th roots of unity determine it: x = g mu^r w^j, r < 3 (mu = the
        // 4n-th root of unity of prover.py:160), "coset-major" [r][j].  Every coset form below is [3][n] in that order.  A blinded
        // prover (prover_blind.h) takes all four: qcosets = 4, and plonk_prover_set_options rebuilds the coset forms as [4][n].
        unsigned qcosets;    // QCOSETS or QCOSETS_BLINDED
        Fr* fixed_lag;       // [K][8][n]   Lagrange values
        Fr* fixed_coef;      // [K][8][n]   coefficient forms
        Fr* fixed_big;       // [K][8][3][n]  the circuit polynomials on the three cosets
        Fr* l0_big;          // [3][n]
        Fr* x_big;           // [3][n]   the points g mu^r w^j
        Fr* g_pow;           // [3][n]   (g mu^r)^i: the load-side scaling of the size-n transform that evaluates on coset r
        Fr* ginv_pow;        // [3][n]   (g mu^r)^-i / 2n: the store-side scaling of the inverse transform of coset r (its 1/n folded in)
        const Fr* roots;     // [n]      w^i (owned by ctx)
        Fr zh[4], zh_inv[4]; // g^n * i^r - 1 and its inverse: Z_H is constant on a coset
        Fr comb_i, comb_g1, comb_g2;  // quotient_combine_kernel's constants: i = mu^n, 1 / g^n, 1 / g^2n
        // Public inputs are the only non-zero entries of the PI column (prover.py:57-62): with few of them PI's
        // coefficient and coset forms are cheaper from the Lagrange basis directly than through two transforms.
        bool sparse_pi;      // n_public <= PI_SPARSE_MAX
        Fr* li_big;          // [n_public][4n]  L_i on the coset: (w^i / n) Z_H(x_k) / (x_k - w^i)
        const Fr* roots_inv; // [n]             w^-i (owned by ctx)
        ChallengeConsts chal;  // for the challenge reduction in transcript_kernel
    } circuit;
    plonk_srs* lag_srs;   // plonk_prover_set_options: Lagrange-basis view of srs (PLONK_PROVER_LAGRANGE_COMMITS), owned by srs
    unsigned seg_forced;  // PLONK_PROVER_SEGMENTS_LOG2: k + 1 forces S = 2^k, 0 = prover_plan_segments
    bool blinding;        // PLONK_PROVER_BLINDING
    unsigned solve_forced;  // PLONK_PROVER_SOLVE_FORM: PLONK_PROVER_SOLVE_LANES or PLONK_PROVER_SOLVE_LEVELS for every input upload, 0 = solve_plan_form
    // ---- what the five rounds read and write: per-batch buffers (capacity cap_b proofs; prover.hip: batch_buffers)
    struct Rounds {
        size_t cap_b;
        Fr *wit_lag;   // [4][B][n]  A, B, C, PI   Lagrange
        Fr *z_lag;     // [B][n]
        Fr *coef;      // [5][B][n]  Ac, Bc, Cc, PIc, Zc   (coefficient forms; Z last so rounds 1 and 2 fill it in order)
        Fr *big;       // [5][B][3][n] A, B, C, PI, Z on the three cosets
        Fr *quot;      // [B][4n]    quotient evaluations on the three cosets, then its 3n coefficients (in place; the last n unused)
        Fr *num;       // [B][n]     round 2: the grand product's numerator factors (the denominators' go to wz); round 5: W_z's numerator
        uint32_t* closes;  // [2][B]  [0]: Z closes to 1 (round 2); [1]: a gate row fails (gate_check_kernel)
        Fr *wz;        // [2][B][n]  W_z, W_zw coefficient forms
        struct LinWeights* lin_w;  // [B]   round-5 linearisation weights
        struct BlindState* blind;  // [B]   the blinders and the tails they give (prover_blind.h); unused without PLONK_PROVER_BLINDING
        // the segmented scans (prover_scans.h): carries and partial sums of the S segments of every proof, none while S = 1
        Fr* seg;                   // [scan_scratch_elems(B, S)]
        size_t seg_cap;            // elements
    } rounds;
    // ---- wiring (plonk_prover_set_wiring): the wire cells are scattered from per-variable values on the device
    struct Wiring {
        uint32_t* cell_index;      // [K][3][n]  variable index of each wire cell; n_vars = empty cell / padding row
        uint32_t* pub_index;       // [K][n_public]  n_vars = a padding entry of a circuit with fewer public inputs: the value 0
        uint32_t* cell_host;       // [K][3][n] host copy of cell_index (what plonk_prover_set_inputs plans from: K = 1 only)
        size_t n_vars;
    } wiring;
    // ---- intake and staging (prover_intake.h): the batch that is resident, and how its bytes came in
    struct Intake {
        size_t resident_b;         // batch size of the witnesses currently resident (run / download must match it)
        size_t cap_b;              // proofs that rounds.wit_lag and pub hold: rounds.cap_b, until an advance brings the other slot's buffers in
        Fr* pub;                   // [B][n_public]   public inputs of the resident batch (Montgomery); a per-batch buffer
        Staging vars;              // [B][n_vars] values of the resident batch (Montgomery); cap in elements; read by the gathers
        Staging inputs;            // [B][n_inputs] the uploaded input values (canonical, as copied); cap in proofs; read by the seed
        bool vars_valid;           // `vars` holds the resident batch (not after plonk_prover_upload_witness)
        hipEvent_t ev_copied;      // async upload: the copy stream's H2D is done
        unsigned long long* bad_input;  // device: index of the first uploaded value that was not below r, or ~0 (PROVER_ST_BAD_INPUT)
        size_t bad_stride;         // values per proof of the last upload that ran the checked conversion: *bad_input / bad_stride owns the bad value
    } intake;
    // ---- the circuit of every proof (plonk_prover_set_labels): part of the resident batch, taken by the upload that follows the call
    struct Labels {
        uint32_t* pending;         // [pending_batch] host: the labels of the NEXT upload
        size_t pending_batch;      // 0: none pending
        uint32_t* host;            // [resident_b] host: the resident batch's (zeros where a K = 1 prover was given none); the verifier's load reads it
        uint32_t* dev;             // [cap] device: what the kernels index the circuit table with (K > 1 only)
        size_t cap, host_cap;
        hipEvent_t copied;         // behind the copy host -> dev on the compute stream: `host` is not rewritten before it
        bool copy_pending;
    } labels;
    StagedSlot staged;             // the batch behind the resident one (plonk_prover_stage_*, plonk_prover_advance)
    // ---- the witness solver (witness_solve.h; plonk_prover_set_inputs, plonk_prover_upload_inputs)
    struct Solver {
        uint8_t* gates_host;       // [5][n] canonical LE: QM, QL, QR, QO, QC as plonk_prover_create was given them
        uint32_t* desc;            // [rows] one descriptor per row (device)
        uint32_t rows;             // rows the solver walks: up to the last one that is not skipped
        // the levelised form's schedule (SolvePlan): built, freed and dropped with desc
        uint32_t* order;           // [active] the rows that are not skipped, sorted by level (device)
        uint32_t* level_start;     // [levels + 1] (device)
        uint32_t active, levels, widest, threads, steps;
        uint32_t* input_index;     // [n_inputs] the input variables (device)
        size_t n_inputs;           // 0: no plan (plonk_prover_set_inputs has not been called since the wiring was set)
        uint32_t* bad;             // [B] 0, or 1 + the first row whose check failed (capacity: intake.inputs.cap proofs)
        bool valid;                // the resident batch came through the solver: `bad` belongs to it
    } solver;
    // ---- blinding (prover_blind.h): where a run's blinders come from.  They belong to a RUN, not to an intake slot
    struct Blinding {
        struct G1Affine* htab;     // [6][16] 2^(16 w) ([tau^(n+k)] - [tau^k]); built when the option is switched on
        Fr* explicit_b;            // [explicit_cap][11] plonk_prover_set_blinders (Montgomery, device)
        size_t explicit_cap;       // proofs explicit_b holds
        size_t explicit_batch;     // batch the pending explicit blinders were set for, 0: none pending
        bool seeded;               // plonk_prover_seed_blinders has been called
        uint8_t seed[32];
        unsigned long long runs;   // blinded runs since the seed was set
    } blinding_src;
    // ---- results: per-batch buffers like the rounds'
    struct Results {
        Fq *commit_xy; // [9][B] x||y canonical
        uint8_t* commit_flags;  // [9][B]
        ProofState* state;      // [B]
    } results;
};
static_assert(std::is_trivially_copyable<plonk_prover>::value, "plonk_prover_create zero-fills it with memset: no constructor, no default member initialiser");
