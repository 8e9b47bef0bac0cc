// prim_probe.hip — TEST INFRASTRUCTURE ONLY.  Not linked into libplonk_hip.so and never loaded by the plonkathon_amd package.
//
// Array probes of the field, curve and wave primitives under every kernel (csrc/fp.h, fpl.h, g1.h, wave.h): small kernels that
// run ONE CASE PER LANE, so that the operands the host unit tests were written for (limbs at +-(2^29 - 1), |a||b| near 128 m^2,
// a negated y whose low 29 bits are zero, equal and opposite points inside a running sum) meet the code hipcc emits for gfx950
// — v_mad_i64_i32, the FPL_ANY_SIGN / PLONK_CHAIN register constraints, the readfirstlane of a uniform operand, and the DPP /
// ds_swizzle / v_permlane exchanges of wave.h — and not only g++'s.  The same file builds two ways (tests/probe/Makefile):
//   hipcc --offload-arch=gfx950, the product's flags  -> libprim_probe_hip.so   (tests/test_gpu_primitives.py, on an MI355X)
//   g++ -DPLONK_EMU with tests/emu/hip_emu.cpp        -> libprim_probe_emu.so   (tests/test_emu_primitive_arrays.py; the range
//                                                                                 checks of fpl.h, FPL_CHECK, stay on)
// The cases and their checks against Python integers are in tests/primitive_cases.py.
//
// Every entry point takes host arrays of n cases, allocates, copies, launches workgroups of 64 lanes (the last one partial when
// n is no multiple of 64), synchronises, copies back, frees, and returns the HIP status (0 = success).  The operation is a kernel
// argument, uniform as in the product; the operands differ per lane.  Words are uint32 little-endian (8 per field element,
// Montgomery form unless said otherwise), limbs int32 (9 per element), points affine = 16 words ((0, 0) = identity),
// XYZZ = 32 words (zz = 0: identity), a lazy XYZZ = 37 int32 (x, y, zz, zzz limbs and the identity flag).
#include "fp.h"
#include "g1.h"
#include "wave.h"
#include "bls12_381_constants.h"

#define PROBE_TRY(x)                          \
    do {                                      \
        const hipError_t e_ = (x);            \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

namespace {
struct DevBuf {  // (never named among a launch's arguments: the emulator's launch copies those into a closure)
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T> T* as() const { return (T*)p; }
};
// device copy of a host array (zeroes when h is null: an output)
int probe_up(DevBuf& b, const void* h, size_t bytes) {
    PROBE_TRY(hipMalloc(&b.p, bytes ? bytes : 16));
    if (!bytes) return 0;
    if (h) PROBE_TRY(hipMemcpy(b.p, h, bytes, hipMemcpyHostToDevice));
    else PROBE_TRY(hipMemset(b.p, 0, bytes));
    return 0;
}
int probe_down(void* h, const DevBuf& b, size_t bytes) {
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    if (bytes) PROBE_TRY(hipMemcpy(h, b.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
dim3 probe_grid(int n) { return dim3((unsigned)((n + 63) / 64)); }
}  // namespace

template <class P> PLONK_HD Fp<P> probe_ld(const uint32_t* w) {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
template <class P> PLONK_HD void probe_st(uint32_t* w, const Fp<P>& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
template <class P> PLONK_HD FpL<P> probe_ldl(const int32_t* w) {
    FpL<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = w[i];
    return r;
}
template <class P> PLONK_HD void probe_stl(int32_t* w, const FpL<P>& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = a.l[i];
}
PLONK_HD G1Affine probe_ld_affine(const uint32_t* w) {
    G1Affine r;
    r.x = probe_ld<FqParams>(w);
    r.y = probe_ld<FqParams>(w + 8);
    return r;
}
PLONK_HD void probe_st_affine(uint32_t* w, const G1Affine& a) {
    probe_st(w, a.x);
    probe_st(w + 8, a.y);
}
PLONK_HD G1Xyzz probe_ld_xyzz(const uint32_t* w) {
    G1Xyzz r;
    r.x = probe_ld<FqParams>(w);
    r.y = probe_ld<FqParams>(w + 8);
    r.zz = probe_ld<FqParams>(w + 16);
    r.zzz = probe_ld<FqParams>(w + 24);
    return r;
}
PLONK_HD void probe_st_xyzz(uint32_t* w, const G1Xyzz& a) {
    probe_st(w, a.x);
    probe_st(w + 8, a.y);
    probe_st(w + 16, a.zz);
    probe_st(w + 24, a.zzz);
}
PLONK_HD void probe_st_lazy(int32_t* w, const G1XyzzL& a) {
    probe_stl(w, a.x);
    probe_stl(w + 9, a.y);
    probe_stl(w + 18, a.zz);
    probe_stl(w + 27, a.zzz);
    w[36] = a.inf ? 1 : 0;
}
PLONK_HD bool probe_xyzz_same_words(const G1Xyzz& a, const G1Xyzz& b) {
    return fp_eq(a.x, b.x) && fp_eq(a.y, b.y) && fp_eq(a.zz, b.zz) && fp_eq(a.zzz, b.zzz);
}

// ---- packed field operations ------------------------------------------------------------------------------------------------
// op: 0 add, 1 sub, 2 mul, 3 inv (division steps), 4 to Montgomery, 5 from Montgomery, 6 neg, 7 sqr, 8 inv (Fermat)
template <class P> __global__ void probe_field_kernel(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    const Fp<P> x = probe_ld<P>(a + 8 * (size_t)t), y = probe_ld<P>(b + 8 * (size_t)t);
    Fp<P> r;
    switch (op) {
        case 0: r = fp_add(x, y); break;
        case 1: r = fp_sub(x, y); break;
        case 2: r = fp_mul(x, y); break;
        case 3: r = fp_inv(x); break;
        case 4: r = fp_to_mont(x); break;
        case 5: r = fp_from_mont(x); break;
        case 6: r = fp_neg(x); break;
        case 7: r = fp_sqr(x); break;
        case 8: r = fp_inv_fermat(x); break;
        default: r = fp_zero<P>();
    }
    probe_st(out + 8 * (size_t)t, r);
}

template <class P> static int probe_field_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
    DevBuf da, db, dout;
    const size_t bytes = (size_t)n * 32;
    if (int e = probe_up(da, a, bytes)) return e;
    if (int e = probe_up(db, b, bytes)) return e;
    if (int e = probe_up(dout, nullptr, bytes)) return e;
    const uint32_t* p_a = da.as<const uint32_t>();
    const uint32_t* p_b = db.as<const uint32_t>();
    uint32_t* p_out = dout.as<uint32_t>();
    if (n > 0)
        PLONK_LAUNCH(PLONK_KERNEL(probe_field_kernel<P>), probe_grid(n), dim3(64), 0, (hipStream_t)0, op, p_a, p_b,
                     p_out, n);
    return probe_down(out, dout, bytes);
}

// field: 0 = BN254 Fr, 1 = BN254 Fq, 2 = BLS12-381 Fr
extern "C" int probe_field(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
    if (n < 0 || op < 0 || op > 8) return (int)hipErrorInvalidValue;
    switch (field) {
        case 0: return probe_field_run<FrParams>(op, a, b, out, n);
        case 1: return probe_field_run<FqParams>(op, a, b, out, n);
        case 2: return probe_field_run<BlsFrParams>(op, a, b, out, n);
        default: return (int)hipErrorInvalidValue;
    }
}

// ---- raw signed limbs (Fq) --------------------------------------------------------------------------------------------------
// op: 0 mul(a, b), 1 sqr(a), 2 mul_add(a, b, c, d), 3 norm(a), 4 to_fp(a) (8 packed words in out[0..7]), 5 pack_lt4m<8>(a),
// 6 pack_lt4m<1>(a) (8 words each); out[8] = 0 for the packed forms
__global__ void probe_fpl_kernel(int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    const size_t o = 9 * (size_t)t;
    const FqL x = probe_ldl<FqParams>(a + o), y = probe_ldl<FqParams>(b + o), z = probe_ldl<FqParams>(c + o), w = probe_ldl<FqParams>(d + o);
    FqL r = fpl_zero<FqParams>();
    switch (op) {
        case 0: r = fpl_mul(x, y); break;
        case 1: r = fpl_sqr(x); break;
        case 2: r = fpl_mul_add(x, y, z, w); break;
        case 3: r = fpl_norm(x); break;
        case 4: {
            const Fq f = fpl_to_fp(x);
            for (int i = 0; i < 8; i++) r.l[i] = (int32_t)f.v[i];
            break;
        }
        case 5: {
            uint32_t p[8];
            fpl_pack_lt4m<8>(x, p);
            for (int i = 0; i < 8; i++) r.l[i] = (int32_t)p[i];
            break;
        }
        case 6: {
            uint32_t p[8];
            fpl_pack_lt4m<1>(x, p);
            for (int i = 0; i < 8; i++) r.l[i] = (int32_t)p[i];
            break;
        }
        default: break;
    }
    probe_stl(out + o, r);
}

extern "C" int probe_fpl(int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out, int n) {
    if (n < 0 || op < 0 || op > 6) return (int)hipErrorInvalidValue;
    DevBuf da, db, dc, dd, dout;
    const size_t bytes = (size_t)n * 36;
    if (int e = probe_up(da, a, bytes)) return e;
    if (int e = probe_up(db, b, bytes)) return e;
    if (int e = probe_up(dc, c, bytes)) return e;
    if (int e = probe_up(dd, d, bytes)) return e;
    if (int e = probe_up(dout, nullptr, bytes)) return e;
    const int32_t* p_a = da.as<const int32_t>();
    const int32_t* p_b = db.as<const int32_t>();
    const int32_t* p_c = dc.as<const int32_t>();
    const int32_t* p_d = dd.as<const int32_t>();
    int32_t* p_out = dout.as<int32_t>();
    if (n > 0)
        PLONK_LAUNCH(probe_fpl_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, op, p_a, p_b, p_c,
                     p_d, p_out, n);
    return probe_down(out, dout, bytes);
}

// limbs[9] of s ? -y : y (s = 0 or ~0, per lane) and (+-y) z / R through fpl_mul against the normalised z: the one product the
// signed limbs enter in the mixed addition (S2 = Y2 ZZZ1)
__global__ void probe_fpl_signed_kernel(const uint32_t* y, const uint32_t* s, const uint32_t* z, int32_t* limbs, uint32_t* prod, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    const Fq a = probe_ld<FqParams>(y + 8 * (size_t)t), b = probe_ld<FqParams>(z + 8 * (size_t)t);
    const FqL l = fpl_from_fp_signed(a, s[t]);
    probe_stl(limbs + 9 * (size_t)t, l);
    probe_st(prod + 8 * (size_t)t, fpl_to_fp(fpl_mul(l, fpl_from_fp(b))));
}

extern "C" int probe_fpl_signed(const uint32_t* y, const uint32_t* s, const uint32_t* z, int32_t* limbs, uint32_t* prod, int n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    DevBuf dy, ds, dz, dl, dp;
    if (int e = probe_up(dy, y, (size_t)n * 32)) return e;
    if (int e = probe_up(ds, s, (size_t)n * 4)) return e;
    if (int e = probe_up(dz, z, (size_t)n * 32)) return e;
    if (int e = probe_up(dl, nullptr, (size_t)n * 36)) return e;
    if (int e = probe_up(dp, nullptr, (size_t)n * 32)) return e;
    const uint32_t* p_y = dy.as<const uint32_t>();
    const uint32_t* p_s = ds.as<const uint32_t>();
    const uint32_t* p_z = dz.as<const uint32_t>();
    int32_t* p_l = dl.as<int32_t>();
    uint32_t* p_p = dp.as<uint32_t>();
    if (n > 0)
        PLONK_LAUNCH(probe_fpl_signed_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, p_y, p_s,
                     p_z, p_l, p_p, n);
    if (int e = probe_down(limbs, dl, (size_t)n * 36)) return e;
    return probe_down(prod, dp, (size_t)n * 32);
}

// out = a * u / R with u a KERNEL ARGUMENT unpacked by fpl_from_fp_uniform (on the device: scalar registers through
// readfirstlane) and a per lane, raw limbs
__global__ void probe_fpl_uniform_kernel(Fq u, const int32_t* a, int32_t* out, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    const FqL ul = fpl_from_fp_uniform(u);
    probe_stl(out + 9 * (size_t)t, fpl_mul(probe_ldl<FqParams>(a + 9 * (size_t)t), ul));
}

extern "C" int probe_fpl_uniform(const uint32_t* u, const int32_t* a, int32_t* out, int n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    DevBuf da, dout;
    if (int e = probe_up(da, a, (size_t)n * 36)) return e;
    if (int e = probe_up(dout, nullptr, (size_t)n * 36)) return e;
    const Fq uu = probe_ld<FqParams>(u);
    const int32_t* p_a = da.as<const int32_t>();
    int32_t* p_out = dout.as<int32_t>();
    if (n > 0) PLONK_LAUNCH(probe_fpl_uniform_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, uu, p_a, p_out, n);
    return probe_down(out, dout, (size_t)n * 36);
}

// fpl_shoup_from_mont + fpl_mul_shoup: a = 9 signed limbs, wt = a constant in canonical Montgomery form (8 words), both per lane;
// out[0..8] = a * w (limbs), out[9..17] = w, out[18..26] = wp = floor(w 2^261 / m)
template <class P> __global__ void probe_shoup_kernel(const int32_t* a, const uint32_t* wt, int32_t* out, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    uint32_t ninv[9];
    fpl_ninv261<P>(ninv);
    const FpLS<P> s = fpl_shoup_from_mont(probe_ld<P>(wt + 8 * (size_t)t), ninv);
    const FpL<P> r = fpl_mul_shoup(probe_ldl<P>(a + 9 * (size_t)t), s);
    int32_t* o = out + 27 * (size_t)t;
    probe_stl(o, r);
    for (int i = 0; i < 9; i++) {
        o[9 + i] = s.w[i];
        o[18 + i] = s.wp[i];
    }
}

// field: 0 = BN254 Fr, 2 = BLS12-381 Fr
extern "C" int probe_fpl_shoup(int field, const int32_t* a, const uint32_t* wt, int32_t* out, int n) {
    if (n < 0 || (field != 0 && field != 2)) return (int)hipErrorInvalidValue;
    DevBuf da, dw, dout;
    if (int e = probe_up(da, a, (size_t)n * 36)) return e;
    if (int e = probe_up(dw, wt, (size_t)n * 32)) return e;
    if (int e = probe_up(dout, nullptr, (size_t)n * 108)) return e;
    const int32_t* p_a = da.as<const int32_t>();
    const uint32_t* p_w = dw.as<const uint32_t>();
    int32_t* p_out = dout.as<int32_t>();
    if (n > 0) {
        if (field == 0) PLONK_LAUNCH(PLONK_KERNEL(probe_shoup_kernel<FrParams>), probe_grid(n), dim3(64), 0, (hipStream_t)0, p_a, p_w, p_out, n);
        else PLONK_LAUNCH(PLONK_KERNEL(probe_shoup_kernel<BlsFrParams>), probe_grid(n), dim3(64), 0, (hipStream_t)0, p_a, p_w, p_out, n);
    }
    return probe_down(out, dout, (size_t)n * 108);
}

// ---- curve: packed formulas ---------------------------------------------------------------------------------------------------
// the five operations of tests/emu/fp_probe.cpp's probe_g1 on affine pairs (p, q): 0 = p + q by the mixed addition, 1 = p + q by
// the full addition, 2 = 2p, 3 = 2p + q (mixed, non-trivial ZZ), 4 = 2p + 2q (full, both ZZ non-trivial); affine out
__global__ void probe_g1_kernel(int op, const uint32_t* p, const uint32_t* q, uint32_t* out, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    const G1Affine a = probe_ld_affine(p + 16 * (size_t)t), b = probe_ld_affine(q + 16 * (size_t)t);
    G1Xyzz acc = g1_xyzz_from_affine(a);
    switch (op) {
        case 0: g1_madd(acc, b); break;
        case 1: g1_add(acc, g1_xyzz_from_affine(b)); break;
        case 2: g1_dbl(acc); break;
        case 3:
            g1_dbl(acc);
            g1_madd(acc, b);
            break;
        case 4: {
            g1_dbl(acc);
            G1Xyzz o = g1_xyzz_from_affine(b);
            g1_dbl(o);
            g1_add(acc, o);
            break;
        }
        default: acc = g1_xyzz_identity();
    }
    probe_st_affine(out + 16 * (size_t)t, g1_to_affine(acc));
}

extern "C" int probe_g1(int op, const uint32_t* p, const uint32_t* q, uint32_t* out, int n) {
    if (n < 0 || op < 0 || op > 4) return (int)hipErrorInvalidValue;
    DevBuf dp, dq, dout;
    const size_t bytes = (size_t)n * 64;
    if (int e = probe_up(dp, p, bytes)) return e;
    if (int e = probe_up(dq, q, bytes)) return e;
    if (int e = probe_up(dout, nullptr, bytes)) return e;
    const uint32_t* p_p = dp.as<const uint32_t>();
    const uint32_t* p_q = dq.as<const uint32_t>();
    uint32_t* p_out = dout.as<uint32_t>();
    if (n > 0)
        PLONK_LAUNCH(probe_g1_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, op, p_p, p_q, p_out, n);
    return probe_down(out, dout, bytes);
}

// ---- curve: the lazy accumulator ----------------------------------------------------------------------------------------------
// Lane t folds its own list pts[start[t] .. start[t + 1]) of +- points into a lazy accumulator and, where the fast step returns
// false, takes the packed formulas exactly as probe_g1l_chain of tests/emu/fp_probe.cpp does.
//   signed_entry = 0: g1l_madd_fast(acc, x, y, neg) on every point, the identity included (which it refuses: a false return)
//   signed_entry = 1: g1l_madd_signed(acc, x, y, neg ? ~0 : 0), the comb loop's entry; an identity addend is passed over BEFORE
//                     the call, as the comb kernel passes it over by its digit (the entry has no zero test)
// out: the affine sum; info[0] = the number of false returns, info[1] = which piece routes agree word for word with the direct
// route g1l_to_xyzz(acc): bit 0 g1l_to_piece -> g1_piece_load, bit 1 g1l_to_piece_wide -> g1_piece_load, bit 2 g1l_to_piece ->
// g1l_from_piece -> g1l_to_xyzz, bit 3 g1l_to_piece_wide -> g1l_from_piece -> g1l_to_xyzz (15 = all)
__global__ void probe_g1l_chain_kernel(int signed_entry, const uint32_t* pts, const int32_t* neg, const int32_t* start, uint32_t* out, int32_t* info, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    G1XyzzL acc = g1l_identity();
    int refused = 0;
    for (int i = start[t]; i < start[t + 1]; i++) {
        G1Affine a = probe_ld_affine(pts + 16 * (size_t)i);
        const bool ng = neg[i] != 0;
        bool ok;
        if (signed_entry) {
            if (g1_affine_is_identity(a)) continue;
            ok = g1l_madd_signed(acc, a.x, a.y, ng ? 0xFFFFFFFFu : 0u);
        } else {
            ok = g1l_madd_fast(acc, a.x, a.y, ng);
        }
        if (!ok) {  // exceptional step: the general packed formulas
            refused++;
            if (ng) a.y = fp_neg(a.y);
            G1Xyzz s = g1l_to_xyzz(acc);
            g1_madd(s, a);
            acc = g1l_from_xyzz(s);
        }
    }
    const G1Xyzz direct = g1l_to_xyzz(acc);
    const G1Xyzz piece = g1l_to_piece(acc), wide = g1l_to_piece_wide(acc);
    int agree = 0;
    if (probe_xyzz_same_words(g1_piece_load(&piece), direct)) agree |= 1;
    if (probe_xyzz_same_words(g1_piece_load(&wide), direct)) agree |= 2;
    if (probe_xyzz_same_words(g1l_to_xyzz(g1l_from_piece(&piece)), direct)) agree |= 4;
    if (probe_xyzz_same_words(g1l_to_xyzz(g1l_from_piece(&wide)), direct)) agree |= 8;
    probe_st_affine(out + 16 * (size_t)t, g1_to_affine(direct));
    info[2 * (size_t)t] = refused;
    info[2 * (size_t)t + 1] = agree;
}

// start: n + 1 ascending offsets into pts / neg, start[0] = 0, start[n] = the number of points
extern "C" int probe_g1l_chain(int signed_entry, const uint32_t* pts, const int32_t* neg, const int32_t* start, uint32_t* out, int32_t* info, int n) {
    if (n < 0 || !start || start[0] != 0) return (int)hipErrorInvalidValue;
    for (int t = 0; t < n; t++)
        if (start[t + 1] < start[t]) return (int)hipErrorInvalidValue;
    const size_t np = (size_t)start[n];
    DevBuf dp, dn, ds, dout, di;
    if (int e = probe_up(dp, pts, np * 64)) return e;
    if (int e = probe_up(dn, neg, np * 4)) return e;
    if (int e = probe_up(ds, start, ((size_t)n + 1) * 4)) return e;
    if (int e = probe_up(dout, nullptr, (size_t)n * 64)) return e;
    if (int e = probe_up(di, nullptr, (size_t)n * 8)) return e;
    const uint32_t* p_p = dp.as<const uint32_t>();
    const int32_t* p_n = dn.as<const int32_t>();
    const int32_t* p_s = ds.as<const int32_t>();
    uint32_t* p_out = dout.as<uint32_t>();
    int32_t* p_i = di.as<int32_t>();
    if (n > 0)
        PLONK_LAUNCH(probe_g1l_chain_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, signed_entry != 0 ? 1 : 0, p_p, p_n,
                     p_s, p_out, p_i, n);
    if (int e = probe_down(out, dout, (size_t)n * 64)) return e;
    return probe_down(info, di, (size_t)n * 8);
}

// pairs of XYZZ points (canonical words, any ZZ) through the lazy general formulas: op 0 = g1l_add_fast<false>(p, q),
// 1 = g1l_add_fast<true>(p, q), 2 = g1l_dbl(p).  out: p afterwards as raw limbs (37 int32), ret: the return value (1 for op 2)
__global__ void probe_g1l_pair_kernel(int op, const uint32_t* p, const uint32_t* q, int32_t* out, int32_t* ret, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n) return;
    G1XyzzL a = g1l_from_xyzz(probe_ld_xyzz(p + 32 * (size_t)t));
    const G1XyzzL b = g1l_from_xyzz(probe_ld_xyzz(q + 32 * (size_t)t));
    bool ok = true;
    switch (op) {
        case 0: ok = g1l_add_fast<false>(a, b); break;
        case 1: ok = g1l_add_fast<true>(a, b); break;
        default: g1l_dbl(a);
    }
    probe_st_lazy(out + 37 * (size_t)t, a);
    ret[t] = ok ? 1 : 0;
}

extern "C" int probe_g1l_pair(int op, const uint32_t* p, const uint32_t* q, int32_t* out, int32_t* ret, int n) {
    if (n < 0 || op < 0 || op > 2) return (int)hipErrorInvalidValue;
    DevBuf dp, dq, dout, dr;
    if (int e = probe_up(dp, p, (size_t)n * 128)) return e;
    if (int e = probe_up(dq, q, (size_t)n * 128)) return e;
    if (int e = probe_up(dout, nullptr, (size_t)n * 148)) return e;
    if (int e = probe_up(dr, nullptr, (size_t)n * 4)) return e;
    const uint32_t* p_p = dp.as<const uint32_t>();
    const uint32_t* p_q = dq.as<const uint32_t>();
    int32_t* p_out = dout.as<int32_t>();
    int32_t* p_r = dr.as<int32_t>();
    if (n > 0)
        PLONK_LAUNCH(probe_g1l_pair_kernel, probe_grid(n), dim3(64), 0, (hipStream_t)0, op, p_p, p_q, p_out,
                     p_r, n);
    if (int e = probe_down(out, dout, (size_t)n * 148)) return e;
    return probe_down(ret, dr, (size_t)n * 4);
}

// ---- wave: one full wave of 64 lanes per launch -------------------------------------------------------------------------------
template <unsigned MASK> PLONK_DEV void probe_wave_words_case(int swap, int32_t& a, int32_t& b, unsigned lane) {
    if (swap) wave_swap_words<MASK>(a, b, (lane & MASK) != 0, lane);
    else a = (int32_t)wave_lane_xor<MASK>((uint32_t)a, lane);
}
// swap = 0: oa[lane] = wave_lane_xor<mask>(a[lane]) (ob = b); swap = 1: (oa, ob)[lane] = wave_swap_words<mask>(a[lane], b[lane])
__global__ void probe_wave_words_kernel(int swap, unsigned mask, const int32_t* a, const int32_t* b, int32_t* oa, int32_t* ob) {
    const unsigned lane = threadIdx.x;
    int32_t x = a[lane], y = b[lane];
    switch (mask) {  // (uniform: every lane of the wave takes the same exchange)
        case 1: probe_wave_words_case<1>(swap, x, y, lane); break;
        case 2: probe_wave_words_case<2>(swap, x, y, lane); break;
        case 4: probe_wave_words_case<4>(swap, x, y, lane); break;
        case 8: probe_wave_words_case<8>(swap, x, y, lane); break;
        case 16: probe_wave_words_case<16>(swap, x, y, lane); break;
        default: probe_wave_words_case<32>(swap, x, y, lane); break;
    }
    oa[lane] = x;
    ob[lane] = y;
}

static bool probe_mask_ok(unsigned mask) { return mask == 1 || mask == 2 || mask == 4 || mask == 8 || mask == 16 || mask == 32; }

extern "C" int probe_wave_words(int swap, unsigned mask, const int32_t* a, const int32_t* b, int32_t* oa, int32_t* ob) {
    if (!probe_mask_ok(mask)) return (int)hipErrorInvalidValue;
    DevBuf da, db, doa, dob;
    if (int e = probe_up(da, a, 256)) return e;
    if (int e = probe_up(db, b, 256)) return e;
    if (int e = probe_up(doa, nullptr, 256)) return e;
    if (int e = probe_up(dob, nullptr, 256)) return e;
    const int32_t* p_a = da.as<const int32_t>();
    const int32_t* p_b = db.as<const int32_t>();
    int32_t* p_oa = doa.as<int32_t>();
    int32_t* p_ob = dob.as<int32_t>();
    PLONK_LAUNCH(probe_wave_words_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, swap != 0 ? 1 : 0, mask, p_a, p_b,
                 p_oa, p_ob);
    if (int e = probe_down(oa, doa, 256)) return e;
    return probe_down(ob, dob, 256);
}

// op 0: g1_wave_reduce, op 1: g1_wave_suffix_scan, of one affine point per lane; XYZZ words out (32 per lane)
__global__ void probe_g1_wave_kernel(int op, const uint32_t* pts, uint32_t* out) {
    const unsigned lane = threadIdx.x;
    G1Xyzz p = g1_xyzz_from_affine(probe_ld_affine(pts + 16 * lane));
    if (op == 0) g1_wave_reduce(p, lane);
    else g1_wave_suffix_scan(p, lane);
    probe_st_xyzz(out + 32 * lane, p);
}

extern "C" int probe_g1_wave(int op, const uint32_t* pts, uint32_t* out) {
    if (op < 0 || op > 1) return (int)hipErrorInvalidValue;
    DevBuf dp, dout;
    if (int e = probe_up(dp, pts, 64 * 64)) return e;
    if (int e = probe_up(dout, nullptr, 64 * 128)) return e;
    const uint32_t* p_p = dp.as<const uint32_t>();
    uint32_t* p_out = dout.as<uint32_t>();
    PLONK_LAUNCH(probe_g1_wave_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, op, p_p, p_out);
    return probe_down(out, dout, 64 * 128);
}

// mask = 1 .. 32: one g1l_wave_reduce_step<mask> (OPPOSITE_OK = false) of one affine point per lane;
// mask = 0: the chain <1, true>, <2, true>, .. <32, true> with the returns and-ed, as msm_comb_finalize_kernel<64> runs it.
// out: the lane's accumulator afterwards as raw limbs (37 int32), ret: the (and-ed) return value
__global__ void probe_g1l_wave_kernel(unsigned mask, const uint32_t* pts, int32_t* out, int32_t* ret) {
    const unsigned lane = threadIdx.x;
    G1XyzzL p = g1l_from_xyzz(g1_xyzz_from_affine(probe_ld_affine(pts + 16 * lane)));
    bool ok = true;
    switch (mask) {
        case 1: ok = g1l_wave_reduce_step<1>(p, lane); break;
        case 2: ok = g1l_wave_reduce_step<2>(p, lane); break;
        case 4: ok = g1l_wave_reduce_step<4>(p, lane); break;
        case 8: ok = g1l_wave_reduce_step<8>(p, lane); break;
        case 16: ok = g1l_wave_reduce_step<16>(p, lane); break;
        case 32: ok = g1l_wave_reduce_step<32>(p, lane); break;
        default:
            ok &= g1l_wave_reduce_step<1, true>(p, lane);
            ok &= g1l_wave_reduce_step<2, true>(p, lane);
            ok &= g1l_wave_reduce_step<4, true>(p, lane);
            ok &= g1l_wave_reduce_step<8, true>(p, lane);
            ok &= g1l_wave_reduce_step<16, true>(p, lane);
            ok &= g1l_wave_reduce_step<32, true>(p, lane);
    }
    probe_st_lazy(out + 37 * lane, p);
    ret[lane] = ok ? 1 : 0;
}

extern "C" int probe_g1l_wave(unsigned mask, const uint32_t* pts, int32_t* out, int32_t* ret) {
    if (mask != 0 && !probe_mask_ok(mask)) return (int)hipErrorInvalidValue;
    DevBuf dp, dout, dr;
    if (int e = probe_up(dp, pts, 64 * 64)) return e;
    if (int e = probe_up(dout, nullptr, 64 * 148)) return e;
    if (int e = probe_up(dr, nullptr, 256)) return e;
    const uint32_t* p_p = dp.as<const uint32_t>();
    int32_t* p_out = dout.as<int32_t>();
    int32_t* p_r = dr.as<int32_t>();
    PLONK_LAUNCH(probe_g1l_wave_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, mask, p_p, p_out, p_r);
    if (int e = probe_down(out, dout, 64 * 148)) return e;
    return probe_down(ret, dr, 256);
}
