// msm_tables.h — the tables of the table MSMs (msm_windows.h, msm_comb.h): the process-wide registry, and the policy that
// picks a table for a budget.  Both reach a layout only through its MsmTableLayout.
#pragma once
#include <algorithm>
#include <chrono>
#include <mutex>

#include "msm_comb.h"
#include "msm_windows.h"

static const MsmTableLayout& msm_layout(unsigned kind) { return kind == MSM_TABLE_COMB ? msm_comb_layout : msm_windows_layout; }

// Registry: one table per (process, device, base set, layout, bits), shared by every plonk_srs that
// was loaded from the same bytes — several contexts / streams / BatchProvers of one GPU use ONE table.
// srs->shared is written under g_lut_mu (and read without it by the launch path of the thread that owns the SRS).
static std::mutex g_lut_mu;
static std::vector<MsmLookupTable*> g_luts;

static void lut_attach(plonk_srs* srs, MsmLookupTable* t) {  // g_lut_mu held
    if (srs->shared == t) return;
    if (srs->shared && --srs->shared->refs == 0) {
        for (size_t k = 0; k < g_luts.size(); k++)
            if (g_luts[k] == srs->shared) g_luts.erase(g_luts.begin() + k);
        hipFree(srs->shared->data);
        hipFree(srs->shared->base_skip);
        delete srs->shared;
    }
    srs->shared = t;
    if (t) t->refs++;
}

// builds, registers and attaches the table of `bits` (nothing changed if the build fails)
static int lut_build(plonk_ctx* ctx, plonk_srs* srs, unsigned kind, unsigned bits, bool top) {  // g_lut_mu held
    const auto t0 = std::chrono::steady_clock::now();
    MsmLookupTable* t = new MsmLookupTable();
    const int rc = msm_layout(kind).build(ctx, srs, bits, top, t);
    if (rc != PLONK_OK) {
        delete t;
        return rc;
    }
    t->device = srs->device;
    t->key = srs->content_key;
    t->n_points = srs->n_points;
    t->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    g_luts.push_back(t);
    lut_attach(srs, t);
    return PLONK_OK;
}

// The registry key is a 64-bit FNV-1a of the loaded bytes — not collision resistant — so a candidate (same device, key,
// number of bases and bits: lut_find_verified) is only attached after its registered shape was found to be what this call
// would build and its entries were compared with THIS SRS's bases on the device (the layout's verify).  Every entry not
// compared is a function of (bases, number of bases, bits) alone, computed by this library when the table was registered.
static MsmLookupTable* lut_verified(plonk_ctx* ctx, const plonk_srs* srs, MsmLookupTable* t) {  // g_lut_mu held
    if (!t || t->n_points != srs->n_points || !msm_layout(t->kind).well_formed(t)) return nullptr;
    void* flag;
    if (ctx_scratch(ctx, 3, 64, &flag) != PLONK_OK) return nullptr;
    unsigned bad = 1;
    if (hipMemsetAsync(flag, 0, 4, ctx->stream) != hipSuccess) return nullptr;
    msm_layout(t->kind).verify(ctx, srs, t, (unsigned*)flag);
    if (hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
    return bad ? nullptr : t;
}
// the registered table of this base set with `bits` window bits (0: the one with the most) that passes the comparison above;
// several tables may sit under one key (a collision, or several window sizes): every candidate is tried, widest first
// (top: 0 = without top tables, 1 = with, -1 = either)
static MsmLookupTable* lut_find_verified(plonk_ctx* ctx, const plonk_srs* srs, unsigned kind, unsigned bits, int top = -1) {  // g_lut_mu held
    std::vector<MsmLookupTable*> cand;
    for (MsmLookupTable* t : g_luts)
        if (t->device == srs->device && t->key == srs->content_key && t->n_points == srs->n_points && t->kind == kind && (!bits || t->bits == bits) &&
            (top < 0 || (t->top_g != 0) == (top != 0)))
            cand.push_back(t);
    std::sort(cand.begin(), cand.end(), [](const MsmLookupTable* a, const MsmLookupTable* b) { return a->bits > b->bits; });
    for (MsmLookupTable* t : cand)
        if (lut_verified(ctx, srs, t)) return t;
    return nullptr;
}
// A Lagrange-basis view is a base set of its own with a table of its own: the automatic choice charges the tables of its
// parent SRS and of the parent's other views against the same budget, so that what the caller granted is not spent twice.
static size_t lut_bytes_of_family(const plonk_srs* srs) {  // g_lut_mu held
    const plonk_srs* root = srs->parent ? srs->parent : srs;
    size_t total = 0;
    if (root != srs && root->shared) total += root->shared->bytes;
    for (const auto& kv : root->lagrange)
        if (kv.second != srs && kv.second->shared) total += kv.second->shared->bytes;
    return total;
}


void msm_srs_release(plonk_srs* srs) {
    std::lock_guard<std::mutex> lk(g_lut_mu);
    lut_attach(srs, nullptr);
}

int msm_lookup_info(const plonk_srs* srs, unsigned* bits, size_t* bytes, double* build_s, int* sharers) {
    std::lock_guard<std::mutex> lk(g_lut_mu);
    const MsmLookupTable* t = srs->shared;
    *bits = t ? t->bits : 0;
    *bytes = t ? t->bytes : 0;
    *build_s = t ? t->build_s : 0;
    *sharers = t ? t->refs : 0;
    return PLONK_OK;
}

int msm_lookup_layout(const plonk_srs* srs, unsigned* kind, unsigned* additions_per_base) {
    std::lock_guard<std::mutex> lk(g_lut_mu);
    const MsmLookupTable* t = srs->shared;
    *kind = t ? t->kind : 0;
    *additions_per_base = t ? t->windows : 0;
    return PLONK_OK;
}

int msm_lookup_top(const plonk_srs* srs, unsigned* top_bits, unsigned* bases_per_group) {
    std::lock_guard<std::mutex> lk(g_lut_mu);
    const MsmLookupTable* t = srs->shared;
    *top_bits = t ? t->top_bits : 0;
    *bases_per_group = t ? t->top_g : 0;
    return PLONK_OK;
}

static size_t msm_default_table_budget() {
    // The table is a memory-for-time trade the CALLER opts into beyond a modest default: 1/16 of the device's memory (18 GB of an
    // MI355X's 288: the comb of 17 teeth for 2^11 bases, 8.6 GB + 1.1 GB while it is built, 15 additions per base) and never more
    // than a quarter of what is FREE at the moment — the default is per process and per SRS family, so several processes or
    // several SRS on one device each take theirs (eight ranks sharing a GPU: 8 x 9.7 GB), and a device that is already
    // nearly full must not be pushed over by a table nobody asked for.  More only through plonk_msm_lookup_configure(budget)
    // or PLONK_MSM_TABLE_GB (bench.py asks for 180 GB: the 157.6 GB comb of 21 teeth with top tables, 12.15 additions; 100 GB buys
    // the 68.7 GB comb of 20 teeth, 13 additions).
    // Window tables, measured (profiles/r05_d_msm_sweep.jsonl, 1152 MSMs of 2^11 per call): c = 11 4.50 ms, 12 4.11, 13 3.86, 14 3.65.
    const char* e = getenv("PLONK_MSM_TABLE_GB");
    if (e && atof(e) > 0) return (size_t)(atof(e) * 1e9);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !total_b) {
        (void)hipGetLastError();
        return (size_t)4 << 30;
    }
    return total_b / 16 < free_b / 4 ? total_b / 16 : free_b / 4;
}

// Decides whether this call runs on a table (then srs->shared): attaches the table another context of this device already
// built for the same bases, or builds one on first use.
static bool msm_table_prepare(plonk_ctx* ctx, plonk_srs* srs) {
    if (ctx->msm_lookup_mode == 1) return false;
    const unsigned want = ctx->msm_lookup_bits, kind = ctx->msm_lookup_kind;
    const MsmTableLayout& layout = msm_layout(kind);
    const bool wtop = want && ctx->msm_lookup_top;  // an explicit size names its variant (plonk_msm_lookup_configure grants `top` to combs only)
    std::lock_guard<std::mutex> lk(g_lut_mu);
    const auto attached_is = [&](unsigned bits) { return srs->shared && srs->shared->kind == kind && srs->shared->bits == bits && (srs->shared->top_g != 0) == wtop; };
    if (ctx->msm_lookup_mode == 2) {  // forced size, any base set
        if (attached_is(want)) return true;
        if (MsmLookupTable* t = lut_find_verified(ctx, srs, kind, want, wtop)) {
            lut_attach(srs, t);
            return true;
        }
        return lut_build(ctx, srs, kind, want, wtop) == PLONK_OK;
    }
    if (!srs->fixed) return false;
    if (srs->shared && srs->shared->kind == kind && (!want || attached_is(want))) return true;
    if (want) {
        if (MsmLookupTable* t = lut_find_verified(ctx, srs, kind, want, wtop)) {
            lut_attach(srs, t);
            return true;
        }
    }
    if (srs->lookup_failed) return false;
    const size_t budget = ctx->msm_lookup_budget ? ctx->msm_lookup_budget : msm_default_table_budget();
    // A table another context of this device already built for these bases is taken as it is — unless this context's
    // budget affords a better one (fewer additions per base), which is then built and shared in its turn.
    MsmLookupTable* have = want ? nullptr : lut_find_verified(ctx, srs, kind, 0);
    // The automatic choice charges the tables of the same SRS family (an SRS and its Lagrange-basis views) against one
    // budget.  An explicit size (`want`) is an explicit request and only has to fit the budget by itself.
    const size_t used = want ? 0 : lut_bytes_of_family(srs);
    // below 8 bits the table no longer beats the bucket method — which, however, cannot index more than 2^15 bases, so
    // larger base sets accept any table that fits
    const unsigned c_min = want ? want : (srs->n_points > 32768 ? 4 : 8);
    const unsigned c_max = want ? want : layout.auto_max_bits;
    // Candidates in the order of their additions per base, the smaller table first among equals (a comb one tooth shorter with
    // as many columns costs the same additions for half the memory).  Combs come without and — where 254 mod teeth allows — with
    // top tables (msm_comb.h): 21 teeth + top tables = 12.15 additions per base of 2^11 from 157.5 GB, between the 13 of 20 teeth
    // (68.7 GB) and the 12 of 22 (275 GB).
    struct Cand { unsigned c; bool top; double adds; size_t bytes; };
    std::vector<Cand> cands;
    for (unsigned c = c_max; c >= c_min; c--)
        for (int top = 0; top < 2; top++) {
            if (top && !layout.takes_top(srs->n_points, c)) continue;
            if (want && (top != 0) != wtop) continue;
            cands.push_back(Cand{c, top != 0, layout.additions(c, top != 0), layout.bytes(srs->n_points, c, top != 0)});
        }
    std::sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) { return x.adds != y.adds ? x.adds < y.adds : x.bytes < y.bytes; });
    const double have_adds = have ? layout.additions(have->bits, have->top_g != 0) : 1e9;
    for (const Cand& k : cands) {
        if (k.adds >= have_adds) break;
        if (k.bytes + used > budget) continue;
        if (lut_build(ctx, srs, kind, k.c, k.top) == PLONK_OK) return true;
    }
    if (have) {
        lut_attach(srs, have);
        return true;
    }
    srs->lookup_failed = true;
    return false;
}
