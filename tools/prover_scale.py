#!/usr/bin/env python3
"""The lock-step prover from 2^12 to 2^16 rows at small batches, and the evidence behind prover_plan_segments (csrc/prover_scans.h).

  --mode grid    n = 2^12 .. 2^16 x B in {1, 8, 64}: milliseconds per plonk_prover_run (median, min, max of 5 after a warm-up, HIP
                 events on the prover's stream), proofs/s, and the three per-proof scan families' own times (plonk_profile_*:
                 prover_grand_product, prover_evaluations, prover_divisions) for every S = 1, 2, 4, ... 256 the size admits and for
                 the automatic rule; the clock sampled over the whole grid (rocm-smi, tools/bench_legs.py).  Every cell says which
                 forced S was fastest, what the rule chose, and whether the rule's choice loses to S = 1 beyond the min-max spread.
  --mode gp      plonk_fr_grand_product alone at 2^14 and 2^16 (B = 1): the call Prover.round_2 makes.  Runs on any tree that has
                 the entry point (--tree: the package to import), which is how the parent commit's baseline is taken.
  --mode merge   joins the JSON files of the runs above (and bench.py's lines) into profiles/prover_large.json.

The chain circuit (x0 public, x_{i+1} = x_i^2) on an SRS of powers of oracle.srs.TEST_TAU made by plonk_g1_mul_many."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TEST_TAU = 314159265358979323846264338327950288419716939937510582097494459230781640628
G1 = (1, 2)
REPEATS = 5


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def device_tau_setup(pa, n_powers):
    from plonkathon_amd._lib import check
    from plonkathon_amd.field import Fq

    ctx = pa.get_context()
    scalars, t = bytearray(32 * n_powers), 1
    for i in range(n_powers):
        scalars[32 * i:32 * i + 32] = t.to_bytes(32, "little")
        t = t * TEST_TAU % R_MOD
    base = G1[0].to_bytes(32, "little") + G1[1].to_bytes(32, "little")
    out, ident = ctypes.create_string_buffer(64 * n_powers), ctypes.create_string_buffer(n_powers)
    check(ctx.L.plonk_g1_mul_many(ctx.handle, base * n_powers, bytes(scalars), n_powers, out, ident))
    raw = out.raw
    pts = [(Fq(int.from_bytes(raw[64 * i:64 * i + 32], "little")), Fq(int.from_bytes(raw[64 * i + 32:64 * i + 64], "little"))) for i in range(n_powers)]
    g2 = pa.kzg.G2  # the prover never reads X2
    return pa.Setup(powers_of_x=pts, X2=g2)


def chain_lines(n):
    return ["x0 public"] + ["x%d <== x%d * x%d" % (i + 1, i, i) for i in range(n - 1)]


def time_runs(ctx, bp, B):
    ms = []
    for _ in range(REPEATS):
        ctx.timer_start()
        bp.run(B)
        ms.append(ctx.timer_stop_ms())
    return ms


def family_times(ctx, bp, B):
    ctx.profile_reset()
    ctx.profile(True)
    bp.run(B)
    ctx.sync()
    ctx.profile(False)
    return {k: round(ctx.profile_read("prover_" + k)[0], 4) for k in ("grand_product", "evaluations", "divisions")}


def grid(args):
    import plonkathon_amd as pa
    from plonkathon_amd._lib import check
    from plonkathon_amd.batch import _pack_witnesses

    sys.path.insert(0, HERE)
    from bench_legs import ClockSampler

    ctx = pa.get_context()
    sampler = ClockSampler(0)
    sampler.start()
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    cells = []
    for log_n in args.log_ns or range(12, 17):
        n = 1 << log_n
        setup = device_tau_setup(pa, n)
        program = pa.Program(chain_lines(n), n)
        bp = pa.BatchProver(setup, program)
        wits = [program.fill_variable_assignments({"x0": 3 + i}) for i in range(8)]
        blob = _pack_witnesses(wits, bp.variables, R_MOD)
        per = len(blob) // 8
        for B in (1, 8, 64):
            check(ctx.L.plonk_mem_info(ctx.handle, ctypes.byref(free), ctypes.byref(total)))
            if 32 * 32 * n * B * 2 > free.value:
                cells.append({"log_n": log_n, "batch": B, "skipped": "needs %d bytes, %d free" % (32 * 32 * n * B, free.value)})
                continue
            bp.upload_values(b"".join(blob[per * (i % 8):per * (i % 8 + 1)] for i in range(B)), B)
            auto = bp.segments_for(B)
            rows, reference = [], None
            forced = [1 << k for k in range(9) if n >> k >= 16]
            for S in [None] + forced:
                check(ctx.L.plonk_prover_set_options(bp._h, 0 if S is None else (S.bit_length() << 8)))
                bp.run(B)  # warm-up (and the tables of the first commitment)
                out = bp.download_raw(B)
                reference = reference or out
                assert out == reference and out[1] == bytes(B), (log_n, B, S)
                ms = time_runs(ctx, bp, B)
                row = {"segments": auto if S is None else S, "automatic": S is None}
                row.update(spread(ms))
                row["proofs_per_s"] = round(1000.0 * B / row["median_ms"], 2)
                row["scan_ms"] = family_times(ctx, bp, B)
                row["scan_ms_total"] = round(sum(row["scan_ms"].values()), 4)
                rows.append(row)
            check(ctx.L.plonk_prover_set_options(bp._h, 0))
            one = next(r for r in rows if not r["automatic"] and r["segments"] == 1)
            best = min((r for r in rows if not r["automatic"]), key=lambda r: r["median_ms"])
            chosen = rows[0]
            cells.append({"log_n": log_n, "batch": B, "automatic_segments": auto, "fastest_forced_segments": best["segments"],
                          "automatic_vs_one_ms": round(chosen["median_ms"] - one["median_ms"], 4),
                          "automatic_loses_beyond_spread": chosen["min_ms"] > one["max_ms"], "runs": rows})
            print(json.dumps({k: v for k, v in cells[-1].items() if k != "runs"}), flush=True)
        del bp
    out = {"device": ctx.name(), "repeats": REPEATS, "timing": "HIP events around plonk_prover_run on the prover's stream, after one warm-up run",
           "scan_ms": "plonk_profile_read of prover_grand_product / prover_evaluations / prover_divisions over one further run",
           "clocks": sampler.summary(), "cells": cells}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def grand_product(args):
    import random

    import plonkathon_amd as pa
    from plonkathon_amd._lib import check
    from plonkathon_amd.field import le32

    ctx = pa.get_context()
    res = {"device": ctx.name(), "tree": os.path.abspath(args.tree), "repeats": REPEATS,
           "timing": "host clock around plonk_fr_grand_product (it waits for its closes flag), after one warm-up call", "sizes": {}}
    for log_n in args.log_ns or (14, 16):
        n = 1 << log_n
        rng = random.Random(log_n)
        dev = [ctx.upload_ints([rng.randrange(R_MOD) for _ in range(n)]) for _ in range(6)]
        beta, gamma = rng.randrange(R_MOD), rng.randrange(R_MOD)
        out, closes = ctx.alloc(n), ctypes.c_int(-1)
        call = lambda: check(ctx.L.plonk_fr_grand_product(ctx.handle, *[d.ptr for d in dev], log_n, le32(beta), le32(gamma), out.ptr, ctypes.byref(closes)))
        call()
        ctx.sync()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ms.append(1000.0 * (time.perf_counter() - t0))
        row = spread(ms)
        if hasattr(ctx.L, "plonk_prover_plan_segments"):
            S = ctypes.c_uint(0)
            check(ctx.L.plonk_prover_plan_segments(ctx.handle, log_n, 1, ctypes.byref(S)))
            row["segments"] = S.value
        import hashlib

        row["z_sha256_16"] = hashlib.sha256(b"".join(x.to_bytes(32, "little") for x in ctx.download_ints(out))).hexdigest()[:16]
        res["sizes"]["2^%d" % log_n] = row
        print(log_n, row, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def merge(args):
    def bench_line(path):
        with open(path) as f:
            for line in reversed(f.read().splitlines()):
                if line.startswith("{"):
                    d = json.loads(line)
                    return {k: d[k] for k in ("metric", "value", "unit", "steps", "warmup") if k in d}
        return None

    out = json.load(open(args.grid)) if args.grid else {}
    out["grand_product_alone"] = {"this_tree": json.load(open(args.gp_new)), "parent_commit": json.load(open(args.gp_parent))}
    out["bench_py"] = {"this_tree": [bench_line(p) for p in args.bench_new], "parent_commit": [bench_line(p) for p in args.bench_parent]}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("grid", "gp", "merge"), default="grid")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="the checkout whose plonkathon_amd is imported")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "prover_large.json"))
    ap.add_argument("--log-ns", type=int, nargs="*", help="group orders (log2) instead of the default grid")
    ap.add_argument("--grid")
    ap.add_argument("--gp-new")
    ap.add_argument("--gp-parent")
    ap.add_argument("--bench-new", nargs="*", default=[])
    ap.add_argument("--bench-parent", nargs="*", default=[])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    {"grid": grid, "gp": grand_product, "merge": merge}[a.mode](a)
