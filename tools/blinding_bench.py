#!/usr/bin/env python3
"""What zero-knowledge blinding (csrc/prover_blind.h, PLONK_PROVER_BLINDING) costs, and that the unblinded prover pays nothing for
it -> profiles/blinding.json, one session.

Shapes, every one blinded (under a seed), unblinded, and — with --parent-lib — unblinded on a build of the parent commit:
    step_2e10    bench.py's step on the 2^10 chain, golden SRS: 20 contexts x 512 proofs, witnesses resident
    batch_2e10   one lone batch of 512 on one context
    proof_2e10   one lone proof
    step_2e11    the same step on the 2^11 chain, on a from-tau SRS of 2^11 + 6 powers (the golden file's 2^11 are six too few)
The comb table of an SRS takes most of the device's memory, so a process holds ONE base set and ONE build: a worker process
(--worker) measures one (build, SRS) pair, its modes alternating inside a repeat, and this process alternates the workers —
this build, the parent's, this build, ... — `--rounds` times; a figure is the median and min-max over rounds x repeats.
There is no pass mark for the blinded cost.  The condition is on the other side: `unblinded` must be level with `parent` within the
spread of the repeats (the record says so per shape).
Per-kernel split of the blinded step: run the worker alone under a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/blinding_bench.py --worker --srs golden --modes blinded --shapes step
and pass the database it leaves with --trace-db."""
import argparse
import collections
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, HERE]
PTAU = os.path.join(REPO, "tests", "golden", "srs_2048.ptau")
NEW_SYMBOLS = ("plonk_prover_set_blinders", "plonk_prover_seed_blinders")
SEED = bytes(range(32))


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def worker(args):
    """One (build, SRS) pair: {shape: {mode: [ms per step, one per repeat]}} as a JSON line."""
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(min(20, max(4, args.streams))))  # as bench.py, before the HIP runtime loads
    from plonkathon_amd import _lib

    probe = ctypes.CDLL(_lib.LIB_PATH)
    has_blinding = all(hasattr(probe, s) for s in NEW_SYMBOLS)
    if not has_blinding:  # a build of the parent commit: the table of prototypes without the two entry points it lacks
        for s in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(s)
    import contextlib

    import plonkathon_amd as pa
    from bench import chain_program_lines

    modes = [m for m in args.modes.split(",") if m == "unblinded" or has_blinding]
    log_n = 10 if args.srs == "golden" else 11
    n, B, S = 1 << log_n, args.batch, args.streams
    ctxs = [pa.get_context()] + [pa.Context(0) for _ in range(S - 1)]
    knobs = contextlib.ExitStack()
    for c in ctxs:
        c.msm_lookup(0, 0, int(args.lookup_budget_gb * 1e9))
        if S >= 8:
            knobs.enter_context(c.tuning(msm_groups=1))  # bench.py's setting for eight or more streams
    if args.srs == "golden":
        setup = pa.Setup.from_file(PTAU)
    else:
        from prover_scale import device_tau_setup

        setup = device_tau_setup(pa, n + 6)
    program = pa.Program(chain_program_lines(n), n)
    wits = [program.fill_variable_assignments({"x0": 3 + b}) for b in range(B)]
    from plonkathon_amd.batch import _pack_witnesses
    from plonkathon_amd.field import R_MOD

    variables = tuple(program.wiring_table()[0])
    blob = _pack_witnesses(wits, variables, R_MOD)
    per = len(blob) // B
    shapes = {"step": (ctxs, B), "batch": (ctxs[:1], B), "proof": (ctxs[:1], 1)}
    out = {}
    for shape in args.shapes.split(","):
        use, b = shapes[shape]
        provers = {}
        for m in modes:
            kw = {"blinding": SEED} if m == "blinded" else {}
            provers[m] = [pa.BatchProver(setup, program, c, **kw) for c in use]
            for pr in provers[m]:
                pr.upload_values(blob[:per * b], b)

        def step(m):
            for pr in provers[m]:
                pr.run()
            for pr in provers[m]:
                raw, st = pr.download_raw()
                assert not any(st)

        def sync():
            for c in use:
                c.sync()

        for m in modes:
            for _ in range(max(1, args.warmup)):  # (the first step builds the MSM table)
                step(m)
        ms = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m in modes:  # alternating: a drift of the clock falls on all of them alike
                sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(m)
                sync()
                ms[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
        out["%s_2e%d" % (shape, log_n)] = ms
        del provers
    knobs.close()
    print("RESULT " + json.dumps({"device": ctxs[0].name(), "has_blinding": has_blinding, "ms": out,
                                  "table": setup.device_bases(ctxs[0]).lookup_info()}))


def run_worker(args, srs, lib, shapes):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--srs", srs, "--shapes", shapes, "--repeats", str(args.repeats), "--steps",
           str(args.steps), "--batch", str(args.batch), "--streams", str(args.streams), "--lookup-budget-gb", str(args.lookup_budget_gb)]
    env = dict(os.environ)
    if lib:
        env["PLONK_HIP_LIB"] = lib
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if done.returncode:
        raise SystemExit("worker failed (%d): %s\n%s" % (done.returncode, " ".join(cmd), done.stderr[-2000:]))
    return json.loads([l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def trace_split(path, steps):
    """Per-kernel totals of a rocpd database (rocprofv3 --kernel-trace) of the worker running the blinded step alone."""
    import sqlite3

    per = collections.defaultdict(list)
    for name, s, e in sqlite3.connect(path).execute("select name, start, end from kernels"):
        per[name.split("(")[0].replace("void ", "")].append((e - s) / 1e3)
    total = sum(sum(v) for v in per.values())
    rows = [{"kernel": k, "calls": len(v), "total_us": round(sum(v), 1), "mean_us": round(sum(v) / len(v), 2), "pct": round(100.0 * sum(v) / total, 2)}
            for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))]
    blind = sum(r["total_us"] for r in rows if r["kernel"].startswith("blind_"))
    return {"steps_in_trace": steps, "kernel_time_us": round(total, 1), "blind_kernels_us": round(blind, 1),
            "blind_kernels_pct": round(100.0 * blind / total, 2), "kernels": rows,
            "note": "whole worker process: set-up, warm-up and timed steps of the blinded step alone; kernel time summed over 20 streams, not wall time"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "blinding.json"))
    ap.add_argument("--parent-lib", default="", help="libplonk_hip.so built from the parent commit (PLONK_HIP_LIB of its workers)")
    ap.add_argument("--rounds", type=int, default=5, help="times the workers of every build are run, alternating")
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats of every mode inside one worker")
    ap.add_argument("--steps", type=int, default=3, help="steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--streams", type=int, default=20)
    ap.add_argument("--lookup-budget-gb", type=float, default=180.0, help="bench.py's DEFAULT_TABLE_GB")
    ap.add_argument("--srs-list", default="golden,tau")
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--trace-db", default="", help="rocpd database of a kernel trace of the blinded step (see above)")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--srs", default="golden", help="worker: golden (2^10) or tau (2^11 on 2^11 + 6 powers)")
    ap.add_argument("--shapes", default="step,batch,proof", help="worker")
    ap.add_argument("--modes", default="blinded,unblinded", help="worker")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    result = {"tool": "tools/blinding_bench.py " + " ".join(a for a in sys.argv[1:] if os.sep not in a),  # (options without their paths)
              "config": {"batch": args.batch, "contexts": args.streams, "steps_per_repeat": args.steps, "rounds": args.rounds,
                         "repeats_per_worker": args.repeats, "lookup_budget_gb": args.lookup_budget_gb}}
    ms = collections.defaultdict(lambda: collections.defaultdict(list))
    for _ in range(args.rounds):
        for srs in args.srs_list.split(","):
            shapes = "step,batch,proof" if srs == "golden" else "step"
            for build, lib in (("this", ""), ("parent", args.parent_lib)):
                if build == "parent" and not lib:
                    continue
                rec = run_worker(args, srs, lib, shapes)
                result["device"] = rec["device"]
                result.setdefault("table", {})[srs] = rec["table"]
                assert rec["has_blinding"] == (build == "this")
                for shape, modes in rec["ms"].items():
                    for m, v in modes.items():
                        ms[shape]["parent" if build == "parent" else m] += v
    shapes = {}
    for shape, modes in ms.items():
        s = {m: spread(v) for m, v in modes.items()}
        u, b = s["unblinded"], s["blinded"]
        s["blinded_over_unblinded"] = round(b["median_ms"] / u["median_ms"], 4)
        if "parent" in s:
            p = s["parent"]
            s["unblinded_minus_parent_ms"] = round(u["median_ms"] - p["median_ms"], 4)
            s["spread_ms"] = round(max(u["max_ms"] - u["min_ms"], p["max_ms"] - p["min_ms"]), 4)
            s["unblinded_level_with_parent"] = u["min_ms"] <= p["max_ms"]  # the two ranges of repeats overlap, or this build is faster
        shapes[shape] = s
    result["shapes"] = shapes
    if args.trace_db and os.path.exists(args.trace_db):
        result["blinded_step_kernel_split"] = trace_split(args.trace_db, args.trace_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result["shapes"], separators=(",", ":")))


if __name__ == "__main__":
    main()
