#!/usr/bin/env python3
"""How much longer a step's kernels run beside the other streams than alone on the chip: from two rocpd databases of
`rocprofv3 --kernel-trace -- python bench.py --gpus 1 --steps 2 --warmup 1` — the step as the benchmark runs it, and the same command
with `--batches-per-step 1 --streams 1` (one batch on one stream: every kernel alone).  Each trace is a run of its own, no counters.

usage: python tools/step_contention.py step_results.db lone_results.db [--steps 2 --warmup 1] [--json out.json] > table.txt

Per kernel: calls per step, mean duration alone, mean duration in the step, their ratio, and the extra stream time per step
((in-step mean - lone mean) x calls per step: time a stream's serial lane spends in the kernel beyond its own work).  For the step:
the wall time in which no accumulation kernel is running and the wall time in which nothing is running.

The timed steps of a trace are found from the accumulation launches: the last steps / (warmup + steps) of them, widened to the
stretches of continuous activity that hold the first and the last (the host synchronises between steps, so the chip is idle there).
What this window misses: kernels of the first timed step that ran BEFORE an idle gap ahead of its first accumulation launch (the
packers of a batch staged early, a copy) fall outside it.  Their calls per step then come out fractional (11.5 pack_proofs_kernel
where a step has 20) and "no accumulation kernel running" is understated by their few microseconds; the kernels between a batch's
first MSM and its last are all inside."""
import argparse
import collections
import json
import re
import sqlite3

ACCUMULATION = r"^(msm_comb_rows_kernel|msm_comb_kernel|msm_accumulate_kernel|msm_lookup_kernel)\b"


def short(name):
    return re.sub(r"<.*", lambda m: m.group(0) if len(m.group(0)) <= 8 else "<..>", name.split("(")[0].replace("void ", ""))


def union(iv):
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def timed_rows(path, steps, warmup, acc):
    """(rows of the timed steps, window start, window end); a row is (name, start, end) in ns."""
    db = sqlite3.connect(path)
    rows = sorted(((short(n), s, e) for n, s, e in db.execute("select name, start, end from kernels")), key=lambda r: r[1])
    a = [r for r in rows if acc.search(r[0])]
    if not a:
        raise SystemExit("%s: no accumulation kernel (%s) in the trace" % (path, acc.pattern))
    first = a[len(a) * warmup // (warmup + steps)]
    last = max(a, key=lambda r: r[2])
    busy = union([(s, e) for _, s, e in rows])
    t0 = next(s for s, e in busy if s <= first[1] < e)
    t1 = next(e for s, e in busy if s < last[2] <= e)
    return [r for r in rows if t0 <= r[1] and r[2] <= t1], t0, t1


def covered(iv, t0, t1):
    return sum(min(e, t1) - max(s, t0) for s, e in union(iv) if e > t0 and s < t1)


def per_kernel(rows):
    per = collections.defaultdict(list)
    for n, s, e in rows:
        per[n].append((e - s) / 1e3)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step_db")
    ap.add_argument("lone_db")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--accumulation", default=ACCUMULATION, help="regular expression of the accumulation kernels' names")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    acc = re.compile(args.accumulation)
    rows, t0, t1 = timed_rows(args.step_db, args.steps, args.warmup, acc)
    lone_rows, _, _ = timed_rows(args.lone_db, args.steps, args.warmup, acc)
    step, lone = per_kernel(rows), per_kernel(lone_rows)
    table = []
    for name, v in step.items():
        alone = lone.get(name)
        mean, med = sum(v) / len(v), sorted(v)[len(v) // 2]
        am = sum(alone) / len(alone) if alone else None
        table.append({"kernel": name, "calls_per_step": len(v) / args.steps, "lone_mean_us": am, "step_mean_us": mean, "step_median_us": med,
                      "ratio": mean / am if am else None, "extra_stream_ms_per_step": (mean - am) * len(v) / args.steps / 1e3 if am is not None else None,
                      "accumulation": bool(acc.search(name))})
    table.sort(key=lambda r: -(r["extra_stream_ms_per_step"] or 0))
    wall = (t1 - t0) / 1e6
    acc_ms = covered([(s, e) for n, s, e in rows if acc.search(n)], t0, t1) / 1e6
    any_ms = covered([(s, e) for _, s, e in rows], t0, t1) / 1e6
    short_extra = sum(r["extra_stream_ms_per_step"] or 0 for r in table if not r["accumulation"])
    summary = {"steps": args.steps, "window_ms_per_step": wall / args.steps, "no_accumulation_running_ms_per_step": (wall - acc_ms) / args.steps,
               "nothing_running_ms_per_step": (wall - any_ms) / args.steps, "extra_stream_ms_per_step_outside_accumulation": short_extra}
    print("%-46s %9s %10s %10s %10s %7s %12s" % ("kernel", "calls/step", "lone_us", "step_us", "step_med", "ratio", "extra_ms/step"))
    f = lambda x, fmt: "-" if x is None else fmt % x
    for r in table:
        print("%-46s %9.1f %10s %10.1f %10.1f %7s %12s" % (r["kernel"][:46], r["calls_per_step"], f(r["lone_mean_us"], "%.1f"), r["step_mean_us"],
                                                          r["step_median_us"], f(r["ratio"], "%.2f"), f(r["extra_stream_ms_per_step"], "%.2f")))
    print()
    print("the timed window (whole steps, host gaps between them included): %.2f ms per step over %d steps" % (wall / args.steps, args.steps))
    print("  wall time with no accumulation kernel running: %.2f ms per step" % summary["no_accumulation_running_ms_per_step"])
    print("  wall time with nothing running:                %.2f ms per step" % summary["nothing_running_ms_per_step"])
    print("  extra stream time outside the accumulation kernels, summed over the streams: %.2f ms per step" % short_extra)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"summary": summary, "kernels": table}, fh, indent=1)


if __name__ == "__main__":
    main()
