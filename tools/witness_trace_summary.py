#!/usr/bin/env python3
"""Where the witness solver's latency stays exposed in a step: from the rocpd database of
`rocprofv3 --kernel-trace --stats -- python tools/witness_bench.py --parts b --modes inputs ...` (a run of its own, no counters).

usage: python tools/witness_trace_summary.py trace_results.db [steps] > profiles/witness_solve_step_kernel_stats.txt
Prints the per-kernel table of tools/rocprof_summary.py, then for witness_solve_kernel: the time its launches cover, how much of
that no other kernel overlaps (the chip runs nothing but lone waves then: the exposed part), and how the launches queue behind
one another."""
import collections
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rows = [(n.split("(")[0].replace("void ", ""), s, e) for n, s, e in db.execute("select name, start, end from kernels")]
per = collections.defaultdict(list)
for name, s, e in rows:
    per[name].append((e - s) / 1e3)
total_all = sum(sum(v) for v in per.values())
print("%-58s %7s %13s %11s %11s %11s %7s" % ("kernel", "calls", "total_us", "mean_us", "median_us", "min_us", "pct"))
for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
    v.sort()
    print("%-58s %7d %13.1f %11.2f %11.2f %11.2f %6.2f%%" % (name, len(v), sum(v), sum(v) / len(v), v[len(v) // 2], v[0], 100.0 * sum(v) / total_all))


def union(iv):
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def minus(a, b):
    """total length of the union `a` outside the union `b`"""
    total, j = 0, 0
    for s, e in a:
        cur = s
        while j < len(b) and b[j][1] <= cur:
            j += 1
        k = j
        while k < len(b) and b[k][0] < e:
            if b[k][0] > cur:
                total += b[k][0] - cur
            cur = max(cur, b[k][1])
            k += 1
        if cur < e:
            total += e - cur
    return total


# the tool's set-up stages every prover once, alone on the chip, and reads the variables back: the steps begin after the last
# variable_gather_kernel
t_setup = max([e for n, s, e in rows if n == "variable_gather_kernel"], default=0)
rows = [r for r in rows if r[1] >= t_setup]
solve = [(s, e) for n, s, e in rows if n == "witness_solve_kernel"]
other = union([(s, e) for n, s, e in rows if n != "witness_solve_kernel"])
if solve:
    su = union(solve)
    covered = sum(e - s for s, e in su)
    alone = minus(su, other)
    depth = collections.Counter()
    for s, e in solve:  # how many solves are in flight when this one starts
        depth[sum(1 for s2, e2 in solve if s2 <= s < e2)] += 1
    print()
    print("after the set-up — witness_solve_kernel: %d launches, %.1f us each on average, %.1f ms of kernel time" % (len(solve), sum(e - s for s, e in solve) / len(solve) / 1e3, sum(e - s for s, e in solve) / 1e6))
    print("  wall time covered by at least one solve: %.2f ms; of that with NO other kernel running: %.2f ms (%.0f %%)" % (covered / 1e6, alone / 1e6, 100.0 * alone / covered))
    if steps:
        print("  per step (%d steps in the trace): %.2f ms covered, %.2f ms exposed" % (steps, covered / 1e6 / steps, alone / 1e6 / steps))
    print("  solves in flight at a solve's start (itself included): " + ", ".join("%d: %d launches" % kv for kv in sorted(depth.items())))
