#!/usr/bin/env python3
"""The two forms of the witness solve (csrc/witness_solve.h) side by side -> profiles/witness_levels.json, one session.

  cells      circuits chain 2^11, Poseidon 2^10, poseidon_multi(8) at 2^13, poseidon_multi(64) at 2^16, each at B in {1, 8, 64, 512}
             (a cell whose batch buffers cannot be allocated is dropped, and says so).  Per cell the solve alone — `witness_solve`
             of plonk_profile_read, HIP events around the one kernel of an upload — forced to one lane per proof, forced to levels,
             and under the automatic rule, with the rule's pick: median and min-max of 5 uploads after one warm-up.
  end to end prove_inputs of one poseidon_multi(64) proof against the same proof from resident variables (wall clock, 5 runs).
  --repo DIR a tree to import plonkathon_amd from instead of this one: a build of the parent commit, which has one form, for the
             baseline cells (--cells); its output is merged into the main run's file with --baseline FILE.

The fit of the rule's two constants (csrc/prover_scans.h: SOLVE_ROW_NS, SOLVE_LEVEL_STEP_NS) is computed here from the forced
cells and written beside them with the cells it used."""
import argparse
import json
import os
import re
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PTAU = os.path.join(REPO, "tests", "golden", "srs_2048.ptau")
REPEATS = 5
CIRCUITS = ("chain_2048", "poseidon_1024", "poseidon_x8_8192", "poseidon_x64_65536")
BATCHES = (1, 8, 64, 512)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def poseidon_multi(lines, K):
    """K independent Poseidon hashes in one circuit: every name of copy k prefixed h{k}x, the `public` lines first."""
    public, rows = [], []
    for k in range(K):
        for line in lines:
            line = re.sub(r"\b[A-Za-z][A-Za-z0-9]*\b", lambda m: m.group(0) if m.group(0) == "public" else "h%dx%s" % (k, m.group(0)), line)
            (public if line.endswith(" public") else rows).append(line)
    return public + rows


def circuit(name):
    """(program lines, group order, inputs of proof b)"""
    from bench import chain_program_lines, poseidon_program_lines

    if name.startswith("chain_"):
        n = int(name.split("_")[1])
        return chain_program_lines(n), n, lambda b: {"x0": 3 + b}
    if name == "poseidon_1024":
        return poseidon_program_lines(), 1024, lambda b: {"L0": 1 + b, "M0": 2 + 3 * b}
    K, n = (int(x) for x in re.match(r"poseidon_x(\d+)_(\d+)", name).groups())
    return (poseidon_multi(poseidon_program_lines(), K), n,
            lambda b: {"h%dx%s" % (k, v): 1 + 10 * b + 100 * k + (5 if v == "M0" else 0) for k in range(K) for v in ("L0", "M0")})


def solve_ms(ctx, bp, blob, B):
    """ms of the solve kernel of REPEATS uploads, after one warm-up upload"""
    bp.upload_input_values(blob, B)
    assert bp.solve_failures() == [None] * B
    ms = []
    ctx.profile(True)
    for _ in range(REPEATS):
        ctx.profile_reset()
        bp.upload_input_values(blob, B)
        total, launches, _ = ctx.profile_read("witness_solve")
        assert launches == 1
        ms.append(total)
    ctx.profile(False)
    return spread(ms)


def measure_cell(pa, ctx, bp, inputs_of, B, has_forms):
    from plonkathon_amd._lib import check

    starts = [inputs_of(b) for b in range(B)]
    blob = le([s[k] for s in starts for k in bp.inputs])
    if not has_forms:
        return {"rule": solve_ms(ctx, bp, blob, B)}
    cell = {}
    for form, k in (("lanes", 1), ("levels", 2), ("rule", 0)):
        check(ctx.L.plonk_prover_set_options(bp._h, k << 16))
        cell[form] = solve_ms(ctx, bp, blob, B)
    cell["pick"] = bp.solve_plan(B)["form"]
    faster = min(("lanes", "levels"), key=lambda f: cell[f]["median_ms"])
    cell["faster_forced"] = faster
    own_spread = max(cell[f]["max_ms"] - cell[f]["min_ms"] for f in ("lanes", "levels", "rule"))
    cell["rule_behind_faster_ms"] = round(cell["rule"]["median_ms"] - cell[faster]["median_ms"], 4)
    cell["spread_ms"] = round(own_spread, 4)
    cell["rule_ok"] = cell["pick"] == faster or cell["rule_behind_faster_ms"] <= own_spread
    return cell


def end_to_end(pa, ctx, bp, inputs_of):
    """One proof from its inputs (upload, solve, prove, download) against the same proof from variables already resident."""
    start = [inputs_of(0)]
    proofs = bp.prove_inputs(start)
    solved = bp.variable_values()[0]
    blob = le([solved[v] for v in bp.variables])
    ms = {"prove_inputs": [], "resident": []}
    for _ in range(REPEATS):
        ctx.sync()
        t0 = time.perf_counter()
        bp.upload_input_values(le([start[0][k] for k in bp.inputs]), 1)
        bp.run()
        raw = bp.download_raw()
        ms["prove_inputs"].append(1e3 * (time.perf_counter() - t0))
        bp.upload_values(blob, 1)
        ctx.sync()
        t0 = time.perf_counter()
        bp.run()
        assert bp.download_raw() == raw
        ms["resident"].append(1e3 * (time.perf_counter() - t0))
    assert raw[1] == bytes(1) and len(proofs) == 1
    out = {k: spread(v) for k, v in ms.items()}
    out["exposed_ms"] = round(out["prove_inputs"]["median_ms"] - out["resident"]["median_ms"], 4)
    return out


def fit(cells):
    """The rule's constants: ns per serial step over the B = 1 cells of every circuit, where the launch is one wave or one
    workgroup and nothing but the chain of dependent steps is timed.  SOLVE_ROW_NS = the median over the circuits of the one-lane
    form's ns per active row; SOLVE_LEVEL_STEP_NS / SOLVE_LEVEL_STEP_WIDE_NS = the levelised form's ns per step with a workgroup
    of one wave (T = 64) / of four (T = 256)."""
    rows, steps, used = [], {64: [], 256: []}, []
    for name, per_b in cells.items():
        c = per_b.get("1")
        if not c or "lanes" not in c:
            continue
        plan = per_b["plan"]
        rows.append(1e6 * c["lanes"]["median_ms"] / plan["active_rows"])
        steps[plan["threads"]].append(1e6 * c["levels"]["median_ms"] / plan["steps"])
        used.append("%s B=1 (T = %d)" % (name, plan["threads"]))
    if not rows:
        return None
    out = {"row_ns_per_cell": [round(x, 1) for x in rows], "level_step_ns_per_cell": {str(t): [round(x, 1) for x in v] for t, v in steps.items()},
           "fitted_on": used, "SOLVE_ROW_NS": round(statistics.median(rows), 1)}
    for t, key in ((64, "SOLVE_LEVEL_STEP_NS"), (256, "SOLVE_LEVEL_STEP_WIDE_NS")):
        if steps[t]:
            out[key] = round(statistics.median(steps[t]), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "witness_levels.json"))
    ap.add_argument("--repo", default=REPO, help="the tree to import plonkathon_amd from")
    ap.add_argument("--cells", default="", help="circuit:B,... (default: every circuit at every batch)")
    ap.add_argument("--baseline", default="", help="the JSON of a --repo run of the parent commit in the same session, to merge in")
    ap.add_argument("--no-end-to-end", action="store_true")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.repo), REPO, HERE]

    import plonkathon_amd as pa
    from bench_legs import ClockSampler
    from prover_scale import device_tau_setup

    ctx = pa.get_context()
    has_forms = hasattr(ctx.L, "plonk_prover_solve_plan")
    wanted = [tuple(c.split(":")) for c in args.cells.split(",") if c] or [(c, str(b)) for c in CIRCUITS for b in BATCHES]
    result = {"device": ctx.name(), "tool": "tools/witness_levels_bench.py " + " ".join(sys.argv[1:]), "package": "this commit" if os.path.abspath(args.repo) == REPO else "parent commit",
              "repeats": REPEATS, "cells": {}}
    sampler = ClockSampler(0)
    sampler.start()
    small = pa.Setup.from_file(PTAU)
    for name in dict.fromkeys(c for c, _ in wanted):
        lines, n, inputs_of = circuit(name)
        t0 = time.perf_counter()
        bp = pa.BatchProver(small if n <= 2048 else device_tau_setup(pa, n), pa.Program(lines, n))
        bp.set_inputs(list(inputs_of(0)))
        per_b = result["cells"].setdefault(name, {})
        if has_forms:
            per_b["plan"] = {k: v for k, v in bp.solve_plan(1).items() if k != "form"}
        print("%s: built in %.1f s" % (name, time.perf_counter() - t0), flush=True)
        for B in [int(b) for c, b in wanted if c == name]:
            try:
                per_b[str(B)] = measure_cell(pa, ctx, bp, inputs_of, B, has_forms)
            except (AssertionError, MemoryError) as e:  # the library's out-of-memory refusal comes up as a failed check()
                if "memory" not in str(e).lower() and "alloc" not in str(e).lower():
                    raise
                per_b[str(B)] = {"dropped": "the batch buffers do not fit: " + str(e)[:200]}
            print(name, B, json.dumps(per_b[str(B)], separators=(",", ":")), flush=True)
        if name == "poseidon_x64_65536" and has_forms and not args.no_end_to_end:
            from plonkathon_amd._lib import check

            check(ctx.L.plonk_prover_set_options(bp._h, 0))
            result["end_to_end_poseidon_x64_B1"] = end_to_end(pa, ctx, bp, inputs_of)
            print("end to end", json.dumps(result["end_to_end_poseidon_x64_B1"], separators=(",", ":")), flush=True)
        del bp
    result["clock"] = sampler.summary()
    if has_forms:
        result["fit"] = fit(result["cells"])
        result["rule_ok_in_every_cell"] = all(c.get("rule_ok", True) for per_b in result["cells"].values() for k, c in per_b.items() if k != "plan")
    if args.baseline and os.path.exists(args.baseline):
        base = json.load(open(args.baseline))
        result["parent_commit"] = {"cells": base["cells"], "clock": base.get("clock"), "tool": base["tool"]}
        versus = {}
        for name, per_b in base["cells"].items():
            for B, c in per_b.items():
                mine = result["cells"].get(name, {}).get(B)
                if B == "plan" or not mine or "rule" not in mine:
                    continue
                sp = max(c["rule"]["max_ms"] - c["rule"]["min_ms"], mine["rule"]["max_ms"] - mine["rule"]["min_ms"])
                versus["%s B=%s" % (name, B)] = {"parent_ms": c["rule"]["median_ms"], "rule_ms": mine["rule"]["median_ms"], "spread_ms": round(sp, 4),
                                                 "speedup": round(c["rule"]["median_ms"] / mine["rule"]["median_ms"], 2),
                                                 "level_within_spread": abs(c["rule"]["median_ms"] - mine["rule"]["median_ms"]) <= sp}
        result["rule_against_parent"] = versus
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, separators=(",", ":")))


if __name__ == "__main__":
    main()
