#!/usr/bin/env python3
"""What a prover over a table of circuits (MultiBatchProver, plonk_prover_create_multi) buys a caller who serves many small
circuits of one setup -> profiles/multi_prover.json, one session.

The batch: 512 proofs at group_order 2^11 as 16 circuits x 32 proofs, the circuits variants of the squaring chain with different
constants (x_{i+1} = x_i^2 + k).  Proved four ways, witnesses resident, a step = run everything and download everything:
    multi          one MultiBatchProver, the 512 proofs dealt round-robin over the circuits
    serial         sixteen BatchProvers of 32 proofs one after another on ONE context
    contexts       sixteen BatchProvers of 32 proofs on SIXTEEN contexts (bench.py's msm_groups = 1 for eight or more streams)
    floor          one BatchProver proving 512 proofs of ONE of the circuits: what the batch would cost were it not mixed
The modes alternate inside a repeat, so that a drift of the clock falls on all of them alike; a figure is the median and min-max
over the repeats.  There is no pass mark: the record states `multi` against the other three."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, HERE]
PTAU = os.path.join(REPO, "tests", "golden", "srs_2048.ptau")
MODES = ("multi", "serial", "contexts", "floor")


def variant_lines(n, k):
    """the squaring chain with the constant k added in every row (k = 0: bench.py's chain)"""
    step = "x%d <== x%d * x%d" + (" + %d" % k if k else "")
    return ["x0 public"] + [step % (i + 1, i, i) for i in range(n - 1)]


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_prover.json"))
    ap.add_argument("--log-n", type=int, default=11)
    ap.add_argument("--circuits", type=int, default=16)
    ap.add_argument("--per-circuit", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats of every mode (at least 5)")
    ap.add_argument("--steps", type=int, default=3, help="steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lookup-budget-gb", type=float, default=180.0, help="bench.py's DEFAULT_TABLE_GB")
    args = ap.parse_args()
    K, per, n = args.circuits, args.per_circuit, 1 << args.log_n
    B = K * per
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(min(20, max(4, K))))  # as bench.py, before the HIP runtime loads
    import plonkathon_amd as pa
    from bench_legs import ClockSampler
    from plonkathon_amd.batch import _pack_witnesses
    from plonkathon_amd.field import R_MOD

    one = pa.get_context()
    many = [pa.Context(0) for _ in range(K)]
    knobs = contextlib.ExitStack()
    for c in [one] + many:
        c.msm_lookup(0, 0, int(args.lookup_budget_gb * 1e9))
    if K >= 8:
        for c in many:
            knobs.enter_context(c.tuning(msm_groups=1))
    setup = pa.Setup.from_file(PTAU)
    programs = [pa.Program(variant_lines(n, k), n) for k in range(K)]
    wits = [[p.fill_variable_assignments({"x0": 3 + j}) for j in range(per)] for p in programs]
    blobs = [_pack_witnesses(w, tuple(p.wiring_table()[0]), R_MOD) for p, w in zip(programs, wits)]
    row = len(blobs[0]) // per  # every variant has the chain's variables: one row width

    multi = pa.MultiBatchProver(setup, programs, one)
    assert all(multi.variables(k) == multi.variables(0) and len(blobs[k]) == per * row for k in range(K)) and multi.n_vars * 32 == row
    ids = [b % K for b in range(B)]
    multi.upload_values(b"".join(blobs[b % K][row * (b // K) : row * (b // K + 1)] for b in range(B)), ids)
    serial = [pa.BatchProver(setup, p, one) for p in programs]
    contexts = [pa.BatchProver(setup, p, c) for p, c in zip(programs, many)]
    for group in (serial, contexts):
        for k, bp in enumerate(group):
            bp.upload_values(blobs[k], per)
    floor = pa.BatchProver(setup, programs[0], one)
    floor_wits = [programs[0].fill_variable_assignments({"x0": 3 + j}) for j in range(B)]
    floor.upload_values(_pack_witnesses(floor_wits, tuple(programs[0].wiring_table()[0]), R_MOD), B)
    provers = {"multi": [multi], "serial": serial, "contexts": contexts, "floor": [floor]}

    def step(mode):
        for pr in provers[mode]:
            pr.run()
        return [pr.download_raw() for pr in provers[mode]]

    def sync():
        for c in [one] + many:
            c.sync()

    # the four ways prove the same thing: the mixed batch's records are the one-circuit provers', position by position
    got = step("multi")[0]
    ref = step("serial")
    assert not any(got[1]) and all(not any(st) for _, st in ref)
    for b in range(B):
        assert got[0][768 * b : 768 * (b + 1)] == ref[b % K][0][768 * (b // K) : 768 * (b // K + 1)], b
    for mode in MODES:
        for _ in range(args.warmup):
            step(mode)
    sampler = ClockSampler(0)
    sampler.start()
    ms = {m: [] for m in MODES}
    for r in range(max(5, args.repeats)):
        order = MODES if r % 2 == 0 else MODES[::-1]  # alternating order
        for mode in order:
            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(mode)
            sync()
            ms[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
    clock = sampler.summary()
    knobs.close()
    result = {"tool": "tools/multi_prover_bench.py " + " ".join(a for a in sys.argv[1:] if os.sep not in a), "device": one.name(), "clock": clock,
              "config": {"group_order": n, "circuits": K, "proofs_per_circuit": per, "proofs": B, "steps_per_repeat": args.steps,
                         "warmup_steps": args.warmup, "lookup_budget_gb": args.lookup_budget_gb, "srs": "tests/golden/srs_2048.ptau",
                         "order": "the four modes in turn inside a repeat, reversed every other repeat"},
              "table": setup.device_bases(one).lookup_info(),
              "ms_per_step": {m: spread(v) for m, v in ms.items()}}
    med = {m: statistics.median(v) for m, v in ms.items()}
    result["multi_against"] = {m: {"speedup": round(med[m] / med["multi"], 3), "multi_is_faster": max(ms["multi"]) < min(ms[m])}
                               for m in MODES if m != "multi"}
    result["proofs_per_s"] = {m: round(B / med[m] * 1e3, 1) for m in MODES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"ms_per_step": result["ms_per_step"], "multi_against": result["multi_against"]}, separators=(",", ":")))


if __name__ == "__main__":
    main()
