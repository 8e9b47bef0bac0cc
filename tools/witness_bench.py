#!/usr/bin/env python3
"""What the witness solver (csrc/witness_solve.h) costs, and what it replaces -> profiles/witness_solve.json, one session.

  (a) the solve alone: `witness_solve` of plonk_profile_read (HIP events around witness_solve_kernel) for the 2^11 chain and the
      Poseidon circuit at B = 512, and for the chain at B = 1 at 2^11 and 2^16 (what a decision about a levelised form for small
      batches needs).
  (b) a step in bench.py's configuration — 20 contexts x 512 proofs, the same table budget, the 2^11 chain, every witness distinct —
      with a fresh batch uploaded INSIDE the timed region, five ways in one process, alternating:
        inputs    upload_input_values_async, 32 B per proof, the device solves
        values    upload_values_async of pre-packed [B][V] bytes (64 KiB per proof): the existing path, the baseline
        resident  the witnesses staged before the timed region: bench.py's own step
        staged_inputs   the two-slot intake (csrc/prover_intake.h): batch k + 1 goes in by stage_input_values_async right after
                        run(k) was enqueued — copy, solve and gathers on the copy stream beside batch k's rounds — then download(k),
                        advance().  One stage per step, the first of a repeat with its advance inside the timed region too.
        staged_values   the same with stage_values_async of the [B][V] bytes
      -> profiles/intake_pipeline.json (--out), with the shader clock sampled over one more, untimed round of every way.
  (c) the host side it replaces: Program.fill_variable_assignments + BatchProver.upload per proof, on the same circuits.

No ratio is fixed in advance: `inputs` is judged against the spread of `values` over its own repeats."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, HERE]
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PTAU = os.path.join(REPO, "tests", "golden", "srs_2048.ptau")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def solve_alone(pa, setup, program, inputs_of, B, repeats):
    """(a): ms of witness_solve_kernel per upload of B proofs, after one warm-up upload."""
    ctx = pa.get_context()
    bp = pa.BatchProver(setup, program)
    starts = [inputs_of(b) for b in range(B)]
    bp.set_inputs(list(starts[0]))
    blob = le([s[k] for s in starts for k in bp.inputs])
    bp.upload_input_values(blob, B)
    assert bp.solve_failures() == [None] * B
    ms = []
    ctx.profile(True)
    for _ in range(repeats):
        ctx.profile_reset()
        bp.upload_input_values(blob, B)
        total, launches, _ = ctx.profile_read("witness_solve")
        assert launches == 1
        ms.append(total)
    ctx.profile(False)
    out = spread(ms)
    out.update(group_order=program.group_order, batch=B, variables=len(bp.variables), inputs=len(bp.inputs),
               us_per_proof=round(1e3 * out["median_ms"] / B, 3))
    return out


def host_fill(pa, setup, program, inputs_of, count):
    """(c): Program.fill_variable_assignments, then BatchProver.upload of the dictionaries, per proof."""
    bp = pa.BatchProver(setup, program)
    t0 = time.perf_counter()
    wits = [program.fill_variable_assignments(inputs_of(b)) for b in range(count)]
    t1 = time.perf_counter()
    bp.upload(wits)
    t2 = time.perf_counter()
    return {"group_order": program.group_order, "proofs": count, "fill_variable_assignments_ms_per_proof": round(1e3 * (t1 - t0) / count, 4),
            "upload_ms_per_proof": round(1e3 * (t2 - t1) / count, 4), "total_ms_per_proof": round(1e3 * (t2 - t0) / count, 4)}


def step_ways(pa, args):
    """(b).  The [B][V] blobs of the baseline come from the device's own solve (plonk_prover_download_variables), which the test
    suite checks against the oracle: no Python loop over 10 240 x 2 048 values."""
    import contextlib

    from bench import chain_program_lines
    from plonkathon_amd._lib import check

    n, B, S = 1 << args.log_n, args.batch, args.streams
    ctxs = [pa.get_context()] + [pa.Context(0) for _ in range(S - 1)]
    budget = int(args.lookup_budget_gb * 1e9)
    knobs = contextlib.ExitStack()
    for c in ctxs:
        c.msm_lookup(0, 0, budget)
        if S >= 8:
            knobs.enter_context(c.tuning(msm_groups=1))  # bench.py's setting for eight or more streams
    setup = pa.Setup.from_file(PTAU)
    program = pa.Program(chain_program_lines(n), n)
    provers = [pa.BatchProver(setup, program, c) for c in ctxs]
    V = len(provers[0].variables)
    small, full = [], []
    for k, pr in enumerate(provers):
        pr.set_inputs(["x0"])
        a = pr.ctx.host_alloc(32 * B)
        a[:] = le(3 + k * B + b for b in range(B))
        pr.upload_input_values(bytes(a), B)
        f = pr.ctx.host_alloc(32 * B * V)
        check(pr.ctx.L.plonk_prover_download_variables(pr._h, B, None, 0, ctypes.addressof(f)))
        small.append(a)
        full.append(f)

    def stage(mode):
        for pr, a, f in zip(provers, small, full):
            if mode == "staged_inputs":
                pr.stage_input_values_async(a, B)
            else:
                pr.stage_values_async(f, B)

    def step(mode, stage_next=False):
        for pr, a, f in zip(provers, small, full):
            if mode == "inputs":
                pr.upload_input_values_async(a, B)
            elif mode == "values":
                pr.upload_values_async(f, B)
            pr.run()
            if stage_next:
                (pr.stage_input_values_async(a, B) if mode == "staged_inputs" else pr.stage_values_async(f, B))
        raw = [pr.download_raw() for pr in provers]
        assert not any(any(st) for _, st in raw)
        return b"".join(r for r, _ in raw)

    def steps(mode, count):
        """`count` steps, every one with a fresh batch's bytes; the proofs of the last."""
        out = None
        if mode.startswith("staged_"):
            stage(mode)
        for i in range(count):
            out = None  # (one step's records at a time, as a loop over step() holds them)
            if mode.startswith("staged_"):
                for pr in provers:
                    pr.advance()
            out = step(mode, stage_next=mode.startswith("staged_") and i + 1 < count)
        return out

    def sync():
        for c in ctxs:
            c.sync()

    modes = tuple(args.modes.split(","))  # (a kernel trace of one way alone: --modes inputs)
    proofs = {m: steps(m, 2 if m.startswith("staged_") else 1) for m in modes for _ in range(max(1, args.warmup))}  # (the first step builds the MSM table)
    assert len(set(proofs.values())) == 1, "every way must give the same proofs"
    ms = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:  # alternating: a drift of the clock falls on all of them alike
            sync()
            t0 = time.perf_counter()
            steps(m, args.steps)
            sync()
            ms[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
    # the shader clock under this load, from one more round of every way that is NOT timed: the sampler starts a process every
    # ~0.2 s, which costs the timed steps 2-3 ms each when it runs beside them
    from bench_legs import ClockSampler

    sampler = ClockSampler(0)
    sampler.start()
    for m in modes:
        steps(m, args.steps)
    sync()
    clocks = sampler.summary()
    if clocks:
        clocks["source"] = "rocm-smi --showclocks --showpower over one more, untimed round of every way, right behind the timed ones"
    knobs.close()
    out = {m: dict(spread(v), proofs_per_s=round(1e3 * B * S / statistics.median(v), 1)) for m, v in ms.items()}
    out["config"] = {"group_order": n, "batch": B, "contexts": S, "steps_per_repeat": args.steps, "lookup_budget_gb": args.lookup_budget_gb,
                     "bytes_per_proof": {"inputs": 32, "values": 32 * V}, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                     "table": setup.device_bases(ctxs[0]).lookup_info()}
    out["clocks"] = clocks
    for m in ("staged_inputs", "staged_values"):  # against the same session's `inputs` and `resident`, and the spread of the repeats
        if m in out and "inputs" in out and "resident" in out:
            lo, hi = out[m], out["inputs"]
            out[m + "_vs_inputs"] = {"gain_ms": round(hi["median_ms"] - lo["median_ms"], 4),
                                     "spread_ms": round(max(hi["max_ms"] - hi["min_ms"], lo["max_ms"] - lo["min_ms"]), 4),
                                     "gain_exceeds_spread": lo["max_ms"] < hi["min_ms"],
                                     "behind_resident_ms": round(lo["median_ms"] - out["resident"]["median_ms"], 4)}
    if "inputs" in out and "values" in out:
        v = out["values"]
        out["inputs_minus_values_ms"] = round(out["inputs"]["median_ms"] - v["median_ms"], 4)
        out["values_spread_ms"] = round(v["max_ms"] - v["min_ms"], 4)
        out["inputs_behind_values_beyond_its_spread"] = out["inputs"]["median_ms"] > v["max_ms"]
    for a, f, pr in zip(small, full, provers):
        pr.ctx.host_free(a)
        pr.ctx.host_free(f)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "witness_solve.json"))
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--log-n", type=int, default=11)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--streams", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5, help="(b): steps per timed repeat")
    ap.add_argument("--repeats", type=int, default=4, help="(b): timed repeats of each way, alternating")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="inputs,values,resident,staged_inputs,staged_values", help="(b): the ways to run, in their alternating order")
    ap.add_argument("--lookup-budget-gb", type=float, default=180.0, help="bench.py's DEFAULT_TABLE_GB")
    ap.add_argument("--large-log-n", type=int, default=16, help="(a): the large chain at B = 1 (0 = skip)")
    ap.add_argument("--bench-line", default="", help="a file holding bench.py's JSON line of the same session, to put beside (b)")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    # as bench.py: one hardware queue per compute stream unless the environment says otherwise; before the HIP runtime loads
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(min(20, max(4, args.streams))))

    import plonkathon_amd as pa
    from bench import chain_program_lines, poseidon_program_lines

    ctx = pa.get_context()
    result = {"device": ctx.name(), "tool": "tools/witness_bench.py " + " ".join(sys.argv[1:])}
    setup = pa.Setup.from_file(PTAU)
    n = 1 << args.log_n
    chain = pa.Program(chain_program_lines(n), n)
    poseidon = pa.Program(poseidon_program_lines(), 1024)
    chain_in = lambda b: {"x0": 3 + b}
    poseidon_in = lambda b: {"L0": 1 + b, "M0": 2 + 3 * b}
    if "a" in parts:
        a = {"chain_B512": solve_alone(pa, setup, chain, chain_in, 512, 10), "poseidon_B512": solve_alone(pa, setup, poseidon, poseidon_in, 512, 10),
             "chain_B1": solve_alone(pa, setup, chain, chain_in, 1, 10)}
        if args.large_log_n:
            from prover_scale import device_tau_setup

            big = 1 << args.large_log_n
            a["chain_large_B1"] = solve_alone(pa, device_tau_setup(pa, big), pa.Program(chain_program_lines(big), big), chain_in, 1, 5)
        result["a_solve_alone"] = a
    if "c" in parts:
        result["c_host_fill"] = {"chain": host_fill(pa, setup, chain, chain_in, 64), "poseidon": host_fill(pa, setup, poseidon, poseidon_in, 64)}
    if "b" in parts:
        result["b_step"] = step_ways(pa, args)
    if args.bench_line and os.path.exists(args.bench_line):
        for line in open(args.bench_line):
            if line.startswith("{"):
                rec = json.loads(line)
                result["bench_py_same_session"] = {k: rec.get(k) for k in ("ms_per_step", "proofs_per_s", "value", "metric", "clock_mhz") if k in rec}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, separators=(",", ":")))


if __name__ == "__main__":
    main()
