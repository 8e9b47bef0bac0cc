#!/usr/bin/env python3
"""What checking a whole step costs next to proving it (one MI355X, one session) -> profiles/verify_batch.json.

At group_order 2^11, for B = 512 and B = 10 240 proofs of the chain circuit on the library's default MSM table:
  (a) device part of BatchVerifier.verify_prover — plonk_verifier_load_prover + plonk_verifier_fold(0, B) — median of 5, timed
      with plonk_timer_* (HIP events on the context's stream); the fold alone is timed beside it;
  (b) the host pairing check of the two folded points;
  (c) ms_per_step of a plain `python bench.py` run as a child process on the same box (bench.py and the prover are the parent
      commit's: this change touches neither), or of `--bench-json FILE` holding such a line;
  (d) VerificationKey.verify_proof on 16 proofs of the same batch, per proof.
Ratios: (a) / (c) — wanted <= 0.10 at B = 10 240 — and (d) x B / ((a) + (b)).

usage: python tools/verify_bench.py [--batches 512,10240] [--bench-json FILE | --no-bench] [--out profiles/verify_batch.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,10240")
    ap.add_argument("--bench-json", default="", help="a file holding bench.py's result line (skips the child run)")
    ap.add_argument("--no-bench", action="store_true", help="leave (c) and the ratio (a) / (c) unmeasured")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "verify_batch.json"))
    args = ap.parse_args()

    import bench
    from bench_legs import ClockSampler
    from plonkathon_amd import BatchProver, BatchVerifier, Program, Setup, get_context
    from plonkathon_amd._lib import check

    n = bench.GROUP_ORDER = 2048
    ctx = get_context()
    setup = Setup.from_file(bench.PTAU)
    program = Program(bench.chain_program_lines(n), n)
    vk = setup.verification_key(program.common_preprocessed_input())
    rec = {"group_order": n, "device": ctx.name(), "runs": []}

    def timed(fn):
        ms = ctypes.c_float(0)
        check(ctx.L.plonk_timer_start(ctx.handle))
        out = fn()
        check(ctx.L.plonk_timer_stop_ms(ctx.handle, ctypes.byref(ms)))
        return ms.value, out

    for B in [int(x) for x in args.batches.split(",")]:
        wits = [bench.witness_for(i) for i in range(B)]
        bp = BatchProver(setup, program)
        bp.upload(wits)
        bp.run()
        blob, status = bp.download_raw()
        assert not any(status)
        bv = BatchVerifier(vk, 1)
        assert bv.verify_prover(bp)  # warm-up: code objects, allocations
        sampler = ClockSampler(0)
        sampler.start()
        dev_ms, fold_ms, pair_ms = [], [], []
        for _ in range(5):
            ms, (L, R) = timed(lambda: (bv.load_prover(bp), bv.fold(0, B))[1])
            dev_ms.append(ms)
            fold_ms.append(timed(lambda: bv.fold(0, B))[0])
            t0 = time.perf_counter()
            assert bv.check_pairing(L, R)
            pair_ms.append(1e3 * (time.perf_counter() - t0))
        clocks = sampler.summary()
        idx = [(i * 2654435761) % B for i in range(16)]
        t0 = time.perf_counter()
        for i in idx:
            assert vk.verify_proof(n, BatchProver.decode(blob[768 * i : 768 * (i + 1)]), [wits[i]["x0"]])
        one_ms = 1e3 * (time.perf_counter() - t0) / len(idx)
        a, b = statistics.median(dev_ms), statistics.median(pair_ms)
        rec["runs"].append({"batch": B, "a_device_ms_median_of_5": a, "a_device_ms_all": dev_ms, "fold_alone_ms_median_of_5": statistics.median(fold_ms),
                            "b_host_pairing_ms_median_of_5": b, "d_verify_proof_ms_per_proof": one_ms,
                            "speedup_d_x_B_over_a_plus_b": one_ms * B / (a + b), "clocks": clocks})
        del bv, bp
    if args.bench_json:
        line = [l for l in open(args.bench_json).read().splitlines() if l.startswith("{")][-1]
    elif not args.no_bench:
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")], capture_output=True, text=True, check=True).stdout
        line = [l for l in out.splitlines() if l.startswith("{")][-1]
    else:
        line = None
    if line:
        b = json.loads(line)
        rec["c_bench_ms_per_step"] = b["ms_per_step"]
        rec["c_bench_proofs_per_s"] = b["value"]
        for r in rec["runs"]:
            if r["batch"] == 10240:
                r["ratio_a_over_c"] = r["a_device_ms_median_of_5"] / b["ms_per_step"]
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
