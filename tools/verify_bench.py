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

`--circuits K[,K...]` adds the mixed leg -> profiles/verify_multi.json: K distinct 2^11 circuits (the chain with another constant
added in its last row per circuit), `--total` resident proofs split evenly over K provers, checked
  (m) by one MultiBatchVerifier: device part of verify_provers — plonk_verifier_load_provers + plonk_verifier_fold(0, B) — median of
      5; beside it one fold of a half range (what every bisection step costs) and the one host pairing check;
  (s) by K BatchVerifiers of B / K proofs each: the sum of their device parts, and their K host pairing checks.
`--batches ""` skips the one-circuit legs.

usage: python tools/verify_bench.py [--batches 512,10240] [--bench-json FILE | --no-bench] [--out profiles/verify_batch.json]
                                    [--circuits 4,16] [--total 10240] [--multi-out profiles/verify_multi.json]"""
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
    ap.add_argument("--circuits", default="", help="table sizes K of the mixed leg, e.g. 4,16")
    ap.add_argument("--total", type=int, default=10240, help="resident proofs of the mixed leg, split evenly over the K circuits")
    ap.add_argument("--multi-out", default=os.path.join(REPO, "profiles", "verify_multi.json"))
    args = ap.parse_args()

    import bench
    from bench_legs import ClockSampler
    from plonkathon_amd import BatchProver, BatchVerifier, MultiBatchVerifier, Program, Setup, get_context
    from plonkathon_amd.field import R_MOD
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

    def mixed_leg(K):
        per = args.total // K
        B = per * K
        provers, vks = [], []
        for c in range(K):
            lines = bench.chain_program_lines(n)
            if c:
                lines[-1] += " + %d" % c
            prog = Program(lines, n)
            vks.append(setup.verification_key(prog.common_preprocessed_input()))
            wits = []
            for i in range(per):
                w = bench.witness_for(c * per + i)
                w["x%d" % (n - 1)] = (w["x%d" % (n - 1)] + c) % R_MOD
                wits.append(w)
            bp = BatchProver(setup, prog)
            bp.upload(wits)
            bp.run()
            assert not any(bp.download_raw()[1])
            provers.append(bp)
        labelled = list(enumerate(provers))
        mv = MultiBatchVerifier([(vk, 1) for vk in vks])
        singles = [BatchVerifier(vk, 1) for vk in vks]
        assert mv.verify_provers(labelled)  # warm-up: code objects, allocations
        assert all(bv.verify_prover(bp) for bv, bp in zip(singles, provers))
        sampler = ClockSampler(0)
        sampler.start()
        m_dev, m_half, m_pair, s_dev, s_pair = [], [], [], [], []
        for _ in range(5):  # the two ways alternate
            ms, (L, R) = timed(lambda: (mv.load_provers(labelled), mv.fold(0, B))[1])
            m_dev.append(ms)
            m_half.append(timed(lambda: mv.fold(0, B // 2))[0])
            t0 = time.perf_counter()
            assert mv.check_pairing(L, R)
            m_pair.append(1e3 * (time.perf_counter() - t0))
            ms, folds = timed(lambda: [(bv.load_prover(bp), bv.fold(0, per))[1] for bv, bp in zip(singles, provers)])
            s_dev.append(ms)
            t0 = time.perf_counter()
            assert all(bv.check_pairing(L, R) for bv, (L, R) in zip(singles, folds))
            s_pair.append(1e3 * (time.perf_counter() - t0))
        med = statistics.median
        return {"circuits": K, "batch": B, "m_device_ms_median_of_5": med(m_dev), "m_device_ms_all": m_dev, "m_half_range_fold_ms_median_of_5": med(m_half),
                "m_host_pairing_ms_median_of_5": med(m_pair), "s_device_ms_sum_median_of_5": med(s_dev), "s_device_ms_sum_all": s_dev,
                "s_host_pairings_ms_median_of_5": med(s_pair), "m_total_ms": med(m_dev) + med(m_pair), "s_total_ms": med(s_dev) + med(s_pair),
                "clocks": sampler.summary()}

    if args.circuits:
        multi = {"group_order": n, "device": ctx.name(), "runs": [mixed_leg(int(k)) for k in args.circuits.split(",")]}
        with open(args.multi_out, "w") as f:
            json.dump(multi, f, indent=1)
        print(json.dumps(multi))

    for B in [int(x) for x in args.batches.split(",") if x]:
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
    if not rec["runs"]:
        return
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
