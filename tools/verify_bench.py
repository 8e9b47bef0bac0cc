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

`--each` runs the localisation leg instead -> profiles/verify_each.json: one batch resident in a BatchVerifier, B = 512 and 10 240, with
k = 1, 16 and 256 proofs corrupted (a_eval + 1, spread evenly over the batch).  Medians of 5, device and host time together
(time.perf_counter around the call), of
  (l) load: the per-proof work every route starts from;
  (b) verify_each's verdicts by bisection: folds and host pairings in series (`pairing_checks` beside it);
  (d) the same verdicts by `device=True`: the whole-batch fold and its host pairing, then ONE plonk_verifier_check_each;
and from plonk_profile_read the device time of check_each's two parts: the nine fixed-point products per proof with the two
affine points, and the pairing kernel itself.

usage: python tools/verify_bench.py [--batches 512,10240] [--bench-json FILE | --no-bench] [--out profiles/verify_batch.json]
                                    [--circuits 4,16] [--total 10240] [--multi-out profiles/verify_multi.json]
       python tools/verify_bench.py --each [--batches 512,10240] [--bad 1,16,256] [--each-out profiles/verify_each.json]"""
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
    ap.add_argument("--each", action="store_true", help="the localisation leg: bisection against device=True")
    ap.add_argument("--bad", default="1,16,256", help="numbers k of corrupted proofs of the localisation leg")
    ap.add_argument("--each-out", default=os.path.join(REPO, "profiles", "verify_each.json"))
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

    def each_leg(B):
        wits = [bench.witness_for(i) for i in range(B)]
        bp = BatchProver(setup, program)
        bp.upload(wits)
        bp.run()
        blob, status = bp.download_raw()
        assert not any(status)
        del bp
        pubs = [[w["x0"]] for w in wits]
        bv = BatchVerifier(vk, 1)
        seed = bytes(range(32))
        med = statistics.median

        def wall(fn):
            t0 = time.perf_counter()
            out = fn()
            return 1e3 * (time.perf_counter() - t0), out

        rows = []
        for k in [int(x) for x in args.bad.split(",") if x]:
            bad = sorted({(2 * j + 1) * B // (2 * k) for j in range(k)})
            recs = bytearray(blob)
            for i in bad:  # a_eval + 1
                e = int.from_bytes(recs[768 * i + 576 : 768 * i + 608], "little")
                recs[768 * i + 576 : 768 * i + 608] = ((e + 1) % R_MOD).to_bytes(32, "little")
            recs = bytes(recs)
            want = [i not in set(bad) for i in range(B)]
            assert bv.verify_each(recs, pubs, seed=seed, device=True) == want  # warm-up: code objects, allocations, the line tables
            sampler = ClockSampler(0)
            sampler.start()
            load_ms, bis_ms, dev_ms, fixed_ms, pair_ms, checks = [], [], [], [], [], 0
            for _ in range(5):  # the two routes alternate
                load_ms.append(wall(lambda: bv.load(recs, pubs, seed))[0])
                ms, got = wall(bv._verdicts)
                assert got == want
                bis_ms.append(ms)
                checks = bv.pairing_checks
                bv.load(recs, pubs, seed)
                ctx.profile_reset()
                ctx.profile(True)
                ms, got = wall(lambda: bv._verdicts(device=True))
                ctx.profile(False)
                assert got == want and bv.pairing_checks == 1 and bv.device_checks == B
                dev_ms.append(ms)
                fixed_ms.append(ctx.profile_read("verify_each_fixed_products")[0])
                pair_ms.append(ctx.profile_read("verify_each_pairings")[0])
            rows.append({"batch": B, "bad": len(bad), "load_ms_median_of_5": med(load_ms), "bisection_ms_median_of_5": med(bis_ms), "bisection_ms_all": bis_ms,
                         "bisection_pairing_checks": checks, "device_route_ms_median_of_5": med(dev_ms), "device_route_ms_all": dev_ms,
                         "check_each_fixed_products_ms_median_of_5": med(fixed_ms), "check_each_pairing_kernel_ms_median_of_5": med(pair_ms),
                         "check_each_pairing_kernel_ms_all": pair_ms, "device_route_over_bisection": med(dev_ms) / med(bis_ms), "clocks": sampler.summary()})
            print(json.dumps(rows[-1]), flush=True)
        return rows

    if args.each:
        each = {"group_order": n, "device": ctx.name(), "corruption": "a_eval + 1, spread evenly", "runs": []}
        for B in [int(x) for x in args.batches.split(",") if x]:
            each["runs"] += each_leg(B)
        with open(args.each_out, "w") as f:
            json.dump(each, f, indent=1)
        print(json.dumps(each))
        return

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
