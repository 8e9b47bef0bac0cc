"""The 8-rank launch contract on real kernels: `bench.py --gpus 8` as eight real processes that share the
one GPU of the test box (socket transport instead of RCCL, which needs a device per rank), the library's default 4 GiB
table budget per process — launch, rendezvous, proof-index sharding, per-rank proving and the final gather are the ones
the driver's 8-GPU run uses; only the transport of the 768-byte records differs.  The 512 gathered proofs (BASELINE
configs[4]: 8 x 64) must be byte-identical to the same 512 witnesses proved as one lock-step batch in this process."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_eight_processes_share_the_gpu_and_gather_512_proofs(tmp_path):
    dump = tmp_path / "proofs.bin"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--dist-backend", "sockets", "--steps", "1", "--warmup", "0",
           "--batch", "64", "--batches-per-step", "1", "--streams", "1", "--lookup-budget-gb", "4", "--full", "--no-cpu-baseline",
           "--no-microbench", "--no-fallbacks", "--no-end-to-end", "--no-configs", "--no-latency", "--dump-proofs", str(dump),
           "--detail", str(tmp_path / "detail.json")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    cfg = json.load(open(tmp_path / "detail.json"))["config"]
    assert line["n_gpus"] == 8 and line["config"]["ranks_in_communicator"] == 8
    assert line["config"]["sampled_proofs_verify"] is True  # four random proofs of the 512 under the pairing check
    assert cfg["results_gathered_per_step"] == 512 and cfg["gather_in_timed_region"]
    assert cfg["msm_table_bits"] == 15  # the 4 GiB budget: the comb of 15 teeth, 2.1 GB per process
    blob = dump.read_bytes()
    assert len(blob) == 512 * 768

    sys.path.insert(0, REPO)
    import bench
    from plonkathon_amd import BatchProver, Program, Setup

    setup = Setup.from_file(bench.PTAU)
    program = Program(bench.chain_program_lines(bench.GROUP_ORDER), bench.GROUP_ORDER)
    bp = BatchProver(setup, program)
    bp.upload([bench.witness_for(i) for i in range(512)])
    bp.run()
    raw, status = bp.download_raw()
    assert not any(status)
    assert raw == blob


def _bench(extra, timeout=1500, env_extra=None):
    """-> (the stdout line, the detail record): the line is the short contract form, everything else is in the detail."""
    import tempfile

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "detail.json")
        cmd = [sys.executable, os.path.join(REPO, "bench.py")] + extra + ["--full", "--detail", path]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-3000:]
        detail = json.load(open(path))
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    # the contract: ONE JSON line on stdout and nothing else (librccl's own banner goes to stderr: bench.py points fd 1 there while
    # the communicator is created), short enough for the driver's record to keep all of it
    assert len(lines) == 1 and lines[0].startswith("{") and len(lines[0]) < 4096, r.stdout[-2000:]
    return json.loads(lines[0]), detail


SHORT = ["--no-cpu-baseline", "--no-microbench", "--no-fallbacks", "--no-end-to-end", "--no-configs", "--no-latency"]


@pytest.mark.gpu
def test_one_rank_rccl_in_a_process_that_never_imports_torch():
    """the process the driver's 8-GPU run starts — bench.py, no PyTorch, the ROCm installation's own librccl,
    ncclCommInitRank — executed on hardware with one rank: `--force-comm` puts the device-resident gather
    (plonk_gather_proofs_device -> ncclAllGather), the max over ranks (ncclAllReduce) and the barrier inside the timed region.
    A fresh subprocess: pytest's own process has torch (and torch's bundled librccl) mapped, this one must not."""
    line, detail = _bench(["--gpus", "1", "--force-comm", "--steps", "2", "--warmup", "1", "--batch", "64", "--batches-per-step", "4", "--streams", "2",
                           "--lookup-budget-gb", "4"] + SHORT)
    cfg = detail["config"]
    assert cfg["gather_transport"] == "rccl" and cfg["gather_in_timed_region"] and cfg["ranks_in_communicator"] == 1
    assert cfg["gather_path"].startswith("device buffers")
    assert cfg["torch_imported"] is False
    assert "torch" not in cfg["rccl_path"] and os.path.basename(cfg["rccl_path"]).startswith("librccl.so"), cfg["rccl_path"]
    assert cfg["rccl_version"].split(".")[0].isdigit() and cfg["rccl_version"] != "0.0.0"
    # the RCCL calls really were issued: one all-gather per step (3 with the warm-up), the barriers / max over ranks (all-reduce)
    # around the timed region and the exchange of the per-rank figures (all-gather through host buffers)
    assert cfg["rccl_calls_issued"] >= 3 + 3
    pr = detail["per_rank"]
    assert len(pr["proofs_per_s"]) == 1 and pr["allgather_us_per_step"][0] > 0
    assert pr["allgather_fraction_of_step"] < 0.05
    assert cfg["results_gathered_per_step"] == 256 and line["value"] > 0
    print("rccl:", cfg["rccl_path"], cfg["rccl_version"], "all-gather us/step:", pr["allgather_us_per_step"])


@pytest.mark.gpu
def test_an_explicit_rccl_path_is_honoured_and_a_wrong_one_fails_loudly():
    _, detail = _bench(["--gpus", "1", "--force-comm", "--steps", "1", "--warmup", "0", "--batch", "8", "--batches-per-step", "1", "--streams", "1",
                        "--log-n", "6", "--no-lookup"] + SHORT, env_extra={"PLONK_RCCL_LIB": "/opt/rocm/lib/librccl.so.1"})
    assert os.path.realpath(detail["config"]["rccl_path"]) == os.path.realpath("/opt/rocm/lib/librccl.so.1")
    env = dict(os.environ, PLONK_RCCL_LIB="/nonexistent/librccl.so.1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--force-comm", "--steps", "1", "--warmup", "0", "--batch", "8",
                        "--batches-per-step", "1", "--streams", "1", "--log-n", "6", "--no-lookup"] + SHORT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "librccl could not be loaded" in r.stderr


@pytest.mark.gpu
def test_dress_rehearsal_eight_ranks_at_the_default_batch():
    """`bench.py --gpus 8` with the bench's DEFAULT step (20 lock-step batches of 512 per rank; 4 streams) as
    eight processes on the one GPU (sockets transport, the library's 4 GiB table budget per process: 8 x ~25 GB of HBM).  The
    eight ranks share one chip, so their summed rate is bounded by the single-process rate on the same budget; what the
    driver's time-slicing of eight processes' queues costs on top was measured at 21 % (22.5 k against 28.5 k proofs/s, every
    rank within 2.5 % of the others: profiles/r04_b_pytest_gpu.log) — the bound below is what a per-rank defect (a rank that
    stalls, serialised table builds, a gather that scales with the rank count) would break, not a performance target."""
    # (four streams on four hardware queues per process, as in round 3: eight processes with the bench's default of twenty queues
    # each would put 160 queues on the one GPU, and what is measured then is the queue scheduler — 0.69 in session q)
    common = ["--steps", "2", "--warmup", "1", "--lookup-budget-gb", "4", "--streams", "4", "--hw-queues", "4", "--verify-samples", "0"] + SHORT
    one, _ = _bench(["--gpus", "1"] + common)
    eight, detail = _bench(["--gpus", "8", "--dist-backend", "sockets"] + common, timeout=2400)
    cfg = detail["config"]
    assert eight["n_gpus"] == 8 and cfg["ranks_in_communicator"] == 8 and cfg["lockstep_batch"] == 512 and cfg["batches_per_step"] == 20
    assert cfg["results_gathered_per_step"] == 8 * 10240 and cfg["msm_table_bits"] == 15
    pr = detail["per_rank"]
    assert len(pr["proofs_per_s"]) == 8 and len(pr["msm_table_build_s"]) == 8 and len(eight["per_rank"]["proofs_per_s"]) == 8
    ratio = eight["value"] / one["value"]
    print("8 ranks on one GPU: %.0f proofs/s; one process: %.0f; ratio %.3f; per rank min/max %.0f / %.0f"
          % (eight["value"], one["value"], ratio, pr["proofs_per_s_min"], pr["proofs_per_s_max"]))
    assert 0.6 <= ratio <= 1.1, ratio  # (0.79 on the window tables; 0.69 with the comb tables' extra launch per MSM call and longer Horner step: r05_n)
    assert pr["proofs_per_s_min"] >= 0.8 * pr["proofs_per_s_max"]  # no straggler


@pytest.mark.gpu
def test_headline_configuration_is_bit_identical_to_the_bucket_method():
    """what bench.py's line is measured on — eight contexts on eight hardware queues, bench.py's table budget (180 GB: the comb
    of 21 teeth with top tables), one workgroup per MSM, sixteen lock-step batches of 512 distinct witnesses in flight together — with EVERY one of
    the 8 192 proofs compared byte for byte with the bucket method's, the step run twice, proofs 0 / 1 against the fixtures and four
    under the pairing check (tests/headline_config_check.py; a subprocess because GPU_MAX_HW_QUEUES is read when the runtime starts)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "headline_config_check.py"), "8", "2", "512"], env=env,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["contexts"] == 8 and out["hw_queues"] == 8 and out["comb_teeth"] == 21 and out["comb_columns"] == 12 and out["top_group"] == 7 and out["table_bytes"] == (2048 + 300) * (1 << 20) * 64
    assert out["proofs"] == 8192 and out["identical_to_bucket_method"] == 8192 and out["fixtures"] == 2 and len(out["pairing_checked"]) == 4
    print("headline configuration:", out)


@pytest.mark.gpu
def test_a_killed_rank_of_eight_stops_the_job_within_seconds():
    """VERDICT r05 #1 on real kernels: eight processes on the one GPU (sockets transport), rank 5 is SIGKILLed between enqueueing its
    batches and the gather of timed step 1.  The launcher names it; the other ranks give up on their own (PeerLost, exit code 76) or
    are stopped; nothing waits for a timeout."""
    import time

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--dist-backend", "sockets", "--steps", "3", "--warmup", "1",
                        "--batch", "64", "--batches-per-step", "2", "--streams", "2", "--hw-queues", "4", "--lookup-budget-gb", "4", "--comm-timeout", "20",
                        "--inject-fault", "5:1:kill"] + SHORT, env=env, capture_output=True, text=True, timeout=900)
    took = time.monotonic() - t0
    assert r.returncode != 0 and not r.stdout.strip(), (r.returncode, r.stdout[-500:])
    assert "rank 5 of 8 was killed by SIGKILL first" in r.stderr, r.stderr[-4000:]
    assert "PeerLost" in r.stderr  # rank 0 lost rank 5 and said so
    print("killed rank named after %.1f s" % took)
    assert took < 240, took  # (eight start-ups and table builds on one GPU; the failure itself is seen within a second)


@pytest.mark.gpu
def test_comm_init_has_a_deadline_on_real_rccl(tmp_path):
    """ncclCommInitRank for rank 0 of TWO with nobody playing rank 1: plonk_comm_create gives up after the process-wide deadline with
    PLONK_ERR_TIMEOUT and a message naming rank, world and device (before: it blocked for ever).  A subprocess, ended with os._exit:
    the helper thread is still inside RCCL."""
    script = tmp_path / "init_deadline.py"
    script.write_text(
        "import ctypes, os, sys, time\n"
        "sys.path.insert(0, %r)\n"
        "from plonkathon_amd import Context, _lib\n"
        "ctx = Context(0)\n"
        "L = ctx.L\n"
        "assert L.plonk_comm_set_default_timeout(3.0) == 0\n"
        "ident = ctypes.create_string_buffer(128)\n"
        "assert L.plonk_comm_unique_id(ident) == 0\n"
        "h = ctypes.c_void_p()\n"
        "t0 = time.monotonic()\n"
        "rc = L.plonk_comm_create(ctx.handle, ident, 0, 2, ctypes.byref(h))\n"
        "print(rc, '%%.1f' %% (time.monotonic() - t0), L.plonk_last_error().decode(), flush=True)\n"
        "os._exit(0)\n" % REPO)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rc, took, msg = r.stdout.strip().splitlines()[-1].split(" ", 2)
    assert int(rc) == -5 and 2.5 <= float(took) <= 30, r.stdout
    assert "ncclCommInitRank(rank 0 of 2, device 0) did not return within 3 s" in msg, msg


@pytest.mark.gpu
def test_preflight_on_a_one_rank_rccl_communicator():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--force-comm", "--preflight", "--batch", "64",
                        "--batches-per-step", "2", "--streams", "2", "--lookup-budget-gb", "4"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    rep = json.loads(lines[0])
    row = rep["ranks"][0]
    assert rep["preflight"] is True and rep["ranks_in_communicator"] == 1 and rep["all_peers_reachable"] is True
    assert row["transport"] == "rccl" and os.path.basename(row["rccl_path"]).startswith("librccl.so") and row["rccl_version"] != "0.0.0"
    assert row["peer_access"][row["device"]] == 1 and row["hbm_total_gb"] > 200 and 0 < row["hbm_free_gb"] <= row["hbm_total_gb"]
    assert row["msm_table"]["layout"] == "comb" and row["msm_table"]["bits"] == 15 and row["msm_table"]["build_s"] > 0
    assert row["allgather_us"] > 0 and row["allgather_measured_by"].startswith("HIP events")
    print("preflight:", row)
