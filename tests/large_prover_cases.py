"""Bodies of the lock-step prover's tests above 2^12 and of the segmented per-proof scans (csrc/prover_scans.h): shared by
tests/test_gpu_prover_large.py (MI355X) and tests/test_emu_prover_segments.py (emulated kernels, fpl.h's range assertions)."""
import ctypes
import random

from helpers import R_MOD, load, pt

import plonkathon_amd as pa
from parity_cases import (CHAIN_X0S, DISPATCH_BATCHES, PTAU, affine, assert_chain_proof_0, chain_batch, chain_lines,  # noqa: F401
                          chain_prove_raw, flat, product_tau_setup, proofs_verify_and_reject)
from plonkathon_amd._lib import check
from oracle import field as ofield, g1 as og1
from oracle.srs import TEST_TAU

ERR_ARG = -1
# (n, S): segments of 16 rows, of one wave, of 2 048 rows; the largest S; the LDS-kernel order 2^6
FORCED_SEGMENTS = ((64, 2), (64, 4), (128, 8), (512, 8), (512, 32), (4096, 2), (4096, 16), (4096, 256))


def seg_option(k):
    """PLONK_PROVER_SEGMENTS_LOG2(k) of include/plonk_hip.h."""
    return ((k + 1) & 15) << 8


def plan_segments(log_n, B, ctx=None):
    ctx = ctx or pa.get_context()
    out = ctypes.c_uint(0)
    check(ctx.L.plonk_prover_plan_segments(ctx.handle, log_n, B, ctypes.byref(out)))
    return out.value


def forced_segments_equal_one_workgroup(setup, n, S, B=7, reference=None):
    """B of the CHAIN_X0S witnesses with the scans cut into S segments: the bytes of the S = 1 run (`reference`, or proved here),
    every status 0, proof 0 the oracle's where a fixture or the live oracle covers it."""
    if reference is None:
        reference, status = chain_prove_raw(setup, n, B, segments=1)
        assert status == bytes(B), list(status)
    blob, status = chain_prove_raw(setup, n, B, segments=S)
    assert status == bytes(B), (n, S, list(status))
    assert len(blob) == 768 * B
    for i in range(B):
        assert blob[768 * i:768 * (i + 1)] == reference[768 * i:768 * (i + 1)], (n, S, i)
    assert_chain_proof_0(n, blob[:768])
    return reference


def large_fixture_case(name):
    """A case of tests/golden/oracle_proofs_large.json (tools/gen_oracle_proofs_large.py)."""
    return {c["name"]: c for c in load("oracle_proofs_large.json")["cases"]}[name]


def large_expected_proof_0(n):
    proof = large_fixture_case("chain_%d_x0_3" % n)["proof"]
    return {k: pt(v) if isinstance(v, list) else int(v) for k, v in proof.items()}


def large_fixture_batch(setup, n, copies=3):
    """A batch of `copies` of the fixture's witness: every proof and its six challenges are the oracle's."""
    case = large_fixture_case("chain_%d_x0_3" % n)
    assert case["group_order"] == n and int(case["srs_tau"]) == TEST_TAU
    program, wits = chain_batch(n)[:2]
    assert wits[0]["x0"] == int(case["start"]["x0"])
    bp = pa.BatchProver(setup, program)
    want = large_expected_proof_0(n)
    for b, proof in enumerate(bp.prove_batch([dict(wits[0]) for _ in range(copies)])):
        assert flat(proof) == want, (n, b)
        for k, v in bp.challenges(b).items():
            assert str(v.n) == case["challenges"][k], (n, b, k)


def same_bytes(blob, status, reference, B, tag):
    """B records of the cycled seven witnesses: record i is record i mod 7 of `reference` (the default run of seven)."""
    assert status == bytes(B), (tag, [i for i, s in enumerate(status) if s])
    assert len(blob) == 768 * B and len(reference) == 768 * 7
    for i in range(B):
        assert blob[768 * i:768 * (i + 1)] == reference[768 * (i % 7):768 * (i % 7 + 1)], (tag, i)


def corrupted_cell_status(setup, n, S, cells):
    """The chain circuit's first len(cells) + 1 witnesses uploaded as wire COLUMNS (plonk_prover_upload_witness), proof i with the
    A cell of row cells[i] raised by one, the last proof intact: the status bytes."""
    program, wits = chain_batch(n)[:2]
    bp = pa.BatchProver(setup, program, segments=S)
    B = len(cells) + 1
    cols = [bp.wire_columns(wits[i]) for i in range(B)]
    for i, row in enumerate(cells):
        cols[i][0][row] = (cols[i][0][row] + 1) % R_MOD
    le = lambda v: b"".join(int(x).to_bytes(32, "little") for x in v)
    abc = b"".join(le(cols[b][k]) for k in range(3) for b in range(B))
    pub = b"".join(le([wits[b]["x0"]]) for b in range(B))
    bp.upload_raw(abc, pub, B)
    bp.run()
    return bp.download_raw()[1]


def grand_product_vs_integers(log_n, seed=1600):
    """plonk_fr_grand_product against Z_{i+1} = Z_i num_i / den_i in Python integers (ratio 0 where den_i = 0), zero denominators
    planted at row 0, row n - 1 and both sides of every boundary of the automatic segmentation, or, where that is S = 1, of the
    boundaries of the one workgroup's lane chunks (per = max(n / 256, 1) rows each) before lanes 1, 128 and 255, where those rows
    exist; then once more without them, with sigma = the identity permutation's columns, so that the product closes: out_closes both
    ways.  Returns S."""
    ctx = pa.get_context()
    n = 1 << log_n
    S = plan_segments(log_n, 1)
    rng = random.Random(seed + log_n)
    w = ofield.root_of_unity(n)
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * w % R_MOD
    beta, gamma = rng.randrange(1, R_MOD), rng.randrange(R_MOD)
    from plonkathon_amd.field import le32

    def run(A, B, C, S1, S2, S3):
        dev = [ctx.upload_ints(v) for v in (A, B, C, S1, S2, S3)]
        out, closes = ctx.alloc(n), ctypes.c_int(-1)
        check(ctx.L.plonk_fr_grand_product(ctx.handle, *[d.ptr for d in dev], log_n, le32(beta), le32(gamma), out.ptr, ctypes.byref(closes)))
        return ctx.download_ints(out), closes.value

    def expect(A, B, C, S1, S2, S3):
        # every ratio through ONE inversion: prefix products of the non-zero denominators (Montgomery's trick)
        num = [(A[i] + beta * roots[i] + gamma) * (B[i] + 2 * beta * roots[i] + gamma) * (C[i] + 3 * beta * roots[i] + gamma) % R_MOD for i in range(n)]
        den = [(A[i] + beta * S1[i] + gamma) * (B[i] + beta * S2[i] + gamma) * (C[i] + beta * S3[i] + gamma) % R_MOD for i in range(n)]
        pre, acc = [0] * n, 1
        for i in range(n):
            pre[i] = acc
            if den[i]:
                acc = acc * den[i] % R_MOD
        inv, dinv = pow(acc, -1, R_MOD), [0] * n
        for i in range(n - 1, -1, -1):
            if den[i]:
                dinv[i] = inv * pre[i] % R_MOD
                inv = inv * den[i] % R_MOD
        Z = [1]
        for i in range(n):
            Z.append(Z[-1] * num[i] % R_MOD * dinv[i] % R_MOD)
        return Z[:n], Z[n] == 1, den

    vec = lambda: [rng.randrange(R_MOD) for _ in range(n)]
    A, B, C, S1, S2, S3 = (vec() for _ in range(6))
    L = n // S
    planted = {0, n - 1} | {s * L - 1 for s in range(1, S)} | {s * L for s in range(1, S)}
    if S == 1:
        per = max(n // 256, 1)
        planted |= {r for t in (1, 128, 255) for r in (per * t - 1, per * t) if r < n}
    planted = sorted(planted)
    for i in planted:
        A[i] = (-(beta * S1[i] + gamma)) % R_MOD
    Z, closes_want, den = expect(A, B, C, S1, S2, S3)
    assert [i for i in range(n) if den[i] == 0] == planted and not closes_want
    got, closes = run(A, B, C, S1, S2, S3)
    assert got == Z, ("grand product", log_n, next(i for i in range(n) if got[i] != Z[i]))
    assert closes == 0
    # the identity permutation: num_i == den_i, every Z_i == 1, the product closes
    S1, S2, S3 = roots, [2 * r % R_MOD for r in roots], [3 * r % R_MOD for r in roots]
    A, B, C = vec(), vec(), vec()
    got, closes = run(A, B, C, S1, S2, S3)
    assert got == [1] * n and closes == 1
    return S


def device_tau_setup(n_powers, tau=TEST_TAU, spot_checks=8):
    """plonkathon_amd.Setup of tau^i G, i < n_powers, the points from plonk_g1_mul_many on the device; `spot_checks` random powers
    are checked against the Python group law (oracle.g1.multiply)."""
    from plonkathon_amd.field import Fq
    from oracle.srs import Setup as OSetup

    ctx = pa.get_context()
    scalars = bytearray(32 * n_powers)
    t = 1
    for i in range(n_powers):
        scalars[32 * i:32 * i + 32] = t.to_bytes(32, "little")
        t = t * tau % R_MOD
    base = og1.G1[0].to_bytes(32, "little") + og1.G1[1].to_bytes(32, "little")
    out, ident = ctypes.create_string_buffer(64 * n_powers), ctypes.create_string_buffer(n_powers)
    check(ctx.L.plonk_g1_mul_many(ctx.handle, base * n_powers, bytes(scalars), n_powers, out, ident))
    assert ident.raw == bytes(n_powers)
    raw = out.raw
    pts = [(int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little")) for i in range(n_powers)]
    rng = random.Random(n_powers)
    for i in rng.sample(range(n_powers), spot_checks):
        assert pts[i] == og1.multiply(og1.G1, pow(tau, i, R_MOD)), i
    x2 = OSetup.from_tau(tau, 1).X2
    return pa.Setup(powers_of_x=[(Fq(x), Fq(y)) for x, y in pts], X2=(pa.kzg.Fq2(x2[0]), pa.kzg.Fq2(x2[1])))


def segment_option_refusals(setup):
    """set_options: S with n / S < 16, k = 9 (S = 512) and a stray bit are PLONK_ERR_ARG; the valid neighbours are accepted."""
    program = chain_batch(128)[0]
    bp = pa.BatchProver(setup, program)
    L = bp.ctx.L
    assert L.plonk_prover_set_options(bp._h, seg_option(3)) == 0          # 128 / 8 = 16 rows
    assert L.plonk_prover_set_options(bp._h, seg_option(4)) == ERR_ARG    # 8 rows
    assert L.plonk_prover_set_options(bp._h, seg_option(9)) == ERR_ARG    # S = 512
    assert L.plonk_prover_set_options(bp._h, seg_option(0) | 2) == ERR_ARG
    assert L.plonk_prover_set_options(bp._h, 1 << 12) == ERR_ARG
    assert L.plonk_prover_set_options(bp._h, seg_option(1) | 1) == 0      # with PLONK_PROVER_LAGRANGE_COMMITS
    assert L.plonk_prover_set_options(bp._h, 0) == 0
    import pytest

    with pytest.raises(ValueError):
        pa.BatchProver(setup, program, segments=3)
    with pytest.raises(Exception):
        pa.BatchProver(setup, program, segments=16)


def plan_is_one_for_benchmarked_shapes():
    """The automatic rule keeps one workgroup per proof for every shape bench.py and the tests up to 2^12 run."""
    shapes = [(10, 512), (11, 512), (11, 20), (12, 300)]
    shapes += [(n.bit_length() - 1, row[0]) for n, rows in DISPATCH_BATCHES.items() for row in rows]
    for log_n, B in shapes:
        assert plan_segments(log_n, B) == 1, (log_n, B)
