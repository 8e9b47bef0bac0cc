"""The lock-step prover from 2^13 to 2^16 rows and the segmented forms of its three per-proof scans (csrc/prover_scans.h), on an
MI355X.  Fixtures: tests/golden/oracle_proofs_large.json (tools/gen_oracle_proofs_large.py: the oracle's proofs at 2^13 and 2^14,
91 s and 184 s on one core).  2^16 has no oracle proof: it is checked by the pairing verifiers and against the S = 1 run."""
import time

import pytest

import large_prover_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ptau_setup():
    from plonkathon_amd import Setup

    return Setup.from_file(lc.PTAU)


@pytest.fixture(scope="module")
def tau_setup():
    """n -> the Setup of n powers of the test-only secret (C oracle; 8 random powers checked against the Python group law)."""
    done = {}

    def get(n):
        if n not in done:
            t0 = time.time()
            done[n] = lc.product_tau_setup(lc.TEST_TAU, n)
            print("SRS of %d powers from the test secret: %.2f s on the CPU" % (n, time.time() - t0))
        return done[n]

    return get


@pytest.fixture(scope="module")
def setup_for(ptau_setup, tau_setup):
    return lambda n: ptau_setup if n <= 2048 else tau_setup(n)


@pytest.fixture(scope="module")
def one_workgroup_reference(setup_for):
    """n -> the 7 x 768 bytes of the CHAIN_X0S proofs with S forced to 1, proved once per n."""
    done = {}

    def get(n):
        if n not in done:
            blob, status = lc.chain_prove_raw(setup_for(n), n, segments=1)
            assert status == bytes(7), list(status)
            done[n] = blob
        return done[n]

    return get


# ---- forced segments at the smallest shapes that can break them ----------------------------------------------------------------
@pytest.mark.parametrize("n,S", lc.FORCED_SEGMENTS)
def test_forced_segments_equal_one_workgroup(setup_for, one_workgroup_reference, n, S):
    lc.forced_segments_equal_one_workgroup(setup_for(n), n, S, reference=one_workgroup_reference(n))


def test_failure_flags_survive_segmentation(ptau_setup):
    """One wire cell off by one, in the last row of segment 0 of proof 0 and in row 0 of the last segment of proof 1 (n = 512,
    S = 8: 64 rows per segment); proof 2 is intact.  The status bytes are those of S = 1 and have bit 1 (Z open) set."""
    n, S = 512, 8
    cells = [n // S - 1, n - n // S]
    want = lc.corrupted_cell_status(ptau_setup, n, 1, cells)
    got = lc.corrupted_cell_status(ptau_setup, n, S, cells)
    assert got == want, (list(got), list(want))
    assert got[0] & 2 and got[1] & 2 and got[2] == 0, list(got)


def test_segment_options_are_checked(ptau_setup):
    lc.segment_option_refusals(ptau_setup)


def test_plan_leaves_the_benchmarked_shapes_alone():
    lc.plan_is_one_for_benchmarked_shapes()


@pytest.mark.parametrize("log_n", [14, 16])
def test_grand_product_segmented_vs_integers(log_n):
    assert lc.plan_segments(log_n, 1) > 1  # these calls do take the segmented form
    assert lc.grand_product_vs_integers(log_n) > 1


@pytest.mark.parametrize("log_n", [5, 8, 10])
def test_grand_product_one_workgroup_vs_integers(log_n):
    """S = 1: fewer rows than lanes (idle lanes carry the neutral element), one row per lane, four rows per lane."""
    assert lc.plan_segments(log_n, 1) == 1
    assert lc.grand_product_vs_integers(log_n) == 1


# ---- 2^13 and 2^14 against the oracle's proofs -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_reference(setup_for):
    """n -> the seven CHAIN_X0S records on the default dispatcher, table choice and segmentation; proof 0 is the oracle's."""
    done = {}

    def get(n):
        if n not in done:
            blob, status = lc.chain_prove_raw(setup_for(n), n)
            assert status == bytes(7), list(status)
            assert lc.flat(lc.pa.BatchProver.decode(blob[:768])) == lc.large_expected_proof_0(n)
            assert len({blob[768 * i:768 * (i + 1)] for i in range(7)}) == 7
            done[n] = blob
        return done[n]

    return get


@pytest.mark.parametrize("n", [8192, 16384])
def test_large_orders_fixture(setup_for, n):
    """A batch of three copies: the oracle's proof and its six challenges."""
    lc.large_fixture_batch(setup_for(n), n, copies=3)


@pytest.mark.parametrize("n", [8192, 16384])
def test_large_orders_lagrange_commits(setup_for, default_reference, n):
    """PLONK_PROVER_LAGRANGE_COMMITS: above 2^12 the Lagrange-basis SRS comes from the transform over the group."""
    blob, status = lc.chain_prove_raw(setup_for(n), n, lagrange_commits=True)
    lc.same_bytes(blob, status, default_reference(n), 7, ("lagrange", n))


@pytest.mark.parametrize("n", [8192, 16384])
def test_large_orders_bucket_method(setup_for, default_reference, n):
    from plonkathon_amd import Context

    c = Context(0)
    c.msm_lookup(1)
    blob, status = lc.chain_prove_raw(setup_for(n), n, ctx=c)
    assert setup_for(n).device_bases(c).lookup_info()["layout"] is None
    lc.same_bytes(blob, status, default_reference(n), 7, ("bucket", n))


@pytest.mark.parametrize("S", [1, 4, 64])
@pytest.mark.parametrize("n", [8192, 16384])
def test_large_orders_forced_segments(setup_for, default_reference, n, S):
    blob, status = lc.chain_prove_raw(setup_for(n), n, segments=S)
    lc.same_bytes(blob, status, default_reference(n), 7, ("segments", n, S))


@pytest.mark.parametrize("B", [1, 7, 24])
def test_2_14_batches_across_the_latency_threshold(setup_for, default_reference, B):
    """The wire transforms run as 3 B vectors per call and take the latency forms while 3 B <= 16: B = 1 on the latency forms, 7
    mixed (wires full, Z and the quotient rows latency), 24 on the full forms."""
    n = 16384
    blob, status = lc.chain_prove_raw(setup_for(n), n, B)
    lc.same_bytes(blob, status, default_reference(n), B, ("batch", B))


@pytest.mark.parametrize("n", [8192, 16384])
def test_large_orders_proofs_verify(setup_for, n):
    """A second witness under the oracle's pairing check and the product's; a flipped evaluation bit and a wrong public input fail."""
    lc.proofs_verify_and_reject(setup_for(n), lc.chain_lines(n), n, {"x0": 0xDEADBEEF12345}, ["x0"])


# ---- 2^16: the documented maximum ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_2_16():
    """SRS of 2^16 powers from the device's scalar multiplication, the compiled chain program, two witnesses, their records on the
    automatic segmentation.  The construction times are printed."""
    n = 1 << 16
    t0 = time.time()
    setup = lc.device_tau_setup(n)
    t1 = time.time()
    program = lc.pa.Program(lc.chain_lines(n), n)
    wits = [program.fill_variable_assignments({"x0": x0}) for x0 in (3, 0xDEADBEEF12345)]
    t2 = time.time()
    bp = lc.pa.BatchProver(setup, program)
    S = bp.segments_for(2)
    bp.upload(wits)
    bp.run()
    blob, status = bp.download_raw()
    t3 = time.time()
    print("2^16: SRS %.2f s, program and witnesses %.2f s, prover construction and two proofs %.2f s, S = %d" % (t1 - t0, t2 - t1, t3 - t2, S))
    assert status == bytes(2), list(status)
    return {"n": n, "setup": setup, "program": program, "wits": wits, "blob": blob, "S": S}


def test_2_16_automatic_segments_equal_one_workgroup(case_2_16):
    c = case_2_16
    assert c["S"] > 1
    bp = lc.pa.BatchProver(c["setup"], c["program"], segments=1)
    bp.upload(c["wits"])
    bp.run()
    blob, status = bp.download_raw()
    assert status == bytes(2) and blob == c["blob"]
    assert blob[:768] != blob[768:]


def test_2_16_proofs_verify(case_2_16):
    """Both proofs pass VerificationKey.verify_proof, one flipped bit fails; BatchVerifier.verify_each accepts the pair and names a
    corrupted one."""
    import copy

    from plonkathon_amd import BatchProver, BatchVerifier, Scalar

    c = case_2_16
    n, blob = c["n"], c["blob"]
    vk = c["setup"].verification_key(c["program"].common_preprocessed_input())
    proofs = [BatchProver.decode(blob[768 * i:768 * (i + 1)]) for i in range(2)]
    pubs = [[w["x0"]] for w in c["wits"]]
    for proof, pub in zip(proofs, pubs):
        assert vk.verify_proof(n, proof, pub)
    bad = copy.deepcopy(proofs[1])
    bad.msg_4.c_eval = Scalar(bad.msg_4.c_eval.n ^ (1 << 100))
    assert not vk.verify_proof(n, bad, pubs[1])
    bv = BatchVerifier(vk, 1)
    assert bv.verify_each(blob, pubs, seed=bytes(32)) == [True, True]
    corrupted = bytearray(blob)
    corrupted[768 + 576 + 5] ^= 1  # an evaluation of proof 1
    assert bv.verify_each(bytes(corrupted), pubs, seed=bytes(32)) == [True, False]


def test_2_16_api_prover_matches_batch_prover(case_2_16):
    """The reference-shaped Prover (round 2 through the segmented plonk_fr_grand_product) gives the batch prover's proof."""
    from plonkathon_amd import BatchProver, Prover

    c = case_2_16
    p1 = Prover(c["setup"], c["program"])
    p1.check = False
    assert lc.flat(p1.prove(dict(c["wits"][0]))) == lc.flat(BatchProver.decode(c["blob"][:768]))
