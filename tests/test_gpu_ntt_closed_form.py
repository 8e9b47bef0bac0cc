"""The scalar-field transforms at 2^25 .. 2^28 on an MI355X against closed-form spectra (tests/ntt_closed_form_cases.py): the
sizes above what the C oracle can pin in seconds, and the first at which these paths can go wrong on their own —
  * 2^27 and 2^28 run on ntt_pass_radix2_kernel with the default plan (tile 2^11, three passes), which smaller sizes reach only
    through plonk_ntt_configure with toy tiles: its digit-reversing store, its two-level twiddle index and its 32-bit tile fields
    meet indices above 2^24 here for the first time;
  * 2^25 = 2^12 x 2^13 and 2^26 = 2^13 x 2^13 are the wave kernels' largest splits, 2^26 the first buffer of 2^31 bytes;
  * the fused coset forms 2^24 -> 2^26 (wave kernels) and 2^26 -> 2^28 (generic kernel): zero padding and in_scale in the first pass;
  * one batched call past 2^32 bytes, by value.
BN254: the whole output against an expected vector built on the device, itself pinned to Python integers on the sample set S(n).
BLS12-381 has no device-side operators and is checked on S(n) and on every non-zero position of its sparse vectors only.

The module runs on a context of its own and closes it at the end: the library's pass scratch (10 GiB after a 2^28 transform),
its twiddle and power tables go back to the driver before the full-size table tests that follow ask for 180 GB."""
import pytest

import ntt_closed_form_cases as cf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _own_context():
    box = {}
    yield box
    ctx = box.pop("ctx", None)
    if ctx is not None:
        ctx.close()


@pytest.fixture
def ctx(_own_context, _backend_binding):
    """The module's context, the default one for the length of a test (Polynomial and bls12_381 use the default)."""
    from plonkathon_amd import Context, backend

    if "ctx" not in _own_context:
        _own_context["ctx"] = Context()
    prev = backend._default
    backend.set_context(_own_context["ctx"])
    yield _own_context["ctx"]
    backend.set_context(prev)


@pytest.mark.parametrize("n", [1 << 28, 136 << 20], ids=["2e28", "136x2e20"])
def test_whole_vector_comparison_sees_one_element(ctx, n):
    """What step 2 of every case below rests on, at the two largest counts it is used with: both sides of the 2^32-byte line
    (element 2^27), the ends, and an index in between."""
    cf.whole_vector_comparison_sees_one_element(ctx, n, (0, (1 << 27) - 1, 1 << 27, (1 << 27) + 3 * (1 << 13) + 5, n - 1))


PLAIN = [(log_n, family, direction) for log_n in (25, 26, 27, 28) for family in ("geometric", "deltas", "periodic")
         for direction in (("fwd", "inv", "fwd_inplace") if log_n >= 27 else ("fwd", "inv"))]


@pytest.mark.parametrize("log_n,family,direction", PLAIN, ids=["%d-%s-%s" % c for c in PLAIN])
def test_bn254_ntt_closed_form(ctx, log_n, family, direction):
    """plonk_fr_ntt on its automatic plan: the wave kernels' two largest splits, and three passes of the generic kernel."""
    cf.bn254_plain(ctx, log_n, family, direction)


@pytest.mark.parametrize("log_n,how", [(25, ("split", 12)), (25, ("split", 13)), (25, ("kind", 4)), (26, ("kind", 4))],
                         ids=["25-split12", "25-split13", "25-kind4", "26-kind4"])
def test_bn254_ntt_forced_plan_equals_automatic(ctx, log_n, how):
    """2^25 as 2^12 x 2^13 and as 2^13 x 2^12; 2^25 and 2^26 on three passes of the generic kernel (kind 4)."""
    cf.bn254_forced(ctx, log_n, how)


@pytest.mark.parametrize("kind", [0, 4], ids=["auto", "kind4"])
def test_bn254_ntt_batch_past_4_gib(ctx, kind):
    """136 transforms of 2^20 in one call, 4.25 GiB: rows 127 and 128 sit on the two sides of the 2^32-byte line."""
    cf.bn254_batched(ctx, 20, 136, (0, 1, 127, 128, 135), kind)


@pytest.mark.parametrize("log_n", [24, 26])
def test_bn254_coset_forms_closed_form(ctx, log_n):
    """to_coset_extended_lagrange and back: 2^24 -> 2^26 on the wave kernels, 2^26 -> 2^28 on the generic kernel."""
    cf.bn254_coset(log_n)


@pytest.mark.parametrize("log_n", [25, 26])
def test_bls12_381_ntt_closed_form(ctx, log_n):
    cf.bls_deltas(log_n)


def test_bls12_381_coset_forms_closed_form(ctx):
    """2^24 -> 2^26 and back; the Lagrange values come from a forward transform at 2^24, a size
    test_bls12_381_ntt_exact_at_microbench_sizes pins bit for bit."""
    cf.bls_coset(24)
