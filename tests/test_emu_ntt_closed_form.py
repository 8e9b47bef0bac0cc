"""tests/ntt_closed_form_cases.py without a GPU: the references checked on every index against the oracle, the comparison helper
against wrong outputs it must reject, and the bodies of tests/test_gpu_ntt_closed_form.py at 2^9 .. 2^14 on the emulated kernels."""
import random

import pytest

import ntt_closed_form_cases as cf
from oracle import c_oracle
from oracle.fr_poly import Basis as OBasis, Polynomial as OPoly, fft_ints


# ---- the references themselves, on every index --------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(cf.FAMILIES))
def test_closed_forms_equal_the_python_transform(family):
    n = 1 << 10
    fam = cf.FAMILIES[family](n, 11)
    x = fam.host_input()
    for inverse in (False, True):
        closed = fam.closed(inverse)
        assert [closed(k) for k in range(n)] == fft_ints(x, inverse), (family, inverse)


@pytest.mark.parametrize("family", list(cf.FAMILIES))
def test_closed_forms_equal_the_c_oracle(family):
    n = 1 << 12
    fam = cf.FAMILIES[family](n, 12)
    x = fam.host_input()
    for inverse in (False, True):
        closed = fam.closed(inverse)
        assert [closed(k) for k in range(n)] == c_oracle.fr_ntt(x, inverse), (family, inverse)


def test_closed_forms_over_bls12_381_equal_the_c_oracle():
    n = 1 << 10
    un = lambda raw: [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(len(raw) // 32)]
    fam = cf.Deltas(n, 13, cf.BLS_M, cf.bls_root)
    raw = b"".join(v.to_bytes(32, "little") for v in fam.host_input())
    for inverse in (False, True):
        closed = fam.closed(inverse)
        assert [closed(k) for k in range(n)] == un(c_oracle.fr_ntt_bytes(raw, inverse, "bls12_381")), inverse
    sp = cf.SparsePoly(n, 14, cf.BLS_M, cf.bls_root)
    raw = b"".join(v.to_bytes(32, "little") for v in sp.coeffs())
    lag = sp.lagrange()
    assert [lag(i) for i in range(n)] == un(c_oracle.fr_ntt_bytes(raw, False, "bls12_381"))
    # p(off mu^k): the 4n-point transform of the coefficients a_t off^(e_t), zero padded
    scaled = [v * pow(sp.off, i, cf.BLS_M) % cf.BLS_M for i, v in enumerate(sp.coeffs())] + [0] * (3 * n)
    on = sp.on_coset()
    assert [on(k) for k in range(4 * n)] == un(c_oracle.fr_ntt_bytes(b"".join(v.to_bytes(32, "little") for v in scaled), False, "bls12_381"))


def test_sparse_polynomial_on_the_coset_equals_the_oracle():
    n = 1 << 10
    sp = cf.SparsePoly(n, 15)
    lag, on = sp.lagrange(), sp.on_coset()
    v = [lag(i) for i in range(n)]
    assert v == fft_ints(sp.coeffs())
    big = OPoly(v, OBasis.LAGRANGE).to_coset_extended_lagrange(sp.off)
    assert [on(k) for k in range(4 * n)] == big.values
    back = big.coset_extended_lagrange_to_coeffs(sp.off).values
    assert back == sp.coeffs(4 * n)
    assert all(not any(back[a:b]) for a, b in sp.gaps(4 * n)) and sum(b - a for a, b in sp.gaps(4 * n)) == 4 * n - len(sp.terms)


def test_sample_set():
    for log_n in (3, 9, 12, 28):
        n = 1 << log_n
        S = cf.sample_set(n, 1)
        assert S == sorted(set(S)) and all(0 <= k < n for k in S)
        want = {0, 1, 2, 3, n - 2, n - 1} | {(1 << b) + d for b in range(1, log_n) for d in (-1, 0, 1)}
        assert want <= set(S) and len(S) <= len(want) + 32
    assert 100 <= len(cf.sample_set(1 << 28)) <= 125


# ---- the checker: wrong outputs it must reject -----------------------------------------------------------------------------
def _checker_case():
    n = 1 << 12
    fam = cf.Geometric(n, 16)
    closed = fam.closed(False)
    E = [closed(k) for k in range(n)]
    assert len(set(E)) == n  # dense, every element differs
    return n, fam, closed, E, cf.sample_set(n, 2)


def _run_checker(closed, S, E, out):
    cf.check_output("checker", S, closed, E.__getitem__, out.__getitem__, lambda: out == E)


def test_checker_accepts_the_right_output():
    n, fam, closed, E, S = _checker_case()
    _run_checker(closed, S, E, list(E))


@pytest.mark.parametrize("wrong", ["blocks_swapped", "wrapped_at_half", "off_by_one_outside_S", "wrong_root"])
def test_checker_rejects(wrong):
    n, fam, closed, E, S = _checker_case()
    out = list(E)
    rng = random.Random(17)
    if wrong == "blocks_swapped":  # two 2^6-blocks of the output swapped
        a, b = 64 * 5, 64 * 41
        out[a : a + 64], out[b : b + 64] = E[b : b + 64], E[a : a + 64]
    elif wrong == "wrapped_at_half":
        out = [E[k % (n // 2)] for k in range(n)]
    elif wrong == "off_by_one_outside_S":
        k = rng.choice([k for k in range(n) if k not in set(S)])
        out[k] = (out[k] + 1) % fam.m
        cf.check_samples("S alone misses it", S, closed, out.__getitem__)  # ... which is why the whole vector is compared
    else:  # the right spectrum of the wrong root
        w3 = pow(fam.w, 3, fam.m)
        out = [fam.numerator(False) * pow((fam.c * pow(w3, k, fam.m) - 1) % fam.m, -1, fam.m) % fam.m for k in range(n)]
    assert out != E
    with pytest.raises(AssertionError):
        _run_checker(closed, S, E, out)
    if wrong in ("wrapped_at_half", "wrong_root"):  # errors tied to a high index bit or to the root are met on S already, which is all BLS12-381 has
        with pytest.raises(AssertionError):
            cf.check_samples("checker", S, closed, out.__getitem__)


def test_checker_rejects_a_wrong_expected_vector():
    n, fam, closed, E, S = _checker_case()
    bad = list(E)
    bad[S[40]] ^= 1
    with pytest.raises(AssertionError, match="expected vector itself"):
        cf.check_output("checker", S, closed, bad.__getitem__, bad.__getitem__, lambda: True)


# ---- the GPU bodies on the emulated kernels ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _own_context():
    box = {}
    yield box
    ctx = box.pop("ctx", None)
    if ctx is not None:
        ctx.close()


@pytest.fixture
def ctx(emu, _own_context, _backend_binding):
    from plonkathon_amd import Context, backend

    if "ctx" not in _own_context:
        _own_context["ctx"] = Context()
    prev = backend._default
    backend.set_context(_own_context["ctx"])
    yield _own_context["ctx"]
    backend.set_context(prev)


def test_whole_vector_comparison_sees_one_element(ctx):
    cf.whole_vector_comparison_sees_one_element(ctx, 5000, (0, 4095, 4096, 4999))


@pytest.mark.parametrize("direction", ["fwd", "inv", "fwd_inplace"])
@pytest.mark.parametrize("family", list(cf.FAMILIES))
@pytest.mark.parametrize("log_n", [9, 14])
def test_bn254_ntt_closed_form(ctx, log_n, family, direction):
    """2^9: one pass; 2^14: two."""
    cf.bn254_plain(ctx, log_n, family, direction)


@pytest.mark.parametrize("log_n,how", [(14, ("split", 7)), (14, ("kind", 4))], ids=["14-split7", "14-kind4"])
def test_bn254_ntt_forced_plan_equals_automatic(ctx, log_n, how):
    cf.bn254_forced(ctx, log_n, how)


@pytest.mark.parametrize("kind", [0, 4], ids=["auto", "kind4"])
def test_bn254_ntt_batched(ctx, kind):
    cf.bn254_batched(ctx, 9, 6, (0, 1, 4, 5), kind)


@pytest.mark.parametrize("log_n", [9, 12])
def test_bn254_coset_forms_closed_form(ctx, log_n):
    cf.bn254_coset(log_n)


def test_bls12_381_closed_form(ctx):
    cf.bls_deltas(9)
    cf.bls_coset(9)
