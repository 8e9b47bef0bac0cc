"""MSM tests on the known-secret SRS (tests/msm_known_secret_cases.py) on the emulated kernels, at reduced sizes: 50 bases, toy
combs and window tables.  The reference itself is pinned here, without the emulator, to the C oracle's MSM."""
import random

import pytest

import msm_known_secret_cases as ks
from helpers import R_MOD

EMU_N = 50
EMU_LANES = [("comb", h, g, {"top": top, "walk": "lanes"}) for h, top in ks.EMU_COMBS for g in (1, 4)]
EMU_WIDE = [("comb", h, 1, {"top": top, "walk": "lanes", "wide": True}) for h, top in ks.EMU_COMBS]
EMU_ROWS = [("comb", h, c, {"top": top, "walk": "rows"}) for h, top in ks.EMU_COMBS for c in (1, 2, 3)]
EMU_METHODS = ks.BUCKET + [("windows", 4, 0, {})] + EMU_LANES + EMU_WIDE + EMU_ROWS + ks.AUTO  # (auto: the bucket method, no GPU)


def test_reference_matches_the_c_oracle():
    """`expected` — a dot product with the powers of the secret and one scalar multiplication — against c_oracle.g1_lincomb over the
    oracle's own SRS of that secret, at n = 300: a uniform vector, a 0/1 vector and the designed identity."""
    from oracle import c_oracle
    from parity_cases import oracle_tau_setup

    n = 300
    pts = oracle_tau_setup(ks.TAU, n).powers_of_x
    rng = random.Random(300)
    head = [rng.randrange(R_MOD) for _ in range(n - 1)]
    for name, sc in (("uniform", head + [rng.randrange(R_MOD)]), ("bits", [rng.randrange(2) for _ in range(n)]),
                     ("designed identity", ks.designed(head, 0, n)), ("designed G", ks.designed(head, 1, n))):
        want = c_oracle.g1_lincomb(pts, sc)
        assert ks.expected(sc) == want, name
        if name.startswith("designed"):
            assert want == (None if name.endswith("identity") else ks.og1.G1), name
    ms, pts = ks.known_points(5)
    sc = [rng.randrange(R_MOD) for _ in range(5)]
    assert ks.expected_on(ms, sc) == c_oracle.g1_lincomb(pts, sc)


@pytest.mark.parametrize("m", EMU_METHODS, ids=ks.method_id)
def test_scalar_families(emu, m):
    ks.scalar_families(m, EMU_N)


@pytest.mark.parametrize("batch", [False, True], ids=["alone", "row 1 of 3"])
@pytest.mark.parametrize("negate", [False, True], ids=["equal", "opposite"])
@pytest.mark.parametrize("site", ["rowsum", "colsum", "tree"])
def test_comb_redo_site(emu, site, negate, batch):
    getattr(ks, "redo_" + site)(negate, batch)


@pytest.mark.parametrize("batch", [False, True], ids=["alone", "row 1 of 3"])
@pytest.mark.parametrize("butterfly", [False, True], ids=["column sum", "butterfly"])
def test_comb_redo_site_horner(emu, butterfly, batch):
    ks.redo_horner(butterfly, batch)


def test_lagrange_view(emu, monkeypatch):
    """2^4 by the n-MSM route and 2^5 by the group transform (forced: it is the route of sizes above 2^12)."""
    setup = ks.tau_setup(64)
    ks.lagrange_view(setup, 4)
    monkeypatch.setenv("PLONK_LAGRANGE_SRS", "ntt")
    ks.lagrange_view(setup, 5)
