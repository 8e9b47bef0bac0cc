"""MSM tests on the known-secret SRS (tests/msm_known_secret_cases.py) on an MI355X: structured scalar families at n = 300 through
every method and at n = 2048 on the bucket method and the automatic table, each comb redo site on its own, the row walk where the
library's rule takes it with every MSM checked, the bucket entry encoding at n = 32768, the Lagrange view against integers."""
import pytest

import msm_known_secret_cases as ks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", ks.METHODS, ids=ks.method_id)
def test_scalar_families(m):
    ks.scalar_families(m, 300)


@pytest.mark.parametrize("m", ks.BUCKET[:1] + ks.AUTO, ids=ks.method_id)
def test_scalar_families_full_width(m):
    ks.scalar_families(m, 2048)


@pytest.mark.parametrize("batch", [False, True], ids=["alone", "row 1 of 3"])
@pytest.mark.parametrize("negate", [False, True], ids=["equal", "opposite"])
@pytest.mark.parametrize("site", ["rowsum", "colsum", "tree"])
def test_comb_redo_site(site, negate, batch):
    getattr(ks, "redo_" + site)(negate, batch)


@pytest.mark.parametrize("batch", [False, True], ids=["alone", "row 1 of 3"])
@pytest.mark.parametrize("butterfly", [False, True], ids=["column sum", "butterfly"])
def test_comb_redo_site_horner(butterfly, batch):
    ks.redo_horner(butterfly, batch)


def test_row_walk_by_the_rule_every_msm():
    ks.row_walk_by_the_rule()


def test_bucket_entry_encoding_boundary():
    ks.bucket_entry_boundary()


@pytest.fixture(scope="module")
def setup_8192():
    from large_prover_cases import device_tau_setup

    return device_tau_setup(1 << 13, ks.TAU)


@pytest.mark.parametrize("log_n", [11, 13])
def test_lagrange_view(setup_8192, log_n):
    """2^11: the n-MSM route; 2^13: the group transform of csrc/g1_ntt.hip."""
    ks.lagrange_view(setup_8192, log_n)
