"""The fixtures of the failing-column tests, held to LAPACK on the CPU (tests/failcol_ref.py): a matrix built to fail at
column k does fail there -- for dpotrf(lower=1) and for oracle.potrf_lower alike -- with a gap, a pivot and an earlier
diagonal that leave the device no room for another answer.  The GPU tests (test_failed_column_gpu.py, the group `panel`
of test_dev_ops.py, the worlds of test_dist_cpp.py) assert the same of every fixture they use before they ask the device.
"""
import numpy as np
import pytest

import failcol_ref as fr
from test_potrf_plan import driver, from_env  # noqa: F401  (the fixture that builds tests/potrf_plan_driver.cpp)

TABLE_N = 1300
TABLE_K = (1, 2, 16, 17, 127, 128, 129, 256, 257, 384, 385, 512, 513, 640, 1024, 1025, 1153, 1299, 1300)
LDL_W, LDL_K = 512, (0, 15, 16, 127, 128, 300, 511)


def test_drillholes_fail_at_the_chosen_column():
    """N = 1300, all 19 columns: LAPACK info == k, gap >= 1e-5, failing pivot <= -0.1, earlier diag(L) >= 1e-3"""
    _X, _y, K = fr.drill_gram(TABLE_N)
    gaps = []
    for k in TABLE_K:
        sn2, f = fr.drill_case(TABLE_N, k)          # asserts the four rules
        assert sn2 < 0 and f["info"] == k
        assert f["pivot"] <= -0.9 and f["min_diag"] >= 0.2, (k, f)      # what was measured when the table was made
        gaps.append(f["gap"])
        print(f"k={k}: sn2={sn2:.17g} gap={f['gap']:.3g} pivot={f['pivot']:.4f} min diag={f['min_diag']:.3g}")
    assert min(gaps) >= 3e-4 and max(gaps) == 1.0
    # the device's K differs by 1e-13 relative in DIRECT mode: orders of magnitude inside the smallest gap
    assert min(gaps) >= 1e9 * 1e-13


def test_sn2_is_monotone_and_one_below_succeeds():
    """interlacing: s grows with k; and with s just above lam(k) the k-minor is still positive definite"""
    _X, _y, K = fr.drill_gram(TABLE_N)
    s = [-fr.sn2_failing_at(K, k)[0] for k in TABLE_K]
    assert all(a < b for a, b in zip(s, s[1:]))
    k = 129
    sn2, gap = fr.sn2_failing_at(K, k)
    lam_k = -sn2 * 2 / (2 - gap)                      # s = lam(k) (1 - gap / 2)
    B = fr.b_matrix(K[:k, :k], -lam_k * (1 + 1e-6))
    assert fr.reference_info(B) == 0


@pytest.mark.parametrize("n,ks", [(700, (129, 257, 385, 600, 700)), (500, (130, 300, 500)), (600, (300,)), (900, (300,))])
def test_the_smaller_sets_of_the_distributed_worlds(n, ks):
    for k in ks:
        sn2, f = fr.drill_case(n, k)
        assert f["info"] == k and f["gap"] >= 6e-4, (n, k, f)


def test_ldl_panel_fails_at_k_plus_one():
    """A = L D L^T with D[k] = -1; an exact zero pivot; a NaN on the diagonal"""
    L = fr.ldl_factor(LDL_W, 1)
    for k in LDL_K:
        for d in (-1.0, 0.0, np.nan):
            f = fr.assert_ldl_discriminates(fr.ldl_panel(L, k, d), k, d)
            assert f["info"] == k + 1


def test_two_clusters_want_the_minimum():
    c = fr.two_clusters()
    assert c["k"] == 200 and c["facts"]["info"] == 200
    assert c["k2"] == 549                              # the second cluster fails on its own, at a LATER global column
    B = fr.b_matrix(c["K"], c["sn2"])
    assert (B[300:, :300] == 0.0).all()
    assert fr.reference_info(B[:300, :300]) == 200 and fr.reference_info(B[300:, 300:]) == 249


def test_three_tier_schedule_of_the_gpu_test(driver):
    """The scaled three-tier row of test_failed_column_gpu.py: all three widths occur at N = 2900, and the chosen columns
    are the first and the last of the wide panels and the first of the narrow panel behind them."""
    sched, caps, bw = from_env(fr.THREE_TIER_ENV)
    Np = (fr.THREE_TIER_N + 127) // 128 * 128
    plan = driver([Np], sched, caps, bw)[Np]
    assert [s["W"] for s in plan] == fr.THREE_TIER_WIDTHS
    first = {s["J"] + 1: s["W"] for s in plan}
    last = {s["J"] + s["W"]: s["W"] for s in plan}
    assert [first.get(k) or -last.get(k) for k in fr.THREE_TIER_KS] == [1024, -1024, 768, -768, 256]
