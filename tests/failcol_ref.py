"""TEST INFRASTRUCTURE (CPU only): matrices whose Cholesky factorisation fails at a CHOSEN column, and the reference
answer for the column.

For a Gram matrix K and a target column k (1-based), let lam(j) be the largest eigenvalue of the leading j x j block of
K, lam(0) = 0.  By interlacing lam is non-decreasing.  With s = (lam(k-1) + lam(k)) / 2 and sn2 = -s the matrix
B = I + K / sn2 = I - K / s has a positive definite leading (k-1)-minor (lam(k-1) < s) and an indefinite k-minor
(lam(k) > s): a Cholesky factorisation fails exactly at column k.  The device's K differs from NumPy's by 1e-13
relative (DIRECT) or 2e-7 (EXPANSION); `gap` = (lam(k) - lam(k-1)) / lam(k) says how far inside that is.

Two further constructions: a dense panel L D L^T with one entry of D made -1, 0 or NaN (`ldl_panel`), and two
drill-hole clusters so far apart that their cross-kernel is exactly 0.0 (`two_clusters`), where the second cluster
fails on its own at a later column: the answer is the MINIMUM, which a last-writer-wins report misses.

`facts` gives what every test asserts of its fixture before it asks the device: the gap, the reference's answer,
the failing pivot and the smallest diagonal entry of L before it (FIXTURE_RULES).
"""
import functools
import os
import sys

import numpy as np
import scipy.linalg as sl
from scipy.linalg import lapack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MIN_GAP, MAX_PIVOT, MIN_DIAG = 1e-5, -0.1, 1e-3        # FIXTURE_RULES: the issue's four conditions (the fourth: ref == k)


def _top(K, j):
    """largest eigenvalue of the leading j x j block (0 for j = 0)"""
    if j == 0:
        return 0.0
    return float(sl.eigvalsh(K[:j, :j], subset_by_index=[j - 1, j - 1])[0])


class Minors:
    """lam(j) of one K, each leading minor solved once"""

    def __init__(self, K):
        self.K = np.asarray(K, dtype=np.float64)
        self._lam = {}

    def lam(self, j):
        if j not in self._lam:
            self._lam[j] = _top(self.K, j)
        return self._lam[j]


_MINORS = {}


def _minors(K):
    key = id(K)
    if key not in _MINORS or _MINORS[key][0] is not K:
        _MINORS[key] = (K, Minors(K))       # holds K, so the id stays its own
    return _MINORS[key][1]


def sn2_failing_at(K, k):
    """(sn2, gap): B = I + K / sn2 fails at column k (1-based); gap = (lam(k) - lam(k-1)) / lam(k)"""
    m = _minors(K)
    lo, hi = m.lam(k - 1), m.lam(k)
    assert 0.0 <= lo < hi, (k, lo, hi)
    return float(-0.5 * (lo + hi)), (hi - lo) / hi


def b_matrix(K, sn2):
    return np.eye(K.shape[0]) + np.asarray(K, dtype=np.float64) / sn2


def reference_info(B):
    """the failing column (1-based; 0: positive definite) from LAPACK's dpotrf(lower=1) and from oracle.potrf_lower,
    the call tests/ctx_model.py uses; the two must agree.  A matrix that holds a NaN is the oracle's alone: reference
    LAPACK tests `ajj <= 0 or disnan(ajj)`, as the oracle and the device (`!(ajj > 0)`) do, but an optimised BLAS's own
    potrf may test `ajj <= 0` only, which a NaN passes."""
    from oracle import oracle as orc
    info_o = int(orc.potrf_lower(B)[1])
    if np.isnan(B).any():
        return info_o
    _c, info = lapack.dpotrf(np.asfortranarray(B), lower=1)
    assert int(info) == info_o, (int(info), info_o)
    return int(info)


def facts(B, k, gap=None):
    """What a fixture must show before the device is asked: {'gap', 'info', 'pivot', 'min_diag'}.  pivot = the k-th
    pivot from a Cholesky factor of the (k-1)-minor; min_diag = the smallest diagonal entry of that factor."""
    B = np.asarray(B, dtype=np.float64)
    out = {"gap": gap, "info": reference_info(B)}
    if k > 1:
        L = np.linalg.cholesky(B[:k - 1, :k - 1])
        v = sl.solve_triangular(L, B[:k - 1, k - 1], lower=True)
        out["pivot"] = float(B[k - 1, k - 1] - v @ v)
        out["min_diag"] = float(np.diag(L).min())
    else:
        out["pivot"], out["min_diag"] = float(B[0, 0]), np.inf
    return out


def assert_discriminates(f, k, what=""):
    """the fixture rules: a case that cannot discriminate fails here, as a test of the fixture and not of the device"""
    assert f["gap"] is None or f["gap"] >= MIN_GAP, (what, k, f)
    assert f["info"] == k, (what, k, f)
    assert not f["pivot"] > MAX_PIVOT, (what, k, f)            # a NaN pivot counts as failing
    assert f["min_diag"] >= MIN_DIAG, (what, k, f)


# ---- the training sets ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drill_gram(n, mode=1):
    """(X, y, K) of synth.drillholes(n) with the default parameters and bias: K from NumPy (exact_grad_ref.gram) in
    DIRECT mode (1), from the oracle in EXPANSION mode (0)"""
    from gp_ss_ak_amd import synth
    X, y = synth.drillholes(n)
    if mode == 1:
        import exact_grad_ref as eg
        K = eg.gram(X, [(0, list(synth.DEFAULT_EXPANS))], synth.DEFAULT_BIAS)
    else:
        from oracle import oracle as orc
        K = np.array(orc.gram(X, X, np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, orc.DIST_EXPANSION))
    K.setflags(write=False)
    return X, y, K


@functools.lru_cache(maxsize=None)
def drill_case(n, k, mode=1):
    """(sn2, facts) of the drill-hole set failing at k, the rules asserted"""
    _X, _y, K = drill_gram(n, mode)
    sn2, gap = sn2_failing_at(K, k)
    f = facts(b_matrix(K, sn2), k, gap)
    assert_discriminates(f, k, f"drillholes({n})")
    return sn2, f


CLUSTER_N, CLUSTER_SPLIT, CLUSTER_SHIFT, CLUSTER_K = 600, 300, 1e4, 200


@functools.lru_cache(maxsize=None)
def two_clusters():
    """drillholes(600) with rows 300.. shifted by 1e4 and bias 0: the cross-kernel is exactly 0.0, and the s chosen for
    k = 200 makes the second cluster alone fail as well.  Returns a dict: X, y, K, sn2, k (200), k2 (the GLOBAL column at
    which the second cluster fails on its own), facts."""
    from gp_ss_ak_amd import synth
    import exact_grad_ref as eg
    X, y = synth.drillholes(CLUSTER_N)
    X = np.array(X, order="F")
    X[CLUSTER_SPLIT:] += CLUSTER_SHIFT
    K = eg.gram(X, [(0, list(synth.DEFAULT_EXPANS))], 0.0)
    assert (K[CLUSTER_SPLIT:, :CLUSTER_SPLIT] == 0.0).all()
    sn2, gap = sn2_failing_at(K, CLUSTER_K)
    B = b_matrix(K, sn2)
    f = facts(B, CLUSTER_K, gap)
    assert_discriminates(f, CLUSTER_K, "two clusters")
    own = reference_info(B[CLUSTER_SPLIT:, CLUSTER_SPLIT:])
    assert own > 0, "the second cluster must fail on its own"
    return {"X": X, "y": y, "K": K, "sn2": sn2, "k": CLUSTER_K, "k2": CLUSTER_SPLIT + own, "facts": f}


# ---- a dense panel with a chosen failure ---------------------------------------------------------------------------
def ldl_factor(W, seed):
    """L = chol(G G^T / W + 2 I): the operand of tests/dev_ops_cases.py's factored blocks"""
    G = np.random.default_rng(seed).standard_normal((W, W))
    return np.linalg.cholesky(G @ G.T / W + 2.0 * np.eye(W))


def ldl_panel(L, k, d=-1.0):
    """A = L D L^T with D = I except D[k] = d (k 0-based): LAPACK fails at k + 1.  d = -1: the pivot is -L[k,k]^2 <= -1,
    and A is formed as L L^T - 2 l_k l_k^T so that the flip changes no bit left of column k.
    d = 0: row and column k of L L^T are set to 0.0, so that the pivot is an EXACT zero in any order of arithmetic (with
    D[k] = 0 alone it would be a rounding error of either sign) -- LAPACK's `ajj <= 0`.  d = NaN: the NaN is put on
    A[k, k] alone, LAPACK's `disnan(ajj)`."""
    if np.isnan(d) or d == 0.0:
        A = L @ L.T
        if d == 0.0:
            A[k, :] = 0.0
            A[:, k] = 0.0
        else:
            A[k, k] = np.nan
        return A
    assert d == -1.0
    A = L @ L.T
    A[k:, k:] -= 2.0 * np.outer(L[k:, k], L[k:, k])     # = L D L^T; every entry left of column k has the bits of L L^T
    return A


def assert_ldl_discriminates(A, k, d):
    """the fixture rules for a panel: the reference answers k + 1, the pivot is <= -0.1 (d = -1), exactly 0.0 (d = 0) or
    NaN, and the earlier diagonal of L is >= 1e-3"""
    f = facts(A, k + 1)
    assert f["info"] == k + 1 and f["min_diag"] >= MIN_DIAG, (k, d, f)
    if np.isnan(d):
        assert np.isnan(f["pivot"]), (k, f)
    elif d == 0.0:
        assert f["pivot"] == 0.0, (k, f)
    else:
        assert f["pivot"] <= MAX_PIVOT, (k, f)
    return f


# ---- the three-tier schedule of tests/test_gpu_parity.py::test_tuning_environment_matrix, scaled to N = 2900 ----------
# Np = 2944: a 256-column first panel, one of 1024 (more than 1700 rows left), one of 768 (more than 900), then 256s and a
# last one of 128 -- test_failed_column.py confirms the widths with tests/potrf_plan_driver.cpp.  The columns: the first
# and the last of the 1024-wide panel, the first and the last of the 768-wide one, the first of the narrow panel after it.
THREE_TIER_N = 2900
THREE_TIER_ENV = {"GPAK_NB_XWIDE": "1024", "GPAK_NB_XWIDE_ROWS": "1700", "GPAK_NB_WIDE": "768", "GPAK_NB_WIDE_ROWS": "900",
                  "GPAK_NB_OUTER": "256"}
THREE_TIER_WIDTHS = [256, 1024, 768, 256, 256, 256, 128]
THREE_TIER_KS = (257, 1280, 1281, 2048, 2049)
