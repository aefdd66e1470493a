"""CPU tests (-m "not gpu") of the leave-one-out feature:

1. tests/loo_ref.py (the NumPy restatement gpak_loo is compared with on the GPU) against N brute-force refits and
   against the CPU checker's predict on the N - 1 remaining points;
2. the summary fields against their definitions;
3. the `cv` verb of the command line refuses what it cannot do, before any device is opened.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
PARAMS = {"defaults": ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2),
          "theta2": ([(xref.EXPANS, THETA2)], 0.35, 0.05),
          "expans+rbf+bias": ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.016)}
# (N, input columns, parameters, stride of the left-out samples)
CASES = [(N, cols, name, 3 if N == 513 else 1) for N in (64, 200, 513) for cols in (3, 4) for name in ("defaults", "theta2")]
CASES.append((200, 3, "expans+rbf+bias", 1))
BOUND = 1e-11   # of max|y| for means, relative per element for variances; the worst seen at these sizes is 1.6e-13


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def data(N, cols):
    return synth.drillholes4(N) if cols == 4 else synth.drillholes(N)


@pytest.mark.parametrize("N,cols,name,stride", CASES)
def test_restatement_matches_brute_force_refits(N, cols, name, stride):
    X, y = data(N, cols)
    terms, bias, sn2 = PARAMS[name]
    K = xref.gram(X, terms, bias)
    mean, var = loo_ref.loo(K, y, sn2)
    idx = np.arange(0, N, stride)
    rm, rv = loo_ref.refit(K, y, sn2, idx)
    em = np.abs(mean[idx] - rm).max() / np.abs(y).max()
    ev = (np.abs(var[idx] - rv) / rv).max()
    print(f"\nN={N} d={cols} {name}: {len(idx)} refits, mean {em:.3g} of max|y|, variance {ev:.3g} relative")
    assert em <= BOUND and ev <= BOUND
    assert np.all(var > sn2) and np.all(var < K.diagonal() + sn2)   # between the noise and the prior variance


def test_restatement_with_a_white_child_matches_refits():
    N = 64
    X, y = data(N, 3)
    terms, bias, sn2 = PARAMS["expans+rbf+bias"]
    K = loo_ref.add_white(xref.gram(X, terms, bias), 0.1)
    mean, var = loo_ref.loo(K, y, sn2)
    rm, rv = loo_ref.refit(K, y, sn2, range(N))
    assert np.abs(mean - rm).max() <= BOUND * np.abs(y).max() and (np.abs(var - rv) / rv).max() <= BOUND
    assert np.all(var > sn2 + 0.1)


def test_restatement_matches_the_cpu_checkers_predict_on_the_remaining_points(orc):
    """compat = 0: the checker's predictive variance includes sn2, as var_i does."""
    N = 200
    X, y = data(N, 3)
    e, bias, sn2 = np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2
    mean, var = loo_ref.loo(xref.gram(X, [(xref.EXPANS, E)], bias), y, sn2)
    worst_m = worst_v = 0.0
    for i in range(0, N, 9):
        keep = np.arange(N) != i
        Xr, yr = np.asfortranarray(X[keep]), y[keep]
        info, alpha, L = orc.nlz_lean(orc.gram(Xr, Xr, e, bias, orc.DIST_DIRECT), yr, sn2)
        assert not info.chol_fail
        m, v = orc.predict(Xr, np.asfortranarray(X[i:i + 1]), e, bias, sn2, alpha, L, orc.DIST_DIRECT, compat=0)
        worst_m = max(worst_m, abs(m[0] - mean[i]) / np.abs(y).max())
        worst_v = max(worst_v, abs(v[0] - var[i]) / var[i])
    print(f"\nN={N}: every 9th sample, mean {worst_m:.3g} of max|y|, variance {worst_v:.3g} relative")
    assert worst_m <= BOUND and worst_v <= BOUND


def test_summary_fields_follow_their_definitions():
    y = np.array([0.5, -1.0, 2.0])
    mean = np.array([0.0, -1.5, 1.0])
    var = np.array([0.25, 1.0, 4.0])
    s = loo_ref.summary(y, mean, var)
    assert s["mse"] == pytest.approx((0.25 + 0.25 + 1.0) / 3, rel=1e-15)
    assert s["mssr"] == pytest.approx((1.0 + 0.25 + 0.25) / 3, rel=1e-15)
    want = sum(math.log(math.exp(-0.5 * (a - m) ** 2 / v) / math.sqrt(2 * math.pi * v)) for a, m, v in zip(y, mean, var))
    assert s["log_pl"] == pytest.approx(want, rel=1e-14)
    # a calibrated model: residuals drawn with the stated variances give mssr near 1
    rng = np.random.default_rng(3)
    v = rng.uniform(0.1, 2.0, 20000)
    r = rng.standard_normal(20000) * np.sqrt(v)
    assert abs(loo_ref.summary(r, np.zeros_like(r), v)["mssr"] - 1.0) < 0.05


@pytest.mark.parametrize("args,msg", [
    (["--gpus", "2", "cv", "train.txt", "model"], "one GPU only"),
    (["-g", "2", "cv", "-np", "train.txt", "model"], "one GPU only"),
    (["cv"], "not enough input parameters"),
    (["cv", "train.txt"], "not enough input parameters"),
    (["cv", "-np", "train.txt"], "not enough input parameters"),
])
def test_cli_refuses_bad_cv_invocations(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()
