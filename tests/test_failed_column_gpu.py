"""gpak_failed_column past column 1: a context told to factor a matrix that fails at a CHOSEN column (tests/failcol_ref.py)
answers that column -- an integer, no tolerance: the gap of every fixture is orders of magnitude wider than the
difference between the device's Gram matrix and NumPy's -- under the schedules that factor panels differently (panel
widths and tiers, look-ahead off, either build of the block kernel, the tail queue, the sub-panel and split updates of
the next block column, no forward substitution beside the factorisation, no optional queues), in EXPANSION mode, in a
GPAK_F32 context and on a group of ranks; every call that needs the factor answers as include/gpak.h promises, the error
text names the column, and good parameters afterwards give the bits of a fresh context.

Column 1 (sn2 = -0.5, what every other test of a failure uses) is the one input for which `col0` dropped, the tile-local
column, a plain store in place of atomicMin and rank 0's value without the min-reduce all answer correctly.
"""
import math
import os
import re

import numpy as np
import pytest

import failcol_ref as fr
from gp_ss_ak_amd import gpak, synth

pytestmark = pytest.mark.gpu

E = np.array(synth.DEFAULT_EXPANS)
BIAS, SN2 = synth.DEFAULT_BIAS, synth.DEFAULT_SN2
N = 1300                                                  # ten full 128-tiles and one of 20 rows
KS = (1, 2, 16, 17, 128, 129, 257, 513, 1025, 1153, 1299, 1300)
GROUP_KS = (1, 129, 257, 385, 513, 1025, 1300)


def _blocks():
    c = np.array([[0.1, -0.2, 0.3], [-0.5, 0.4, 0.0], [0.7, 0.7, -0.6]])
    return gpak.block_points(c, (0.1, 0.1, 0.05), (2, 2, 2))


def _raises_notpd(fn):
    with pytest.raises(gpak.GpakError) as ei:
        fn()
    assert ei.value.status == gpak.ENOTPD, ei.value


def _assert_failure(g, k, full=True):
    """every answer of a context whose factorisation fails at column k"""
    assert g.factor() is False, k
    assert g.failed_column() == k, (g.failed_column(), k)
    assert math.isnan(g.logLikelihood()), k
    assert g.failed_column() == k, (g.failed_column(), k)
    if not full:
        return
    Xte = synth.test_points(5)
    _raises_notpd(g.solve_alpha)                                        # GPAK_ENOTPD, nothing to hand out
    _raises_notpd(lambda: g.posteriorMeanVar(Xte))
    mean, var, s = g.loo()
    assert s["status"] == gpak.ENOTPD and np.isnan(mean).all() and np.isnan(var).all() and math.isnan(s["log_pl"]), k
    Xd, nd = _blocks()
    bm, bv = g.predict_block(Xd, nd)
    assert np.isnan(bm).all() and np.isnan(bv).all(), k
    assert re.search(rf"column {k}\b", g.last_error()), (k, g.last_error())
    jm, jc = g.predict_joint(Xd, nd)
    assert np.isnan(jm).all() and np.isnan(jc).all(), k
    assert re.search(rf"column {k}\b", g.last_error()), (k, g.last_error())
    assert g.failed_column() == k, (g.failed_column(), k)


def _good(g, mode=gpak.DIST_DIRECT, bias=BIAS):
    g.set_params(E, bias, SN2, mode)
    nlz, alpha = g.logLikelihood(), g.solve_alpha()
    return nlz, alpha, g.failed_column()


def _run(make, n, ks, mode=gpak.DIST_DIRECT, full=True):
    """one context through every k, then recovery against a fresh context made the same way"""
    X, y, _K = fr.drill_gram(n, mode)
    cases = [(k,) + fr.drill_case(n, k, mode) for k in ks]             # the fixture rules are asserted on the CPU first
    g = make()
    try:
        g.set_train(X, y)
        for k, sn2, _f in cases:
            g.set_params(E, BIAS, sn2, mode)
            _assert_failure(g, k, full)
        nlz, alpha, col = _good(g, mode)
    finally:
        g.close()
    f = make()
    try:
        f.set_train(X, y)
        nlz0, alpha0, col0 = _good(f, mode)
    finally:
        f.close()
    assert col == 0 and col0 == 0
    assert np.isfinite(nlz) and np.array([nlz]).view(np.uint64)[0] == np.array([nlz0]).view(np.uint64)[0], (nlz, nlz0)
    assert np.array_equal(alpha.view(np.uint64), alpha0.view(np.uint64))


def _with_options(opts, precision=gpak.F64):
    def make():
        g = gpak.Gpak(0, precision)
        for o, v in opts.items():
            g.set_option(o, v)
        return g
    return make


OPTION_SCHEDULES = {
    "default": {},
    "nb_outer=128": {gpak.OPT_NB_OUTER: 128},
    "nb_outer=256": {gpak.OPT_NB_OUTER: 256},
    "nb_outer=512": {gpak.OPT_NB_OUTER: 512},
    "lookahead=0": {gpak.OPT_LOOKAHEAD: 0},
    "potrf_co=0": {gpak.OPT_POTRF_CO: 0},
    "potrf_co=2": {gpak.OPT_POTRF_CO: 2},
    "tail queue from the first panel": {gpak.OPT_TAIL_ROWS: 100000},
    "no tail queue at this size": {gpak.OPT_TAIL_ROWS: 0},
    "nb_outer=128, lookahead=0, potrf_co=2": {gpak.OPT_NB_OUTER: 128, gpak.OPT_LOOKAHEAD: 0, gpak.OPT_POTRF_CO: 2},
}


@pytest.mark.parametrize("name", list(OPTION_SCHEDULES))
def test_failed_column_under_option_schedules(name):
    _run(_with_options(OPTION_SCHEDULES[name]), N, KS, full=(name == "default"))


# the rows of test_tuning_environment_matrix (tests/test_gpu_parity.py) that change how panels are factored
ENV_SCHEDULES = {
    "three tiers": (fr.THREE_TIER_N, fr.THREE_TIER_KS, fr.THREE_TIER_ENV),
    "sub_next": (N, KS, {"GPAK_SUB_NEXT": "1", "GPAK_TAIL_ROWS": "100000"}),
    "sub_next + next_split": (N, KS, {"GPAK_NEXT_SPLIT_ROWS": "100000", "GPAK_SUB_NEXT": "1", "GPAK_NB_OUTER": "384"}),
    "next_split": (N, KS, {"GPAK_NEXT_SPLIT_ROWS": "100000"}),
    "fwd_in_factor=0": (N, KS, {"GPAK_FWD_IN_FACTOR": "0"}),
    "no tail, no bulk queue": (N, KS, {"GPAK_TAIL_MASK": "0", "GPAK_BULK_QUEUE": "0"}),
}


@pytest.mark.parametrize("name", list(ENV_SCHEDULES))
def test_failed_column_under_environment_schedules(name):
    from gp_ss_ak_amd import _lib
    lib = _lib.load()
    n, ks, env = ENV_SCHEDULES[name]
    keys = sorted({k for _n, _k, e in ENV_SCHEDULES.values() for k in e})
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        lib.gpak_reload_tuning()
        _run(lambda: gpak.Gpak(0), n, ks, full=False)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.gpak_reload_tuning()


@pytest.mark.parametrize("lookahead", [1, 0])
def test_two_failures_report_the_first(lookahead):
    """Two clusters with a cross-kernel of exactly 0.0: the first fails at column 200, the second ON ITS OWN at global
    column 549 -- two writers of `info`, in different panels; the answer is the minimum."""
    c = fr.two_clusters()                                  # asserts the rules and that the second cluster fails alone
    assert c["k"] == 200 and c["k2"] > 512
    g = _with_options({gpak.OPT_LOOKAHEAD: lookahead, gpak.OPT_NB_OUTER: 256})()
    try:
        g.set_train(c["X"], c["y"])
        g.set_params(E, 0.0, c["sn2"], gpak.DIST_DIRECT)
        assert np.array_equal(g.gram()[fr.CLUSTER_SPLIT:, :fr.CLUSTER_SPLIT], np.zeros((300, 300)))
        g.set_params(E, 0.0, c["sn2"], gpak.DIST_DIRECT)
        _assert_failure(g, 200, full=False)
        nlz, _alpha, col = _good(g, bias=0.0)
        assert np.isfinite(nlz) and col == 0
    finally:
        g.close()


def test_failed_column_in_expansion_mode():
    k = 513
    _sn2, f = fr.drill_case(N, k, gpak.DIST_EXPANSION)
    assert f["gap"] >= 1e3 * 2e-7                          # the two K's differ by 2e-7 relative (test_gram_matches_oracle)
    _run(lambda: gpak.Gpak(0), N, (k,), mode=gpak.DIST_EXPANSION)


def test_failed_column_in_an_f32_context():
    """the training step is fp64 in a GPAK_F32 context too: the same answer"""
    _run(_with_options({}, gpak.F32), N, (257,), full=False)


@pytest.mark.parametrize("ranks", [2, 3])
def test_failed_column_on_a_group(ranks):
    """Gpak(devices=[0] * ranks): the failing column is owned by each rank in turn; the group's answer is the min-reduced
    one, and good parameters afterwards give the bits of a fresh group."""
    X, y, _K = fr.drill_gram(N)
    cases = [(k,) + fr.drill_case(N, k) for k in GROUP_KS]
    make = lambda: gpak.Gpak(devices=[0] * ranks)
    g = make()
    try:
        g.set_train(X, y)
        owners = set()
        for k, sn2, _f in cases:
            g.set_params(E, BIAS, sn2, gpak.DIST_DIRECT)
            assert math.isnan(g.logLikelihood()), k
            assert g.failed_column() == k, (g.failed_column(), k)
            assert g.factor() is False and g.failed_column() == k, k
            assert re.search(rf"column {k}\b", g.last_error()), (k, g.last_error())
            nb = g.rank_stats(0)["nb"]
            owners.add((k - 1) // nb % ranks)
        assert owners == set(range(ranks)), (owners, nb)            # every rank owned a failing column
        nlz, alpha, col = _good(g)
    finally:
        g.close()
    f = make()
    try:
        f.set_train(X, y)
        nlz0, alpha0, col0 = _good(f)
    finally:
        f.close()
    assert col == 0 and col0 == 0 and np.isfinite(nlz)
    assert np.array([nlz]).view(np.uint64)[0] == np.array([nlz0]).view(np.uint64)[0], (nlz, nlz0)
    assert np.array_equal(alpha.view(np.uint64), alpha0.view(np.uint64))
