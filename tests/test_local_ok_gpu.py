"""GPU tests (-m gpu) of ordinary kriging in a moving neighbourhood: gpak_predict_local_ok, gpak_dev_local_krige_ok and
`gp_ss_ak --kriging ordinary [--octant n] local`.

The reference is tests/local_ok_ref.py in long double (held in tests/test_local_ok.py against a second route, the augmented
system solved with pivoting; its float64 route meets the bound below on the CPU).  Bounds: the project's GPU bound, 1e-8
(BOUND of tests/test_block_gpu.py), means and local means relative to max|y|, variances and latent
variances to the prior variance; the invariances through the library twice that (two quantities, each held to 1e-8).  The
kernel alone has a derived bound of its own (tests/local_ok_worker.py).  Byte-for-byte claims are held byte for byte.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import local_cases as lc  # noqa: E402
import local_ok_ref as okr  # noqa: E402
import local_ok_worker  # noqa: E402
import test_block_gpu as tb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu
BOUND = tb.BOUND
U = 2.0 ** -53
QUIET = np.uint64(0x7FF8000000000000)
PARITY = ["N300-M37-nd1-defaults", "N513-M130-nd8-defaults", "N300-M37-nd8-d4-defaults", "N513-M130-nd1-expans+rbf+bias+white"]


@pytest.fixture(scope="module")
def lg():
    """a context that never sees a training set: parameters are all gpak_predict_local_ok needs"""
    g = gpak.Gpak(0)
    yield g
    g.close()


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1. parity with the long-double restatement; it is not simple kriging --------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_predict_local_ok_matches_the_long_double_reference(lg, name):
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    ref = okr.reference(name)
    assert not ref["notpd"].any()
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, mu, s = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    mean_l, lat, mu_l, _ = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True, latent=True)
    mean_o, none_v, none_m, _ = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_var=False)
    mean_v, var_v, none_m2, _ = lg.predict_local_ok(Xs, ys, Xd, nd, nbr)
    sk_mean, sk_var, sk_s = lg.predict_local(Xs, ys, Xd, nd, nbr)
    _, sk_lat, _ = lg.predict_local(Xs, ys, Xd, nd, nbr, latent=True)
    tb.set_composition(lg, terms, bias, sn2, white, gpak.DIST_EXPANSION)     # the distance is the direct form whatever the mode
    mean_e, var_e, mu_e, _ = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    tb.set_composition(lg, terms, bias, sn2, white)
    err = {"mean": okr.errors(comp, ys, mean, ref, "mean"), "var": okr.errors(comp, ys, var, ref, "var"),
           "latent": okr.errors(comp, ys, lat, ref, "latent"), "mu": okr.errors(comp, ys, mu, ref, "mu")}
    gap = float(np.abs(lat - sk_lat).max() / tb.prior_variance(comp))
    print(f"\n{name}: {err} (means of max|y|, variances of the prior variance); max|latent_OK - latent_SK| {gap:.3g} of the prior "
          f"variance; {s}")
    assert max(err.values()) <= BOUND
    assert all(np.all(np.isfinite(v)) for v in (mean, var, lat, mu))                 # no node is left out
    assert none_v is None and none_m is None and none_m2 is None
    assert same(mean_l, mean) and same(mean_o, mean) and same(mean_v, mean) and same(var_v, var) and same(mu_l, mu)
    assert same(mean_e, mean) and same(var_e, var) and same(mu_e, mu)
    assert np.all(np.abs(var - (lat + sn2 / nd)) <= 4 * U * var)
    keys = ("nodes", "empty", "notpd", "batches", "max_used")
    assert [s[k] for k in keys] == [sk_s[k] for k in keys] == [M, 0, 0, 1, min(128, max(lc.S[:M]))]
    assert lg.timing()["predict_ms"] > 0 and s["krige_ms"] > 0
    assert gap > 0.1                                                                 # it is not simple kriging


# ---- 2. invariances through the library ------------------------------------------------------------------------------
def test_a_constant_in_the_bias_or_in_ys(lg):
    name = "N300-M37-nd8-d4-defaults"
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    ymax, prior = np.abs(ys).max(), tb.prior_variance(comp)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, mu, _ = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    lifted = lg.predict_local_ok(Xs, ys + 7.25, Xd, nd, nbr, want_mu=True)
    tb.set_composition(lg, terms, bias + 3.0, sn2, white)
    try:
        more = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    finally:
        tb.set_composition(lg, terms, bias, sn2, white)
    eb = [np.abs(more[0] - mean).max() / ymax, np.abs(more[1] - var).max() / prior, np.abs(more[2] - mu).max() / ymax]
    ey = [np.abs(lifted[0] - 7.25 - mean).max() / ymax, np.abs(lifted[1] - var).max() / prior, np.abs(lifted[2] - 7.25 - mu).max() / ymax]
    print(f"\nbias + 3: mean {eb[0]:.3g}, var {eb[1]:.3g}, mu {eb[2]:.3g}; ys + 7.25: mean {ey[0]:.3g}, var {ey[1]:.3g}, mu {ey[2]:.3g}")
    assert max(eb) <= 2 * BOUND and max(ey) <= 2 * BOUND


@pytest.mark.parametrize("comp,nd", [("defaults", 8), ("expans+rbf+bias+white", 1), ("d4-defaults", 1)])
def test_all_samples_in_every_list_is_global_ordinary_kriging(lg, comp, nd):
    Ns, M = 100, 37
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys = tb.data(Ns, cols)
    Xd = tb.blocks(Ns, cols, M, nd)
    nbr = np.tile(np.arange(Ns, dtype=np.int32), (M, 1))
    ref = okr.local_predict_ok(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, mu, s = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    err = {k: okr.errors(comp, ys, v, ref, k) for k, v in (("mean", mean), ("var", var), ("mu", mu))}
    print(f"\n{comp} nd={nd}: against the reference's global ordinary kriging: {err}")
    assert max(err.values()) <= 2 * BOUND and s["max_used"] == 100
    assert np.abs(mu - mu[0]).max() <= 2 * BOUND * np.abs(ys).max()                  # one set of samples: one local mean


# ---- 3. independence, byte for byte ------------------------------------------------------------------------------------
def test_a_node_does_not_depend_on_its_company(lg):
    name = "N513-M130-nd8-defaults"
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, mu, s1 = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    again = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    assert same(again[0], mean) and same(again[1], var) and same(again[2], mu)       # two calls
    lg.set_option(gpak.OPT_PRED_BATCH, 16)
    try:
        m16, v16, u16, s16 = lg.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True)
    finally:
        lg.set_option(gpak.OPT_PRED_BATCH, 0)
    assert s1["batches"] == 1 and s16["batches"] == 9 and same(m16, mean) and same(v16, var) and same(u16, mu)
    pts = np.asarray(Xd).reshape(M, nd, -1)
    for b in range(len(lc.S)):                                                       # every size once
        s = lc.S[b]
        one = pts[b].reshape(nd, -1)
        for k in sorted({s, 128, 16 * ((s + 15) // 16)}):                            # padded to s, to its tier's edge, to 128
            m1, v1, u1, _ = lg.predict_local_ok(Xs, ys, one, nd, nbr[b:b + 1, :k], want_mu=True)   # alone, M = 1
            assert same(m1, mean[b:b + 1]) and same(v1, var[b:b + 1]) and same(u1, mu[b:b + 1]), (s, k)
    # a sub-list of the nodes in another order and another tier
    sel = [b for b in range(M) if lc.S[b % len(lc.S)] <= 32][::-1]
    m2, v2, u2, _ = lg.predict_local_ok(Xs, ys, pts[sel].reshape(len(sel) * nd, -1), nd, nbr[sel][:, :32], want_mu=True)
    assert same(m2, mean[sel]) and same(v2, var[sel]) and same(u2, mu[sel])


# ---- 4. simple kriging and the context are undisturbed -----------------------------------------------------------------
def test_predict_local_ok_disturbs_nothing():
    N = 513
    X, y = tb.data(N, 3)
    Xte = synth.test_points(50)
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd1-defaults")
    g = gpak.Gpak(0)
    try:
        g.set_train(X, y)
        tb.set_defaults(g)

        def state():
            pm, pv = g.posteriorMeanVar(Xte)
            return [np.array([g.logLikelihood()]), g.solve_alpha(), pm, pv]

        before, ev0 = state(), g.timing()["evaluations"]
        sk_before = g.predict_local(Xs, ys, Xd, 1, nbr)
        first = g.predict_local_ok(Xs, ys, Xd, 1, nbr, want_mu=True)
        assert g.timing()["evaluations"] == ev0
        sk_after = g.predict_local(Xs, ys, Xd, 1, nbr)
        after = state()
        assert same(sk_before[0], sk_after[0]) and same(sk_before[1], sk_after[1])
        assert all(same(a, b) for a, b in zip(before, after)) and g.timing()["evaluations"] == ev0
        fresh = gpak.Gpak(0)                                                         # parameters but no training set
        try:
            tb.set_defaults(fresh)
            second = fresh.predict_local_ok(Xs, ys, Xd, 1, nbr, want_mu=True)
        finally:
            fresh.close()
        assert all(same(first[i], second[i]) for i in range(3))
    finally:
        g.close()


# ---- 5. empty and failing nodes --------------------------------------------------------------------------------------
def test_an_empty_list_has_no_estimate(lg):
    comp = "expans+rbf+bias+white"
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd8-expans+rbf+bias+white")
    nbr = nbr.copy()
    gone = [0, 5, 36]
    nbr[gone] = -1
    ref = okr.local_predict_ok(Xs, ys, Xd, 8, nbr, terms, bias, white, sn2)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, mu, s = lg.predict_local_ok(Xs, ys, Xd, 8, nbr, want_mu=True)
    live = np.ones(37, dtype=bool)
    live[gone] = False
    assert s["empty"] == 3 and s["notpd"] == 0
    for v in (mean, var, mu):
        assert np.all(v[gone].view(np.uint64) == QUIET) and np.all(np.isfinite(v[live]))
    part = {k: ref[k][live] for k in ("mean", "var", "mu")}
    err = [okr.errors(comp, ys, v[live], part, k) for k, v in (("mean", mean), ("var", var), ("mu", mu))]
    assert max(err) <= BOUND


def test_a_failing_node_is_nan_and_counted(lg):
    """sn2 = -(prior variance + 1): the first pivot of every node is negative; the call still returns GPAK_OK"""
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd1-defaults")
    nbr = nbr.copy()
    nbr[3] = -1
    lg.set_params(np.array(tb.E), synth.DEFAULT_BIAS, -(tb.prior_variance("defaults") + 1.0), gpak.DIST_DIRECT)
    try:
        mean, var, mu, s = lg.predict_local_ok(Xs, ys, Xd, 1, nbr, want_mu=True)
    finally:
        tb.set_defaults(lg)
    ynan = np.array(ys)
    ynan[nbr[0, 0]] = np.nan                                                         # a NaN in ys is no failed pivot
    m_nan, _, _, s_nan = lg.predict_local_ok(Xs, ynan, Xd, 1, nbr)
    assert np.isnan(m_nan[0]) and s_nan["notpd"] == 0 and s_nan["empty"] == 1
    assert s["notpd"] == 36 and s["empty"] == 1
    for v in (mean, var, mu):
        assert np.all(v.view(np.uint64) == QUIET)                                    # the failing nodes and the empty one


# ---- 6. the kernel alone -----------------------------------------------------------------------------------------------
_KERNEL = {}


def kernel_records():
    if not _KERNEL:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_ok_worker.py")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        _KERNEL["rc"], _KERNEL["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _KERNEL[rec["name"]] = rec
    return _KERNEL


@pytest.mark.parametrize("shape", local_ok_worker.SHAPES, ids=[s[0] for s in local_ok_worker.SHAPES])
def test_kernel_alone(shape):
    """gpak_dev_local_krige_ok on caller-owned buffers (tests/local_ok_worker.py, where the bound is derived): mean, variance,
    latent variance and local mean within their backward-error bounds of the long-double values; info 0; every refusal
    writes nothing; the read-only operands and the guard bands bit-identical; the same bytes from a second call, and the
    same mean when var and mu are NULL; a node without a sample is quiet NaN.  And the check bites: simple kriging's
    variance is beyond 1e3 bounds away."""
    recs = kernel_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[shape[0]]
    print(f"\n{rec}")
    assert rec["notpd_in_reference"] is False
    assert rec["ratio_mean"] <= 1.0 and rec["ratio_var"] <= 1.0 and rec["ratio_latent"] <= 1.0 and rec["ratio_mu"] <= 1.0
    for key in ("rc", "info", "refusals", "refusals_write_nothing", "guards", "repeatable", "operands_untouched", "latent_mean_same",
                "mean_alone_same", "empty_nodes_nan"):
        assert rec[key] is True, (key, rec)
    assert rec["bites"] > 1e3


def test_kernel_alone_with_a_negative_first_pivot():
    recs = kernel_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs["failing"]
    print(f"\n{rec}")
    assert rec["rc"] is True and rec["info"] == rec["first"] == 1 and rec["nan"] is True
    assert rec["has_empty"] is True and rec["operands_untouched"] is True


# ---- 7. statuses: the outputs stay as they were ------------------------------------------------------------------------
def test_statuses_leave_the_outputs_untouched(lg):
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd1-defaults")
    Xs, Xd = np.asfortranarray(Xs), np.asfortranarray(Xd)
    nbr = np.ascontiguousarray(nbr)
    tb.set_defaults(lg)
    lib, p = lg._lib, gpak._p

    def ip(a):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    mean, var, mu = np.full(37, 7.5), np.full(37, -2.5), np.full(37, 11.0)
    summ = _lib.LocalSummary()

    def call(h=None, xs=Xs, y=ys, ns=300, d=3, xd=Xd, m=37, nd=1, nb=nbr, k=128, mn=mean, flags=0):
        return lib.gpak_predict_local_ok(lg._h if h is None else h, p(xs), p(y), ns, d, p(xd), m, nd, ip(nb), k, p(mn), p(var), p(mu),
                                         flags, ctypes.byref(summ))

    low, high, late = nbr.copy(), nbr.copy(), nbr.copy()
    low[4, 0] = -2
    high[9, 0] = 300
    late[0, 1:3] = [-1, 5]                                                           # node 0 has one sample: a valid index after a -1
    einval = [call(xs=None), call(y=None), call(xd=None), call(nb=None), call(mn=None), call(ns=0), call(m=0), call(nd=0), call(k=0),
              call(k=129), call(nb=low), call(nb=high), call(nb=late), call(flags=2), call(flags=3)]
    assert einval == [gpak.EINVAL] * len(einval)
    assert call(d=2) == gpak.ENOTIMPL and call(d=5) == gpak.ENOTIMPL
    bare = gpak.Gpak(0)
    multi = gpak.Gpak(devices=[0, 0])
    trained = gpak.Gpak(0)
    try:
        assert call(h=bare._h) == gpak.ESTATE                                        # no parameters
        assert call(h=multi._h) == gpak.ENOTIMPL
        X4, y4 = tb.data(256, 4)
        trained.set_train(X4, y4)
        tb.set_defaults(trained)
        assert call(h=trained._h) == gpak.ENOTIMPL                                   # d other than the training set's
    finally:
        bare.close(); multi.close(); trained.close()
    assert np.all(mean == 7.5) and np.all(var == -2.5) and np.all(mu == 11.0)
    assert call() == gpak.OK and np.all(np.isfinite(mean)) and np.all(np.isfinite(mu)) and summ.nodes == 37


# ---- 8. the command line -----------------------------------------------------------------------------------------------
def test_cli_local_ordinary_after_train(tmp_path):
    """train on N = 400 (two iterations), then local with ordinary kriging on 50 nodes, with the plain search and with the
    octant search.  The standardisation of this set is the identity, so the file's columns are the Python route's
    (postData_var returns a standard deviation), at the file's six digits."""
    import make_golden_lbfgs
    tb.build()
    N, M = 400, 50
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(51)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (M, 3))
    yb = np.linspace(-0.5, 0.5, M)
    tb.write_csv(tmp_path / "nodes.txt", centres, yb)
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    r = subprocess.run([exe, "-v", "1", "--neighbours", "24", "--kriging", "ordinary", "local", str(tmp_path / "nodes.txt"), model,
                        str(tmp_path / "train.txt")], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert "Nodes: 50 of 1 points from 400 samples" in r.stdout.decode() and "ordinary kriging" in r.stdout.decode()
    r = subprocess.run([exe, "-v", "1", "--neighbours", "24", "--radius", "0.6", "--octant", "4", "--kriging", "ordinary", "local",
                        str(tmp_path / "nodes.txt"), model, str(tmp_path / "train.txt"), str(tmp_path / "octant.txt")], cwd=tmp_path,
                       input=b"", stdout=subprocess.PIPE, check=True)
    assert "4 per octant" in r.stdout.decode() and "ordinary kriging" in r.stdout.decode()
    header = "# NodeNo, Y, Ylocal, StdYlocal, Neighbours, LocalMean, Inputs\n"
    assert open(model + "_local.txt").readline() == header and open(tmp_path / "octant.txt").readline() == header
    rows = np.loadtxt(model + "_local.txt", comments="#")
    rows_o = np.loadtxt(tmp_path / "octant.txt", comments="#")
    for t in (rows, rows_o):
        assert t.shape == (M, 9) and np.array_equal(t[:, 0], np.arange(1, M + 1))    # input order

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    g = gpak.Gpak(0)
    try:
        g.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
        G = g.local_metric(0)
        nbr, used = gpak.local_neighbours(Xs, centres, 24, G)
        mean, var, mu, _ = g.predict_local_ok(Xs, ys, centres, 1, nbr, want_mu=True)
        nbr_o, used_o = gpak.local_neighbours(Xs, centres, 24, G, radius=0.6, octant=4)
        nbr_r, used_r = gpak.local_neighbours(Xs, centres, 24, G, radius=0.6)
        mean_o, var_o, mu_o, _ = g.predict_local_ok(Xs, ys, centres, 1, nbr_o, want_mu=True)
    finally:
        g.close()

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b) + 1e-12)

    assert close(rows[:, 1], yb) and close(rows[:, 2], mean) and close(rows[:, 3], np.sqrt(var)) and close(rows[:, 5], mu)
    assert close(rows[:, 6:], centres) and np.array_equal(rows[:, 4], used) and np.all(used == 24)
    live = used_o > 0
    assert live.any()
    assert close(rows_o[live, 2], mean_o[live]) and close(rows_o[live, 3], np.sqrt(var_o[live])) and close(rows_o[live, 5], mu_o[live])
    assert np.all(np.isnan(rows_o[~live][:, [2, 3, 5]])) and np.array_equal(rows_o[:, 4], used_o) and close(rows_o[:, 6:], centres)
    assert not np.array_equal(nbr_o, nbr_r)                                          # the octant cap changes at least one list
