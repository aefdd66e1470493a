"""GPU tests (-m gpu) of moving-neighbourhood kriging: gpak_predict_local, gpak_dev_local_krige and `gp_ss_ak local`.

The reference is tests/local_ref.py in long double (pinned in tests/test_local.py against block_ref.block_predict on a model
of exactly a node's samples; its float64 route meets the bound below on the CPU).  Bounds: the project's GPU bound, 1e-8
(BOUND of tests/test_block_gpu.py), means relative to max|y|, variances and latent variances to the
prior variance; against the global path through the library twice that (two quantities, each held to 1e-8).  The kernel alone
has a derived bound of its own (tests/local_worker.py).  Byte-for-byte claims are held byte for byte.
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
import local_ref  # noqa: E402
import local_worker  # noqa: E402
import test_block_gpu as tb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu
BOUND = tb.BOUND
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lg():
    """a context that never sees a training set: parameters are all gpak_predict_local needs"""
    g = gpak.Gpak(0)
    yield g
    g.close()


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1. parity with the long-double restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_predict_local_matches_the_long_double_reference(lg, name):
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    ref = lc.reference(name)
    assert not ref["notpd"].any()
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, s = lg.predict_local(Xs, ys, Xd, nd, nbr)
    mean_l, lat, _ = lg.predict_local(Xs, ys, Xd, nd, nbr, latent=True)
    mean_o, none, _ = lg.predict_local(Xs, ys, Xd, nd, nbr, want_var=False)
    tb.set_composition(lg, terms, bias, sn2, white, gpak.DIST_EXPANSION)     # the distance is the direct form whatever the mode
    mean_e, var_e, _ = lg.predict_local(Xs, ys, Xd, nd, nbr)
    em, ev = lc.errors(comp, ys, mean, var, ref)
    _, el = lc.errors(comp, ys, mean, lat, ref, "latent")
    print(f"\n{name}: mean {em:.3g} of max|y|, variance {ev:.3g} and latent variance {el:.3g} of the prior variance; {s}")
    assert em <= BOUND and ev <= BOUND and el <= BOUND
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))                    # no node is left out
    assert none is None and same(mean_l, mean) and same(mean_o, mean)
    assert same(mean_e, mean) and same(var_e, var)
    assert np.all(np.abs(var - (lat + sn2 / nd)) <= 4 * U * var)                     # sn2 / nd = noise / nd without a White child
    assert (s["nodes"], s["empty"], s["notpd"], s["batches"], s["max_used"]) == (M, 0, 0, 1, min(128, max(lc.S[:M])))
    assert lg.timing()["predict_ms"] > 0 and s["krige_ms"] > 0


# ---- 2. against the global path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp,nd", [("defaults", 8), ("defaults", 1), ("theta2", 2), ("expans+rbf+bias+white", 8),
                                     ("expans+rbf+bias+white", 1), ("d4-defaults", 1)])
def test_all_samples_in_every_list_is_the_global_model(comp, nd):
    """Ns = 100 and every sample in every list: gpak_predict_block of a context trained on those samples, and for points
    posteriorMeanVar(compat=0)."""
    Ns, M = 100, 37
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys = tb.data(Ns, cols)
    Xd = tb.blocks(Ns, cols, M, nd)
    nbr = np.tile(np.arange(Ns, dtype=np.int32), (M, 1))
    g = gpak.Gpak(0)
    try:
        g.set_train(Xs, ys)
        tb.set_composition(g, terms, bias, sn2, white)
        mean, var, _ = g.predict_local(Xs, ys, Xd, nd, nbr)
        _, lat, _ = g.predict_local(Xs, ys, Xd, nd, nbr, latent=True)
        bm, bv = g.predict_block(Xd, nd)
        _, bl = g.predict_block(Xd, nd, latent=True)
        em, ev = tb.errors(comp, ys, mean, var, bm, bv)
        el = np.abs(lat - bl).max() / tb.prior_variance(comp)
        print(f"\n{comp} nd={nd}: against predict_block: mean {em:.3g} of max|y|, variance {ev:.3g}, latent {el:.3g} of the prior variance")
        assert em <= 2 * BOUND and ev <= 2 * BOUND and el <= 2 * BOUND
        if nd == 1:
            pm, pv = g.posteriorMeanVar(Xd, compat=0)
            em, ev = tb.errors(comp, ys, mean, var, pm, pv)
            print(f"against posteriorMeanVar: mean {em:.3g}, variance {ev:.3g}")
            assert em <= 2 * BOUND and ev <= 2 * BOUND
    finally:
        g.close()


# ---- 3. independence, byte for byte ------------------------------------------------------------------------------------
def test_a_node_does_not_depend_on_its_company(lg):
    name = "N513-M130-nd8-defaults"
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, s1 = lg.predict_local(Xs, ys, Xd, nd, nbr)
    again = lg.predict_local(Xs, ys, Xd, nd, nbr)
    assert same(again[0], mean) and same(again[1], var)                              # two calls
    lg.set_option(gpak.OPT_PRED_BATCH, 16)
    try:
        m16, v16, s16 = lg.predict_local(Xs, ys, Xd, nd, nbr)
    finally:
        lg.set_option(gpak.OPT_PRED_BATCH, 0)
    assert s1["batches"] == 1 and s16["batches"] == 9 and same(m16, mean) and same(v16, var)
    pts = np.asarray(Xd).reshape(M, nd, -1)
    for b in range(len(lc.S)):                                                       # every size once
        s = lc.S[b]
        one = pts[b].reshape(nd, -1)
        for k in sorted({s, 128, 16 * ((s + 15) // 16)}):                            # padded to s, to its tier's edge, to 128
            m1, v1, _ = lg.predict_local(Xs, ys, one, nd, nbr[b:b + 1, :k])          # alone, M = 1
            assert same(m1, mean[b:b + 1]) and same(v1, var[b:b + 1]), (s, k)
    # a sub-list of the nodes in another order and another tier
    sel = [b for b in range(M) if lc.S[b % len(lc.S)] <= 32][::-1]
    m2, v2, _ = lg.predict_local(Xs, ys, pts[sel].reshape(len(sel) * nd, -1), nd, nbr[sel][:, :32])
    assert same(m2, mean[sel]) and same(v2, var[sel])


# ---- 4. the context is untouched -------------------------------------------------------------------------------------
def test_predict_local_leaves_a_trained_context_alone():
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
        first = g.predict_local(Xs, ys, Xd, 1, nbr)
        assert g.timing()["evaluations"] == ev0
        after = state()
        assert all(same(a, b) for a, b in zip(before, after)) and g.timing()["evaluations"] == ev0
        fresh = gpak.Gpak(0)                                                         # parameters but no training set
        try:
            tb.set_defaults(fresh)
            second = fresh.predict_local(Xs, ys, Xd, 1, nbr)
        finally:
            fresh.close()
        assert same(first[0], second[0]) and same(first[1], second[1])
        f32 = gpak.Gpak(0, precision=gpak.F32)                                       # fp64 whatever the context's precision
        try:
            tb.set_defaults(f32)
            third = f32.predict_local(Xs, ys, Xd, 1, nbr)
        finally:
            f32.close()
        assert same(first[0], third[0]) and same(first[1], third[1])
    finally:
        g.close()


# ---- 5. empty and failing nodes --------------------------------------------------------------------------------------
def test_an_empty_list_returns_the_prior(lg):
    comp = "expans+rbf+bias+white"
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd8-expans+rbf+bias+white")
    nbr = nbr.copy()
    nbr[[0, 5, 36]] = -1
    ref = local_ref.local_predict(Xs, ys, Xd, 8, nbr, terms, bias, white, sn2)
    tb.set_composition(lg, terms, bias, sn2, white)
    mean, var, s = lg.predict_local(Xs, ys, Xd, 8, nbr)
    _, lat, _ = lg.predict_local(Xs, ys, Xd, 8, nbr, latent=True)
    em, ev = lc.errors(comp, ys, mean, var, ref)
    assert s["empty"] == 3 and s["notpd"] == 0 and np.all(mean[[0, 5, 36]] == 0.0) and em <= BOUND and ev <= BOUND
    prior = ref["latent"][[0, 5, 36]].astype(float)
    assert np.all(np.abs(lat[[0, 5, 36]] - prior) <= BOUND * tb.prior_variance(comp))
    assert np.all(lat[[0, 5, 36]] > lat[1:5].max())


def test_a_failing_node_is_nan_and_counted(lg):
    """sn2 = -(prior variance + 1): the first pivot of every node is negative; the call still returns GPAK_OK"""
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd1-defaults")
    nbr = nbr.copy()
    nbr[3] = -1
    lg.set_params(np.array(tb.E), synth.DEFAULT_BIAS, -(tb.prior_variance("defaults") + 1.0), gpak.DIST_DIRECT)
    try:
        mean, var, s = lg.predict_local(Xs, ys, Xd, 1, nbr)
    finally:
        tb.set_defaults(lg)
    ynan = np.array(ys)
    ynan[nbr[0, 0]] = np.nan                                                         # a NaN in ys is no failed pivot
    m_nan, _, s_nan = lg.predict_local(Xs, ynan, Xd, 1, nbr)
    assert np.isnan(m_nan[0]) and s_nan["notpd"] == 0 and s_nan["empty"] == 1
    quiet = np.uint64(0x7FF8000000000000)
    live = np.arange(37) != 3
    assert s["notpd"] == 36 and s["empty"] == 1 and mean[3] == 0.0 and np.isfinite(var[3])
    assert np.all(mean[live].view(np.uint64) == quiet) and np.all(var[live].view(np.uint64) == quiet)


# ---- 6. the kernel alone -----------------------------------------------------------------------------------------------
_KERNEL = {}


def kernel_records():
    if not _KERNEL:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_worker.py")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        _KERNEL["rc"], _KERNEL["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _KERNEL[rec["name"]] = rec
    return _KERNEL


@pytest.mark.parametrize("shape", local_worker.SHAPES, ids=[s[0] for s in local_worker.SHAPES])
def test_kernel_alone(shape):
    """gpak_dev_local_krige on caller-owned buffers (tests/local_worker.py, where the bound is derived): mean, variance and
    latent variance within their backward-error bounds of the long-double values; info 0; every refusal writes nothing; the
    read-only operands and the guard bands bit-identical; the same bytes from a second call.  And the check bites."""
    recs = kernel_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[shape[0]]
    print(f"\n{rec}")
    assert rec["notpd_in_reference"] is False
    assert rec["ratio_mean"] <= 1.0 and rec["ratio_var"] <= 1.0 and rec["ratio_latent"] <= 1.0
    for key in ("rc", "info", "refusals", "refusals_write_nothing", "guards", "repeatable", "operands_untouched", "latent_mean_same"):
        assert rec[key] is True, (key, rec)
    assert rec["bites"] > 1e3


def test_kernel_alone_with_a_negative_first_pivot():
    recs = kernel_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs["failing"]
    print(f"\n{rec}")
    assert rec["rc"] is True and rec["info"] == rec["first"] == 1 and rec["nan"] is True
    assert rec["empty_nodes_finite"] is True and rec["operands_untouched"] is True


# ---- 7. statuses: the outputs stay as they were ------------------------------------------------------------------------
def test_statuses_leave_the_outputs_untouched(lg):
    Xs, ys, Xd, nbr = lc.inputs("N300-M37-nd1-defaults")
    Xs, Xd = np.asfortranarray(Xs), np.asfortranarray(Xd)
    nbr = np.ascontiguousarray(nbr)
    tb.set_defaults(lg)
    lib, p = lg._lib, gpak._p

    def ip(a):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    mean, var = np.full(37, 7.5), np.full(37, -2.5)
    summ = _lib.LocalSummary()

    def call(h=None, xs=Xs, y=ys, ns=300, d=3, xd=Xd, m=37, nd=1, nb=nbr, k=128, mn=mean, flags=0):
        return lib.gpak_predict_local(lg._h if h is None else h, p(xs), p(y), ns, d, p(xd), m, nd, ip(nb), k, p(mn), p(var), flags,
                                      ctypes.byref(summ))

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
        with pytest.raises(gpak.GpakError) as ei:
            trained.local_metric(1)
        assert ei.value.status == gpak.EINVAL
        with pytest.raises(gpak.GpakError) as ei:
            bare.local_metric(0)
        assert ei.value.status == gpak.ESTATE
    finally:
        bare.close(); multi.close(); trained.close()
    assert np.all(mean == 7.5) and np.all(var == -2.5)
    assert call() == gpak.OK and np.all(np.isfinite(mean)) and summ.nodes == 37


def test_local_metric_is_the_distance_of_the_term(lg):
    """|(x - x') G|^2 = D2 of the term: exp(-sqrt(D2)) var2 + bias is the kernel value of a one-term model"""
    cols, terms, bias, white, sn2 = tb.COMPS["d4-defaults"]
    X, _ = tb.data(300, 4)
    tb.set_composition(lg, terms, bias, sn2, white)
    G = lg.local_metric(0)
    g2 = gpak.Gpak(0)
    try:
        g2.set_train(X[:64], np.zeros(64))
        tb.set_composition(g2, terms, bias, sn2, white)
        K = g2.gram()
    finally:
        g2.close()
    T = X[:64] @ G
    D = np.sqrt(((T[:, None, :] - T[None, :, :]) ** 2).sum(axis=2))
    want = tb.E[6] ** 2 * np.exp(-D) + bias
    assert np.abs(K - want).max() <= 1e-12 * np.abs(want).max() and G[3, 3] != 0.0 and np.all(G[3, :3] == 0.0)
    tb.set_defaults(lg)


# ---- 8. the command line -----------------------------------------------------------------------------------------------
def test_cli_local_after_train(tmp_path):
    """train on N = 400 (two iterations), then local on 50 nodes as points and as 2 x 2 x 2 blocks.  The standardisation of
    this set is the identity, so the file's columns are the Python route's (postData_var returns a standard deviation), at
    the file's six digits; --neighbours 128 with 100 samples reproduces the block verb's Yblock column."""
    import make_golden_lbfgs
    tb.build()
    N, M = 400, 50
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    tb.write_csv(tmp_path / "small.txt", Xs[:100], ys[:100])
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
    size, disc = ["--block-size", "0.08,0.06,0.04"], ["--block-disc", "2,2,2"]
    r = subprocess.run([exe, "-v", "1", "--neighbours", "24", "local", str(tmp_path / "nodes.txt"), model, str(tmp_path / "train.txt")],
                       cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert "Nodes: 50 of 1 points from 400 samples" in r.stdout.decode() and "search" in r.stdout.decode()
    subprocess.run([exe, "-v", "0", "--neighbours", "24", "--radius", "0.6", *size, *disc, "--latent", "local", str(tmp_path / "nodes.txt"),
                    model, str(tmp_path / "train.txt"), str(tmp_path / "blocks_local.txt")], cwd=tmp_path, input=b"",
                   stdout=subprocess.PIPE, check=True)
    subprocess.run([exe, "-v", "0", "--neighbours", "128", *size, *disc, "local", str(tmp_path / "nodes.txt"), model,
                    str(tmp_path / "small.txt"), str(tmp_path / "all.txt")], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    subprocess.run([exe, "-v", "0", *size, *disc, "block", str(tmp_path / "nodes.txt"), model, str(tmp_path / "small.txt"),
                    str(tmp_path / "block.txt")], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert open(model + "_local.txt").readline() == "# NodeNo, Y, Ylocal, StdYlocal, Neighbours, Inputs\n"
    rows = np.loadtxt(model + "_local.txt", comments="#")
    rows_b = np.loadtxt(tmp_path / "blocks_local.txt", comments="#")
    rows_all = np.loadtxt(tmp_path / "all.txt", comments="#")
    rows_blk = np.loadtxt(tmp_path / "block.txt", comments="#")
    assert rows.shape == (M, 8) and np.array_equal(rows[:, 0], np.arange(1, M + 1))  # input order

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    g = gpak.Gpak(0)
    try:
        g.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
        G = g.local_metric(0)
        nbr, used = gpak.local_neighbours(Xs, centres, 24, G)
        mean, var, _ = g.predict_local(Xs, ys, centres, 1, nbr)
        Xd, nd = gpak.block_points(centres, (0.08, 0.06, 0.04), (2, 2, 2))
        nbr_r, used_r = gpak.local_neighbours(Xs, centres, 24, G, radius=0.6)
        mean_b, lat_b, _ = g.predict_local(Xs, ys, Xd, nd, nbr_r, latent=True)
    finally:
        g.close()

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b) + 1e-12)

    assert close(rows[:, 1], yb) and close(rows[:, 2], mean) and close(rows[:, 3], np.sqrt(var)) and close(rows[:, 5:], centres)
    assert np.array_equal(rows[:, 4], used) and np.all(used == 24)
    assert close(rows_b[:, 2], mean_b) and close(rows_b[:, 3], np.sqrt(lat_b)) and np.array_equal(rows_b[:, 4], used_r)
    assert used_r.min() < 24                                                         # the radius decides something
    # every sample in every list: the block verb's columns, at the files' digits
    assert np.all(rows_all[:, 4] == 100)
    assert np.all(np.abs(rows_all[:, 2] - rows_blk[:, 2]) <= 2e-5 * np.abs(rows_blk[:, 2]) + 2 * BOUND * np.abs(ys).max())
    assert np.all(np.abs(rows_all[:, 3] - rows_blk[:, 3]) <= 2e-5 * np.abs(rows_blk[:, 3]))
