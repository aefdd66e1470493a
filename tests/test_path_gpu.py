"""GPU tests (-m gpu) of simulation at any node count: gpak_dev_kmm, gpak_condition, gpak_sample_path, `sim --method path`.

The reference is tests/path_ref.py (long double; pinned in tests/test_path.py against joint_ref's latent covariance and
against the closed form of the spectral version).  The data, blocks and compositions are those of tests/test_block_gpu.py.
Bounds: the fused kernel alone per element (tests/path_worker.py, where the bound is stated); everything downstream of the
factor to the project's 1e-8, relative to max|y| + max|Ysim| + max|Fsim|; the spectral sampler
also gets the rounding of theta, 8 u sum_f |amp_f| (1 + sum_k |omega_fk u_k|).
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import path_ref  # noqa: E402
import path_worker  # noqa: E402
import test_block_gpu as tb  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 1e-8
U = 2.0 ** -53
LD = np.longdouble


def same(a, b):
    """the same bytes"""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def model(N, comp, M, nd):
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y = tb.data(N, cols)
    return path_ref.Model(X, y, tb.blocks(N, cols, M, nd), nd, terms, bias, white, sn2)


def draws(N, M, S, seed):
    rng = np.random.default_rng(seed)
    return 0.7 * rng.standard_normal((N, S)), 1.3 * rng.standard_normal((M, S))


def load(gp, N, comp):
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y = tb.data(N, cols)
    gp.set_train(X, y)
    tb.set_composition(gp, terms, bias, sn2, white)
    return X, y


# ---- 1. the fused kernel alone ------------------------------------------------------------------------------------------
_KMM = {}


def kmm_records():
    if not _KMM:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "path_worker.py")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        _KMM["rc"], _KMM["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _KMM[rec["name"]] = rec
    return _KMM


@pytest.mark.parametrize("case", path_worker.CASES, ids=[path_worker.case_id(c) for c in path_worker.CASES])
def test_kmm_alone_against_long_double(case):
    """gpak_dev_kmm on caller-owned buffers: every element within its bound of Kbar A + F0 in long double; A, F0, the points,
    the skew rows and the guard bands bit-identical; the same bytes from a second call; the refusals.  And the check bites."""
    recs = kmm_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[path_worker.case_id(case)]
    print(f"\n{rec}")
    assert rec["slabs"] == (2 if case[4] == path_worker.N_SLABS2 else 1)
    assert rec["ratio"] <= 1.0
    for key in ("rc", "refused", "skew_untouched", "guards", "inputs_untouched", "repeatable"):
        assert rec[key] is True, (key, rec)
    assert rec["bites"] > 1e3


# ---- 2. gpak_condition against the reference -------------------------------------------------------------------------------
# every composition at N = 300 with one shape each; N = 1000 (two sample slabs) for two of them
CONDITION = [("defaults", 300, 130, 17, 8), ("theta2", 300, 1, 1, 1), ("d4-defaults", 300, 257, 130, 2), ("d4-theta2", 300, 130, 17, 27),
             ("expans+exp", 300, 257, 17, 8), ("rbf", 300, 130, 130, 1), ("expans+rbf+bias+white", 300, 257, 17, 8),
             ("defaults", 1000, 257, 17, 8), ("expans+rbf+bias+white", 1000, 130, 17, 2)]


@pytest.mark.parametrize("comp,N,M,S,nd", CONDITION, ids=[f"{c}-N{n}-M{m}-S{s}-nd{d}" for c, n, m, s, d in CONDITION])
def test_condition_against_long_double(gp, comp, N, M, S, nd):
    cols = tb.COMPS[comp][0]
    m = model(N, comp, M, nd)
    Ysim, Fsim = draws(N, M, S, 17 * N + M + S)
    want_z, want_mean = m.condition(Ysim, Fsim)
    want_z0, _ = m.condition(Ysim, None)
    X, y = load(gp, N, comp)
    Xd = tb.blocks(N, cols, M, nd)
    try:
        fused = gp.condition(Xd, nd, Ysim, Fsim)
        unfused = gp.condition(Xd, nd, Ysim, Fsim, unfused=True)
        nof = gp.condition(Xd, nd, Ysim)
        again = gp.condition(Xd, nd, Ysim, Fsim)
        block_mean, _ = gp.predict_block(Xd, nd)
    finally:
        tb.set_defaults(gp)
    scale = np.abs(y).max() + np.abs(Ysim).max() + np.abs(Fsim).max()
    for name, (Z, mean, s), wz in (("fused", fused, want_z), ("unfused", unfused, want_z), ("fused, Fsim NULL", nof, want_z0)):
        ez = float(np.abs(Z - wz).max()) / scale
        em = float(np.abs(mean - want_mean).max()) / scale
        eb = float(np.abs(mean - block_mean).max()) / scale
        print(f"\n{comp} N={N} M={M} S={S} nd={nd} {name}: Z {ez / BOUND:.3g}, mean {em / BOUND:.3g}, mean against predict_block "
              f"{eb / BOUND:.3g} of the bound; {s}")
        assert Z.shape == (M, S) and ez <= BOUND and em <= BOUND and eb <= BOUND
        assert s["status"] == gpak.OK and s["batches"] == 1 and s["prior_ms"] == 0.0 and s["product_ms"] > 0 and s["solve_ms"] > 0
    assert fused[2]["fused"] == 1 and unfused[2]["fused"] == 0
    assert same(again[0], fused[0]) and same(again[1], fused[1])       # two calls: the same bytes
    assert gp.timing()["predict_ms"] > 0


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
def test_condition_in_three_batches_returns_the_same_bytes(gp, unfused):
    """M = 700 at 256 nodes per batch (256 + 256 + 188) against the default batch; and an F32 context: everything is fp64."""
    comp, N, M, S, nd = "defaults", 300, 700, 17, 2
    m = model(N, comp, M, nd)
    Ysim, Fsim = draws(N, M, S, 5)
    want_z, want_mean = m.condition(Ysim, Fsim)
    X, y = load(gp, N, comp)
    Xd = tb.blocks(N, 3, M, nd)
    one = gp.condition(Xd, nd, Ysim, Fsim, unfused=unfused)
    gp.set_option(gpak.OPT_PRED_BATCH, 256)
    try:
        three = gp.condition(Xd, nd, Ysim, Fsim, unfused=unfused)
    finally:
        gp.set_option(gpak.OPT_PRED_BATCH, 0)
    scale = np.abs(y).max() + np.abs(Ysim).max() + np.abs(Fsim).max()
    assert one[2]["batches"] == 1 and three[2]["batches"] == 3
    assert float(np.abs(one[0] - want_z).max()) / scale <= BOUND and float(np.abs(one[1] - want_mean).max()) / scale <= BOUND
    assert same(one[0], three[0]) and same(one[1], three[1])
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        tb.set_defaults(f32)
        Zf, mf, _ = f32.condition(Xd, nd, Ysim, Fsim, unfused=unfused)
    finally:
        f32.close()
    assert same(Zf, one[0]) and same(mf, one[1])


def test_condition_in_the_expansion_form(gp):
    """GPAK_DIST_EXPANSION: the pooled mean over the training set and all M * nd points; the direct form's values to the
    fill tolerance of that form (2e-7 of max|K|, tests/dev_ops_cases.py) through sum_j |A_js|."""
    comp, N, M, S, nd = "defaults", 300, 130, 17, 8
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    m = model(N, comp, M, nd)
    Ysim, Fsim = draws(N, M, S, 6)
    want_z, want_mean = m.condition(Ysim, Fsim)
    X, y = tb.data(N, cols)
    gp.set_train(X, y)
    tb.set_composition(gp, terms, bias, sn2, white, gpak.DIST_EXPANSION)
    try:
        Z, mean, _ = gp.condition(tb.blocks(N, cols, M, nd), nd, Ysim, Fsim)
    finally:
        tb.set_defaults(gp)
    A = m.alpha[:, None] - path_ref.solve_ky(m.L, Ysim.astype(LD))
    kmax = float(np.abs(m.Kbar).max())
    bound = 2e-7 * kmax * np.abs(A).sum(axis=0).astype(float)[None, :] + BOUND * (np.abs(y).max() + np.abs(Ysim).max() + np.abs(Fsim).max())
    err = np.abs(Z - want_z).astype(float)
    print(f"\nexpansion form: worst error over its bound {(err / bound).max():.3g}")
    assert np.all(err <= bound)


# ---- 3. gpak_sample_path as a linear map -------------------------------------------------------------------------------------
PATH = [("defaults", 1), ("expans+rbf+bias+white", 8), ("d4-theta2", 8), ("expans+exp", 1)]


def features(comp, nfeat, seed):
    """nfeat features spread over the composition's terms; one frequency of order 1e4"""
    cols, terms = tb.COMPS[comp][0], tb.COMPS[comp][1]
    rng = np.random.default_rng(seed)
    ft = (np.arange(nfeat) % len(terms)).astype(np.int32)
    om = rng.standard_normal((nfeat, 4)) / np.abs(rng.standard_normal((nfeat, 1)))
    if cols == 3:
        om[:, 3] = 0.0
    big = min(5, nfeat - 1)
    om[big] *= 1e4 / np.abs(om[big]).max()
    return ft, om


@pytest.mark.parametrize("comp,nd", PATH, ids=[f"{c}-nd{d}" for c, d in PATH])
def test_sample_path_is_the_reference_linear_map(gp, comp, nd):
    """S = 2 nfeat + 1 + N realisations with one unit normal each: Z - mean is the matrix of the map from the normals to the
    realisations.  It matches path_ref, and Z Z' the closed form of tests/path_ref.py spectral_cov."""
    N, M, nfeat = 300, 130, 24
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    m = model(N, comp, M, nd)
    ft, om = features(comp, nfeat, 11)
    S = 2 * nfeat + 1 + N
    I = np.eye(S)
    ab, b0, E = I[:2 * nfeat], I[2 * nfeat], I[2 * nfeat + 1:]
    Fsim, Ysim = m.prior_draw(ft, om, ab, b0 if bias != 0.0 else None, E)
    want_z, want_mean = m.condition(Ysim, Fsim)
    _, amp, arg = m.features(m.Xd, nd, ft, om)
    _, _, argx = m.features(m.X, 1, ft, om)
    theta = 8 * U * float((amp.astype(float) * (1 + np.maximum(arg, argx))).sum())
    X, y = load(gp, N, comp)
    Xd = tb.blocks(N, cols, M, nd)
    try:
        fused = gp.sample_path(Xd, nd, ft, om, ab, b0 if bias != 0.0 else None, E)
        unfused = gp.sample_path(Xd, nd, ft, om, ab, b0 if bias != 0.0 else None, E, unfused=True)
        again = gp.sample_path(Xd, nd, ft, om, ab, b0 if bias != 0.0 else None, E)
    finally:
        tb.set_defaults(gp)
    bound = BOUND * float(np.abs(y).max() + np.abs(Ysim).max() + np.abs(Fsim).max()) + theta
    cov = m.spectral_cov(ft, om)
    for name, (Z, mean, s) in (("fused", fused), ("unfused", unfused)):
        ez, em = float(np.abs(Z - want_z).max()), float(np.abs(mean - want_mean).max())
        T = Z - mean[:, None]
        ec = float(np.abs(T @ T.T - cov).max()) / tb.prior_variance(comp)
        print(f"\n{comp} nd={nd} {name}: Z {ez / bound:.3g}, mean {em / bound:.3g} of the bound (theta's share {theta / bound:.3g}); "
              f"Z Z' against the closed form {ec / BOUND:.3g} of 1e-8 of the prior variance; {s}")
        assert ez <= bound and em <= bound and ec <= BOUND
        assert s["status"] == gpak.OK and s["prior_ms"] > 0
    assert same(again[0], fused[0]) and same(again[1], fused[1])


# ---- 4. state and statuses ---------------------------------------------------------------------------------------------------
def test_condition_only_reads_the_context(gp):
    """nlZ, a block prediction and the leave-one-out values around a condition call equal a fresh context's, byte for byte."""
    comp, N, M, S, nd = "theta2", 513, 130, 5, 8
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y = tb.data(N, cols)
    Xd = tb.blocks(N, cols, M, nd)
    Ysim, Fsim = draws(N, M, S, 8)

    def state(g):
        loo = g.loo()
        return (np.array([g.logLikelihood()]),) + tuple(g.predict_block(Xd, nd)) + (loo[0], loo[1])

    fresh = gpak.Gpak(0)
    try:
        fresh.set_train(X, y)
        tb.set_composition(fresh, terms, bias, sn2, white)
        want = state(fresh)
    finally:
        fresh.close()
    load(gp, N, comp)
    try:
        nlz = gp.logLikelihood()
        n0 = gp.timing()["evaluations"]
        first = gp.condition(Xd, nd, Ysim, Fsim)
        mid = state(gp)
        gp.condition(Xd, nd, Ysim, Fsim, unfused=True)
        after = state(gp)
        assert gp.timing()["evaluations"] == n0 and after[0][0] == nlz
        # fresh parameters, no explicit factor call: the call factors by itself
        tb.set_composition(gp, terms, bias, sn2, white)
        third = gp.condition(Xd, nd, Ysim, Fsim)
    finally:
        tb.set_defaults(gp)
    for a, b, c in zip(want, mid, after):
        assert same(a, b) and same(a, c)
    assert same(first[0], third[0]) and same(first[1], third[1])


def test_statuses(gp):
    comp, N, M, S, nd = "defaults", 300, 130, 3, 2
    cols = 3
    X, y = load(gp, N, comp)
    Xd = np.asfortranarray(tb.blocks(N, cols, M, nd))
    Ysim, Fsim = draws(N, M, S, 9)
    Ysim, Fsim = np.asfortranarray(Ysim), np.asfortranarray(Fsim)
    Z, mean = np.zeros((M, S), order="F"), np.zeros(M)
    lib, h, p = gp._lib, gp._h, gpak._p
    ft, om = features(comp, 8, 3)
    ab, b0, E = np.asfortranarray(np.ones((16, S))), np.ones(S), np.asfortranarray(np.ones((N, S)))
    ip = ft.ctypes.data_as(gpak.C.POINTER(gpak.C.c_int))

    def cond(**kw):
        a = dict(Xd=p(Xd), M=M, nd=nd, d=cols, Ysim=p(Ysim), Fsim=p(Fsim), S=S, Z=p(Z), mean=p(mean), flags=0, summary=None)
        a.update(kw)
        return lib.gpak_condition(h, *a.values())

    def path(**kw):
        a = dict(Xd=p(Xd), M=M, nd=nd, d=cols, nfeat=8, ft=ip, om=p(om), ab=p(ab), b0=p(b0), E=p(E), S=S, Z=p(Z), mean=p(mean), flags=0,
                 summary=None)
        a.update(kw)
        return lib.gpak_sample_path(h, *a.values())

    try:
        n0 = gp.timing()["evaluations"]
        for kw in (dict(Xd=None), dict(Ysim=None), dict(Z=None), dict(M=0), dict(nd=0), dict(S=0), dict(S=-1), dict(d=4), dict(flags=2)):
            assert cond(**kw) == gpak.EINVAL, kw
        assert lib.gpak_condition(None, p(Xd), M, nd, cols, p(Ysim), None, S, p(Z), None, 0, None) == gpak.EINVAL
        for kw in (dict(Xd=None), dict(Z=None), dict(M=0), dict(nd=0), dict(S=0), dict(d=4), dict(flags=4), dict(nfeat=0), dict(ft=None),
                   dict(om=None), dict(ab=None), dict(E=None), dict(b0=None)):       # the default composition has a constant
            assert path(**kw) == gpak.EINVAL, kw
        bad = ft.copy()
        bad[3] = 1                                                                  # one term only
        assert path(ft=bad.ctypes.data_as(gpak.C.POINTER(gpak.C.c_int))) == gpak.EINVAL and "feature 3" in gp.last_error()
        assert gp.timing()["evaluations"] == n0                                     # nothing was factored for any of them
        assert cond(mean=None, Fsim=None) == gpak.OK and path(mean=None) == gpak.OK
        # a failed training factor: every output quiet NaN
        gp.set_params(np.array(tb.THETA2), 0.35, -1.0)                              # a negative sn2: B is not positive definite
        Zc, mc, s = gp.condition(Xd, nd, Ysim, Fsim)
        assert s["status"] == gpak.ENOTPD and np.all(np.isnan(Zc)) and np.all(np.isnan(mc))
        Zp, mp, s = gp.sample_path(Xd, nd, ft, om, ab, b0, E)
        assert s["status"] == gpak.ENOTPD and np.all(np.isnan(Zp)) and np.all(np.isnan(mp))
    finally:
        tb.set_defaults(gp)
    g2 = gpak.Gpak(0)
    try:
        assert g2._lib.gpak_condition(g2._h, p(Xd), M, nd, cols, p(Ysim), None, S, p(Z), None, 0, None) == gpak.ESTATE
        g2.set_train(X, y)
        assert g2._lib.gpak_condition(g2._h, p(Xd), M, nd, cols, p(Ysim), None, S, p(Z), None, 0, None) == gpak.ESTATE
        assert "no parameters" in g2.last_error()
    finally:
        g2.close()


def test_multi_gpu_context_is_refused():
    X, y = tb.data(513, 3)
    Xd = tb.blocks(513, 3, 130, 2)
    g = gpak.Gpak(devices=[0, 0])
    try:
        g.set_train(X[:256], y[:256])
        g.set_params(np.array(tb.THETA2), 0.35, 0.05)
        g.N = 256
        with pytest.raises(gpak.GpakError) as ei:
            g.condition(Xd, 2, np.zeros((256, 2)))
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
        ft, om = features("theta2", 4, 1)
        with pytest.raises(gpak.GpakError) as ei:
            g.sample_path(Xd, 2, ft, om, np.zeros((8, 2)), np.zeros(2), np.zeros((256, 2)))
        assert ei.value.status == gpak.ENOTIMPL
    finally:
        g.close()


# ---- 5. the command line -------------------------------------------------------------------------------------------------------
def test_cli_sim_path_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then `sim --method path --features 256 --realisations 4 --seed 1` on 50 block
    centres at 2 x 2 x 2: the joint verb's file format, Ymean the `block` verb's column, the same bytes from a second
    run, other realisations about the same mean from another seed."""
    import make_golden_lbfgs
    tb.build()
    N, M, S, F = 512, 50, 4, 256
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(52)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (M, 3))
    yb = np.linspace(-0.5, 0.5, M)
    tb.write_csv(tmp_path / "nodes.txt", centres, yb)
    exe, model = os.path.join(tb.HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    size, disc = ["--block-size", "0.08,0.06,0.04"], ["--block-disc", "2,2,2"]
    files = [str(tmp_path / "nodes.txt"), model, str(tmp_path / "train.txt")]
    path = ["sim", "--method", "path", "--features", str(F), "--realisations", str(S), "--seed", "1"]
    r = subprocess.run([exe, "-v", "1", *size, *disc, *path, *files], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert "spectral prior of 256 frequencies per term" in r.stdout.decode()
    first = open(model + "_sim.txt").read()
    assert first.splitlines()[0] == "# NodeNo, Y, Ymean, Sim1, Sim2, Sim3, Sim4, Inputs"
    rows = np.loadtxt(model + "_sim.txt", comments="#")
    assert rows.shape == (M, 3 + S + 3) and np.array_equal(rows[:, 0], np.arange(1, M + 1)) and np.all(np.isfinite(rows))
    subprocess.run([exe, "-v", "0", *size, *disc, "block", *files], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    block = np.loadtxt(model + "_block.txt", comments="#")
    assert np.array_equal(rows[:, 2], block[:, 2])                     # Ymean is the block verb's column, digit for digit
    subprocess.run([exe, "-v", "0", *size, *disc, *path, *files, str(tmp_path / "again.txt")], cwd=tmp_path, input=b"",
                   stdout=subprocess.PIPE, check=True)
    assert open(tmp_path / "again.txt").read() == first
    subprocess.run([exe, "-v", "0", *size, *disc, *path[:-1], "2", "--latent", *files, str(tmp_path / "other.txt")], cwd=tmp_path,
                   input=b"", stdout=subprocess.PIPE, check=True)
    other = np.loadtxt(tmp_path / "other.txt", comments="#")
    assert np.array_equal(other[:, 2], rows[:, 2]) and not np.array_equal(other[:, 3:3 + S], rows[:, 3:3 + S])
    # the realisations scatter about the mean by no more than the prior allows: a draw, not noise of another scale
    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    dev = rows[:, 3:3 + S] - rows[:, 2:3]
    assert 0 < np.abs(dev).max() <= 6 * np.sqrt(e[6] ** 2 + bias + sn2)
