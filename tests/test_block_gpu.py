"""GPU tests (-m gpu) of block-support prediction: gpak_block_cross, gpak_predict_block and `gp_ss_ak block`.

The reference is tests/block_ref.py (NumPy; pinned in tests/test_block.py against the averaged full posterior covariance
of the discretisation points and against the CPU checker's predict).  Bounds: the averaged fill alone is held to the
project's fill tolerance (tests/dev_ops_cases.py FILL_TOL, relative to max|K|) plus the rounding of a sum of nd terms;
everything downstream to the project's 1e-8, means relative to max|y|, variances as the largest
absolute difference over the prior variance.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import block_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
from dev_ops_cases import FILL_TOL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
BOUND = 1e-8
U = 2.0 ** -53
DISC = {1: (1, 1, 1), 2: (1, 1, 2), 8: (2, 2, 2), 27: (3, 3, 3), 64: (4, 4, 4)}
SIZE = (0.1, 0.1, 0.05)

# name -> (input columns, terms, bias, white, sn2)
COMPS = {
    "defaults": (3, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "theta2": (3, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "d4-defaults": (4, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "d4-theta2": (4, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "expans+exp": (3, [(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.0, 0.016),
    "rbf": (3, [(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03),
    "expans+rbf+bias+white": (3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016),
}


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(g, terms, bias, sn2, white=0.0, mode=gpak.DIST_DIRECT):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, mode)
    else:
        g.set_kernel(terms, bias, white, sn2, mode)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


@functools.lru_cache(maxsize=None)
def data(N, cols):
    return synth.drillholes4(N) if cols == 4 else synth.drillholes(N)


@functools.lru_cache(maxsize=None)
def blocks(N, cols, M, nd):
    """M blocks with centres inside the data's bounding box.  Point 0 of the last block is moved exactly onto training
    sample 5 (distance 0 in the cross-kernel), and from nd = 2 on point 1 of the first block repeats its point 0
    (distance 0 off the diagonal of the block's own covariance)."""
    X, _ = data(N, cols)
    rng = np.random.default_rng(1000 * N + 10 * M + nd)
    centres = rng.uniform(X.min(axis=0), X.max(axis=0), (M, X.shape[1]))
    Xd, n = gpak.block_points(centres, SIZE, DISC[nd])
    assert n == nd
    Xd[(M - 1) * nd] = X[5]
    if nd >= 2:
        Xd[1] = Xd[0]
    Xd.setflags(write=False)
    return Xd


@functools.lru_cache(maxsize=None)
def reference(N, M, nd, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    return block_ref.block_predict(X, y, blocks(N, cols, M, nd), nd, terms, bias, white, sn2)


def prior_variance(comp):
    _, terms, bias, white, _ = COMPS[comp]
    return bias + white + sum(p[{xref.EXPANS: 6, xref.EXP: 1, xref.RBF: 2}[k]] ** 2 for k, p in terms)


def errors(comp, y, got_mean, got_var, want_mean, want_var):
    return np.abs(got_mean - want_mean).max() / np.abs(y).max(), np.abs(got_var - want_var).max() / prior_variance(comp)


# ---- 1. the averaged fill alone ------------------------------------------------------------------------------------
CROSS = [(comp, M, nd) for comp in COMPS for M in (1, 130, 257) for nd in (1, 2, 8, 27)]


@pytest.mark.parametrize("comp,M,nd", CROSS, ids=[f"{c}-M{m}-nd{n}" for c, m, n in CROSS])
def test_block_cross_against_long_double(gp, comp, M, nd):
    N = 300
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    Xd = blocks(N, cols, M, nd)
    want = block_ref.block_cross(X, Xd, nd, terms, bias)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    got = gp.block_cross(Xd, nd)
    bound = FILL_TOL[gpak.DIST_DIRECT] * float(np.abs(want).max()) + (nd + 2) * U * np.abs(want).astype(float)
    err = np.abs(got - want).astype(float)
    print(f"\n{comp} M={M} nd={nd}: worst error over its bound {(err / bound).max():.3g} "
          f"(largest error {err.max():.3g}, max|K| {float(np.abs(want).max()):.3g})")
    assert got.shape == (N, M) and np.all(err <= bound)
    set_defaults(gp)


def test_block_cross_in_the_expansion_form(gp):
    """GPAK_DIST_EXPANSION: the pooled mean is over the training set and all M * nd points; the values are those of
    the direct form to the fill tolerance of that form."""
    N, M, nd = 300, 130, 8
    cols, terms, bias, white, sn2 = COMPS["defaults"]
    X, y = data(N, cols)
    Xd = blocks(N, cols, M, nd)
    want = block_ref.block_cross(X, Xd, nd, terms, bias)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white, gpak.DIST_EXPANSION)
    try:
        got = gp.block_cross(Xd, nd)
    finally:
        set_defaults(gp)
    bound = FILL_TOL[gpak.DIST_EXPANSION] * float(np.abs(want).max()) + (nd + 2) * U * np.abs(want).astype(float)
    err = np.abs(got - want).astype(float)
    print(f"\nexpansion form: worst error over its bound {(err / bound).max():.3g} (largest error {err.max():.3g})")
    assert np.all(err <= bound)


# ---- 2. predict_block against the NumPy reference ---------------------------------------------------------------------
PREDICT = [
    (64, 1, 1, "defaults"), (64, 37, 2, "defaults"), (200, 130, 8, "defaults"), (200, 257, 27, "defaults"),
    (513, 37, 64, "defaults"), (513, 700, 2, "defaults"), (1000, 130, 27, "defaults"), (1000, 257, 8, "defaults"),
    (2500, 37, 27, "defaults"), (2500, 130, 8, "defaults"),
    (200, 37, 8, "theta2"), (513, 257, 2, "theta2"), (1000, 1, 64, "theta2"), (2500, 257, 1, "theta2"),
    (300, 130, 8, "d4-defaults"), (512, 37, 27, "d4-theta2"),
    (512, 130, 8, "expans+exp"), (512, 37, 27, "rbf"),
    (512, 257, 8, "expans+rbf+bias+white"), (200, 37, 1, "expans+rbf+bias+white"), (512, 37, 2, "expans+rbf+bias+white"),
]


@pytest.mark.parametrize("N,M,nd,comp", PREDICT, ids=[f"N{n}-M{m}-nd{k}-{c}" for n, m, k, c in PREDICT])
def test_predict_block_matches_numpy_reference(gp, N, M, nd, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    Xd = blocks(N, cols, M, nd)
    want = reference(N, M, nd, comp)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    mean, var = gp.predict_block(Xd, nd)
    mean_l, lat = gp.predict_block(Xd, nd, latent=True)
    mean_only, none = gp.predict_block(Xd, nd, want_var=False)
    set_defaults(gp)
    em, ev = errors(comp, y, mean, var, want["mean"], want["var"])
    el = np.abs(lat - want["latent"]).max() / prior_variance(comp)
    print(f"\nN={N} M={M} nd={nd} {comp}: mean {em:.3g} of max|y|, variance {ev:.3g} and latent variance {el:.3g} "
          f"of the prior variance")
    assert em <= BOUND and ev <= BOUND and el <= BOUND
    assert none is None and np.array_equal(mean_l, mean) and np.array_equal(mean_only, mean)
    assert np.all(lat >= 0.0) and np.all(np.abs(var - (lat + sn2 / nd)) <= 4 * U * var)


# ---- 3. one point per block is the point path ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,comp", [(200, 37, "defaults"), (513, 257, "theta2"), (512, 130, "expans+rbf+bias+white"),
                                      (300, 130, "d4-defaults")])
def test_one_point_blocks_are_point_predictions(gp, N, M, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    Xd = blocks(N, cols, M, 1)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    mean, var = gp.predict_block(Xd, 1)
    pm, pv = gp.posteriorMeanVar(Xd, compat=0)
    set_defaults(gp)
    em, ev = errors(comp, y, mean, var, pm, pv)
    print(f"\nN={N} M={M} {comp}: mean {em:.3g} of max|y| (same bytes: {np.array_equal(mean, pm)}), "
          f"variance {ev:.3g} of the prior variance (same bytes: {np.array_equal(var, pv)})")
    assert em <= BOUND and ev <= BOUND


# ---- 4. consistency with the point path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 8192])
def test_block_mean_is_the_average_of_the_point_means(gp, N):
    M, nd = 300, 8
    X, y = data(N, 3)
    Xd = blocks(N, 3, M, nd)
    gp.set_train(X, y)
    set_defaults(gp)
    mean, lat = gp.predict_block(Xd, nd, latent=True)
    pm, pv = gp.posteriorMeanVar(Xd, compat=0)
    em = np.abs(mean - pm.reshape(M, nd).mean(axis=1)).max() / np.abs(y).max()
    point_latent = (pv - synth.DEFAULT_SN2).reshape(M, nd).mean(axis=1)
    print(f"\nN={N}: block mean against the average of the point means {em:.3g} of max|y|; the latent block variance is "
          f"below the average latent point variance by {(point_latent - lat).min():.3g} .. {(point_latent - lat).max():.3g}; "
          f"predict_ms {gp.timing()['predict_ms']:.2f}")
    assert em <= BOUND
    assert np.all(lat <= point_latent)


# ---- 5. batches ---------------------------------------------------------------------------------------------------------
def test_result_holds_in_three_batches(gp):
    """M = 700 at 256 blocks per batch: 256 + 256 + 188."""
    N, M, nd = 200, 700, 8
    X, y = data(N, 3)
    Xd = blocks(N, 3, M, nd)
    want = reference(N, M, nd, "defaults")
    gp.set_train(X, y)
    set_defaults(gp)
    one = gp.predict_block(Xd, nd)
    gp.set_option(gpak.OPT_PRED_BATCH, 256)
    try:
        three = gp.predict_block(Xd, nd)
        cross3 = gp.block_cross(Xd, nd)
    finally:
        gp.set_option(gpak.OPT_PRED_BATCH, 0)
    cross1 = gp.block_cross(Xd, nd)
    for name, (mean, var) in (("one batch", one), ("three batches", three)):
        em, ev = errors("defaults", y, mean, var, want["mean"], want["var"])
        print(f"\n{name}: mean {em:.3g} of max|y|, variance {ev:.3g} of the prior variance")
        assert em <= BOUND and ev <= BOUND
    print(f"one batch against three: mean differs by {np.abs(one[0] - three[0]).max():.3g}, variance by "
          f"{np.abs(one[1] - three[1]).max():.3g}, the averaged cross-kernel by {np.abs(cross1 - cross3).max():.3g}")


# ---- 6. the call only reads ---------------------------------------------------------------------------------------------
def test_predict_block_leaves_the_context_state_alone(gp):
    N, M, nd = 513, 130, 8
    X, y = data(N, 3)
    Xd = blocks(N, 3, M, nd)
    Xte = synth.test_points(100)
    gp.set_train(X, y)
    set_defaults(gp)

    def state():
        loo = gp.loo()
        pm, pv = gp.posteriorMeanVar(Xte)
        return [np.array([gp.logLikelihood()]), gp.GradLL(), gp.GradLL_exact(), loo[0], loo[1], pm, pv]

    before = state()
    first = gp.predict_block(Xd, nd)
    after = state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    second = gp.predict_block(Xd, nd)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    # fresh parameters, no explicit factor call
    set_defaults(gp)
    third = gp.predict_block(Xd, nd)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1])
    assert gp.timing()["predict_ms"] > 0
    f32 = gpak.Gpak(0, precision=gpak.F32)   # block prediction is fp64 whatever the context's precision
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        fm, fv = f32.predict_block(Xd, nd)
        assert np.array_equal(fm, first[0]) and np.array_equal(fv, first[1])
        assert np.array_equal(f32.block_cross(Xd, nd), gp.block_cross(Xd, nd))
    finally:
        f32.close()


# ---- 7. statuses --------------------------------------------------------------------------------------------------------
def test_statuses(gp):
    X, y = data(512, 3)
    Xd = np.asfortranarray(blocks(512, 3, 37, 8))
    gp.set_train(X, y)
    set_defaults(gp)
    lib, h = gp._lib, gp._h
    mean, var = np.zeros(37), np.zeros(37)
    K = np.zeros((512, 37), order="F")
    p = gpak._p
    assert lib.gpak_predict_block(h, p(Xd), 37, 0, 3, p(mean), p(var), 0) == gpak.EINVAL
    assert lib.gpak_predict_block(h, p(Xd), 0, 8, 3, p(mean), p(var), 0) == gpak.EINVAL
    assert lib.gpak_predict_block(h, p(Xd), 37, 8, 4, p(mean), p(var), 0) == gpak.EINVAL
    assert lib.gpak_predict_block(h, None, 37, 8, 3, p(mean), p(var), 0) == gpak.EINVAL
    assert lib.gpak_predict_block(h, p(Xd), 37, 8, 3, None, p(var), 0) == gpak.EINVAL
    assert lib.gpak_block_cross(h, p(Xd), 37, 0, 3, p(K)) == gpak.EINVAL
    assert lib.gpak_block_cross(h, p(Xd), 0, 8, 3, p(K)) == gpak.EINVAL
    assert lib.gpak_block_cross(h, p(Xd), 37, 8, 4, p(K)) == gpak.EINVAL
    assert lib.gpak_block_cross(h, p(Xd), 37, 8, 3, None) == gpak.EINVAL
    with pytest.raises(gpak.GpakError) as ei:
        gp.predict_block(Xd[:-1], 8)
    assert ei.value.status == gpak.EINVAL
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    assert lib.gpak_predict_block(h, p(Xd), 37, 8, 3, p(mean), p(var), 0) == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var))
    assert lib.gpak_block_cross(h, p(Xd), 37, 8, 3, p(K)) == gpak.ENOTPD and np.all(np.isnan(K))
    m2, v2 = gp.predict_block(Xd, 8)
    assert np.all(np.isnan(m2)) and np.all(np.isnan(v2))
    set_defaults(gp)
    m3, v3 = gp.predict_block(Xd, 8)                                    # recovery at valid parameters
    assert np.all(np.isfinite(m3)) and np.all(v3 > synth.DEFAULT_SN2 / 8)
    multi = gpak.Gpak(devices=[0, 0])
    try:
        multi.set_train(X[:256], y[:256])
        set_defaults(multi)
        for call in (lambda: multi.predict_block(Xd, 8), lambda: multi.block_cross(Xd, 8)):
            with pytest.raises(gpak.GpakError) as ei:
                call()
            assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        multi.close()


# ---- 8. the command line ------------------------------------------------------------------------------------------------
def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def test_cli_block_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then block on 50 centres at 2 x 2 x 2.  The standardisation of this set is the
    identity, so the file's columns are predict_block's mean and the square root of its variance (Control::postData_var
    returns a standard deviation, as in _predict.txt), at the file's six digits."""
    import make_golden_lbfgs
    build()
    N, M = 512, 50
    Xs, ys = make_golden_lbfgs.prepared(N)
    write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(50)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (M, 3))
    yb = np.linspace(-0.5, 0.5, M)
    write_csv(tmp_path / "blocks.txt", centres, yb)
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    size, disc = ["--block-size", "0.08,0.06,0.04"], ["--block-disc", "2,2,2"]
    subprocess.run([exe, "-v", "1", *size, *disc, "block", str(tmp_path / "blocks.txt"), model, str(tmp_path / "train.txt")],
                   cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    subprocess.run([exe, "-v", "0", *size, *disc, "--latent", "block", str(tmp_path / "blocks.txt"), model,
                    str(tmp_path / "train.txt"), str(tmp_path / "latent.txt")], cwd=tmp_path, input=b"", stdout=subprocess.PIPE,
                   check=True)
    assert open(model + "_block.txt").readline() == "# BlockNo, Y, Yblock, StdYblock, Inputs\n"
    rows = np.loadtxt(model + "_block.txt", comments="#")
    rows_l = np.loadtxt(tmp_path / "latent.txt", comments="#")
    assert rows.shape == (M, 7) and np.array_equal(rows[:, 0], np.arange(1, M + 1))     # input order

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    Xd, nd = gpak.block_points(centres, (0.08, 0.06, 0.04), (2, 2, 2))
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    mean, var = gp.predict_block(Xd, nd)
    _, lat = gp.predict_block(Xd, nd, latent=True)
    set_defaults(gp)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b))

    assert close(rows[:, 1], yb) and close(rows[:, 2], mean) and close(rows[:, 3], np.sqrt(var)) and close(rows[:, 4:], centres)
    assert close(rows_l[:, 2], mean) and close(rows_l[:, 3], np.sqrt(lat))
    assert np.all(rows_l[:, 3] < rows[:, 3])
