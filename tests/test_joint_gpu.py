"""GPU tests (-m gpu) of the joint posterior of block averages and of conditional simulation: gpak_predict_joint,
gpak_sample_joint and `gp_ss_ak sim`.

Data, blocks and compositions are those of tests/test_block_gpu.py (its blocks() places a point on a training sample
and repeats a point inside a block).  The reference is tests/joint_ref.py (NumPy; pinned in tests/test_joint.py).
Bounds:
  * the pair fill alone (GPAK_JOINT_PRIOR) is held to the project's fill tolerance (tests/dev_ops_cases.py FILL_TOL,
    relative to max|K|) plus the rounding of a sum of nd^2 terms;
  * everything downstream of the training factor to the project's 1e-8: means relative to max|y|,
    covariances as the largest absolute difference over the largest prior variance;
  * the factor of the covariance and the realisations by backward-error bounds that hold whatever the condition number.
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
import joint_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402
from dev_ops_cases import FILL_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
BOUND = 1e-8
COMPS, data, blocks = tb.COMPS, tb.data, tb.blocks
p = gpak._p


def train(g, N, comp, mode=gpak.DIST_DIRECT, zero_y=False):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    g.set_train(X, 0.0 * y if zero_y else y)
    tb.set_composition(g, terms, bias, sn2, white, mode)
    return X, y


@functools.lru_cache(maxsize=None)
def reference(N, M, nd, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = data(N, cols)
    # the point covariance of the definition up to 2400 points in all; beyond that the averages are taken first
    method = "points" if N + M * nd <= 2400 else "blocks"
    return joint_ref.joint(X, y, blocks(N, cols, M, nd), nd, terms, bias, white, sn2, want_prior=False, method=method)


# ---- 1. the covariance against the NumPy reference -------------------------------------------------------------------
# M = 1, 130, 257: one tile, one tile and a sliver, three row tiles (one partial) against 64-wide column tiles;
# nd = 27 and the two- and three-term compositions at nd = 8 stage the columns' points chunk by chunk (12 / 6 / 4 points
# of 1 / 2 / 3 terms fit at once)
COV = [
    (300, 1, 1, "defaults"), (300, 130, 2, "defaults"), (300, 257, 8, "defaults"), (300, 130, 27, "defaults"),
    (300, 257, 1, "theta2"), (300, 1, 27, "theta2"), (1000, 257, 8, "theta2"), (1000, 130, 27, "defaults"),
    (1000, 257, 2, "defaults"), (1000, 1, 8, "defaults"),
    (300, 130, 8, "d4-defaults"), (300, 257, 2, "d4-theta2"),
    (300, 130, 8, "expans+exp"), (300, 257, 1, "expans+exp"), (300, 130, 8, "rbf"), (300, 130, 27, "rbf"),
    (300, 257, 8, "expans+rbf+bias+white"), (300, 130, 1, "expans+rbf+bias+white"), (1000, 130, 2, "expans+rbf+bias+white"),
    (2500, 700, 8, "defaults"),
]


@pytest.mark.parametrize("N,M,nd,comp", COV, ids=[f"N{n}-M{m}-nd{k}-{c}" for n, m, k, c in COV])
def test_predict_joint_matches_numpy_reference(gp, N, M, nd, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    Xd = blocks(N, cols, M, nd)
    want = reference(N, M, nd, comp)
    X, y = train(gp, N, comp)
    mean, cov = gp.predict_joint(Xd, nd)
    mean_l, lat = gp.predict_joint(Xd, nd, latent=True)
    mean_only, none = gp.predict_joint(Xd, nd, want_cov=False)
    bmean, bvar = gp.predict_block(Xd, nd)
    tb.set_defaults(gp)
    pv = tb.prior_variance(comp)
    em = np.abs(mean - want["mean"]).max() / np.abs(y).max()
    el = np.abs(lat - want["latent"]).max() / pv
    ec = np.abs(cov - (want["latent"] + sn2 / nd * np.eye(M))).max() / pv
    # the block path clamps at 0; it does not where the reference's latent variance is positive (asserted)
    assert np.all(np.diag(want["latent"]) > 0.0)
    ed = np.abs(np.diag(cov) - bvar).max() / pv
    eb = np.abs(mean - bmean).max() / np.abs(y).max()
    print(f"\nN={N} M={M} nd={nd} {comp}: mean {em:.3g} of max|y|, latent covariance {el:.3g} and covariance {ec:.3g} of "
          f"the prior variance; diagonal against predict_block {ed:.3g}; means against predict_block {eb:.3g} "
          f"(same bytes: {np.array_equal(mean, bmean)})")
    assert em <= BOUND and el <= BOUND and ec <= BOUND and ed <= BOUND and eb <= BOUND
    assert none is None and np.array_equal(mean_l, mean) and np.array_equal(mean_only, mean)
    assert cov.shape == (M, M) and np.array_equal(cov, cov.T) and np.array_equal(lat, lat.T)
    if M == 257:
        for name, c in (("noisy", cov), ("latent", lat)):
            ev = np.linalg.eigvalsh(c).min()
            print(f"smallest eigenvalue, {name}: {ev:.3g} (largest variance {np.diag(c).max():.3g})")
            assert ev >= -1e-8 * np.diag(c).max()


@pytest.mark.parametrize("N,M,comp", [(300, 130, "defaults"), (1000, 257, "theta2"), (300, 257, "expans+rbf+bias+white"),
                                      (300, 130, "d4-defaults")])
def test_one_point_blocks_have_the_point_paths_diagonal(gp, N, M, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    Xd = blocks(N, cols, M, 1)
    X, y = train(gp, N, comp)
    mean, cov = gp.predict_joint(Xd, 1)
    pm, pvar = gp.posteriorMeanVar(Xd, compat=0)
    tb.set_defaults(gp)
    em = np.abs(mean - pm).max() / np.abs(y).max()
    ev = np.abs(np.diag(cov) - pvar).max() / tb.prior_variance(comp)
    print(f"\nN={N} M={M} {comp}: mean {em:.3g} of max|y|, diagonal {ev:.3g} of the prior variance")
    assert em <= BOUND and ev <= BOUND


# ---- 2. the pair fill alone (GPAK_JOINT_PRIOR: no substitution, no product) --------------------------------------------
PRIOR = [(comp, M, nd) for comp in COMPS for M, nd in ((1, 8), (130, 1), (130, 8), (257, 2), (257, 8))]
PRIOR += [(comp, 130, 27) for comp in ("defaults", "expans+exp", "expans+rbf+bias+white")] + [("d4-theta2", 1, 27)]


def prior_check(gp, comp, M, nd, mode):
    N = 300
    cols, terms, bias, white, sn2 = COMPS[comp]
    Xd = blocks(N, cols, M, nd)
    want = joint_ref.prior_long(Xd, nd, terms, bias, white)
    train(gp, N, comp, mode)
    try:
        mean, got = gp.predict_joint(Xd, nd, latent=True, prior=True)
        _, noisy = gp.predict_joint(Xd, nd, prior=True)
    finally:
        tb.set_defaults(gp)
    # the block fill's bound with nd^2 terms in the sum in place of nd
    bound = FILL_TOL[mode] * float(np.abs(want).max()) + (nd * nd + 2) * U * np.abs(want).astype(float)
    err = np.abs(got - want).astype(float)
    print(f"\n{comp} M={M} nd={nd} mode {mode}: worst error over its bound {(err / bound).max():.3g} "
          f"(largest error {err.max():.3g}, max|K| {float(np.abs(want).max()):.3g})")
    assert got.shape == (M, M) and np.all(err <= bound) and np.array_equal(got, got.T)
    assert np.all(np.isfinite(mean))
    off = ~np.eye(M, dtype=bool)
    assert np.array_equal(noisy[off], got[off]) and np.all(np.abs(np.diag(noisy) - np.diag(got) - sn2 / nd) <= 4 * U * np.diag(noisy))


@pytest.mark.parametrize("comp,M,nd", PRIOR, ids=[f"{c}-M{m}-nd{n}" for c, m, n in PRIOR])
def test_pair_fill_against_long_double(gp, comp, M, nd):
    prior_check(gp, comp, M, nd, gpak.DIST_DIRECT)


def test_pair_fill_in_the_expansion_form(gp):
    """GPAK_DIST_EXPANSION: the values are those of the direct form to the fill tolerance of that form."""
    prior_check(gp, "defaults", 130, 8, gpak.DIST_EXPANSION)


def exact_sum_sets(nd, cols=3):
    """A training set and 257 blocks whose column sums are exactly 0 in floating point whatever the order, also over the
    first 130 blocks alone: coordinates on a grid of 2^-20 (every partial sum is exact), points in +/- pairs, the last
    block at the origin.  The pooled mean that centres the points before the transform is then exactly 0 for M = 130 and
    for M = 257, so the blocks the two sets share have the same transformed points."""
    X, y = data(300, cols)
    q = lambda a: np.round(a * 2.0 ** 20) / 2.0 ** 20   # noqa: E731
    Xh = q(X[:150])
    Xs = np.asfortranarray(np.vstack([Xh, -Xh]))
    half = q(blocks(300, cols, 128, nd))
    Xd = np.asfortranarray(np.vstack([half[:65 * nd], -half[:65 * nd], half[65 * nd:], -half[65 * nd:],
                                      np.zeros((nd, cols))]))
    assert Xd.shape[0] == 257 * nd and np.all(Xs.sum(axis=0) == 0) and np.all(Xd.sum(axis=0) == 0)
    assert np.all(Xd[:130 * nd].sum(axis=0) == 0)
    return Xs, y, Xd


@pytest.mark.parametrize("comp,nd", [("defaults", 1), ("defaults", 8), ("defaults", 27), ("expans+exp", 8),
                                     ("expans+rbf+bias+white", 27)])
def test_an_elements_bytes_do_not_depend_on_m(gp, comp, nd):
    """The same pair of blocks at M = 130 (one row tile and a sliver) and inside M = 257 (three row tiles)."""
    cols, terms, bias, white, sn2 = COMPS[comp]
    Xs, y, Xd = exact_sum_sets(nd)
    gp.set_train(Xs, y)
    tb.set_composition(gp, terms, bias, sn2, white)
    try:
        _, big = gp.predict_joint(Xd, nd, prior=True)
        _, small = gp.predict_joint(Xd[:130 * nd], nd, prior=True)
    finally:
        tb.set_defaults(gp)
    assert small.shape == (130, 130) and np.array_equal(small, big[:130, :130])


# ---- 3. sampling ---------------------------------------------------------------------------------------------------------
# The covariance does not depend on y: with y = 0 the mean is exactly 0 and Z = Lc Xi carries no rounding of a
# mean added and taken away again, so Z - mean 1' IS what the device formed.  The addition of the mean is checked on its
# own, in bytes, in test_the_mean_is_added_once.
_FACTORS = {}   # (M, latent) -> what run_factor found: shared by the two tests below, computed once


def run_factor(gp, M, latent):
    """(Xd, nd, nugget, A = cov + nugget I from predict_joint, Lc = Z at Xi = I) at N = 300, nd = 8, defaults, y = 0."""
    case = _FACTORS.setdefault((M, latent), {})
    if case:
        return case
    N, nd, comp = 300, 8, "defaults"
    Xd = blocks(N, 3, M, nd)
    train(gp, N, comp, zero_y=True)
    try:
        mean, cov = gp.predict_joint(Xd, nd, latent=latent)
        nugget = 1e-8 * np.diag(cov).max() if latent else 0.0
        Z, zmean = gp.sample_joint(Xd, nd, np.eye(M), nugget=nugget, latent=latent)
    finally:
        tb.set_defaults(gp)
    assert np.all(mean == 0.0) and np.all(zmean == 0.0)
    case.update(Xd=Xd, nd=nd, nugget=nugget, A=cov + nugget * np.eye(M), Lc=Z)
    return case


@pytest.mark.parametrize("M", [130, 257])
@pytest.mark.parametrize("latent", [False, True], ids=["noisy-nugget0", "latent-nugget1e-8"])
def test_identity_normals_return_the_factor(gp, M, latent):
    """Xi = I (S = M): Z is the factor Lc itself.  Lc Lc' against cov + nugget I of predict_joint within
    8 (M + 1) u max diag: the backward error of a Cholesky factorisation is |A - L L'| <= gamma_(M+1) |L| |L'| (Higham,
    Accuracy and Stability of Numerical Algorithms, theorem 10.3) and (|L| |L'|)_ij <= sqrt(a_ii a_jj) (1 + O(u)) <=
    max diag by Cauchy-Schwarz on the rows of L; the 8 covers the blocked variant (panel solves through explicit
    inverses of the 128-blocks, MFMA products summed in another order) and the rounding of the input matrix itself."""
    case = run_factor(gp, M, latent)
    Lc, A = case["Lc"], case["A"]
    assert np.all(np.isfinite(Lc)) and np.all(Lc[np.triu_indices(M, 1)] == 0.0) and np.all(np.diag(Lc) > 0.0)
    LL = (Lc.astype(LD) @ Lc.astype(LD).T).astype(float)
    err, bound = np.abs(LL - A).max(), 8 * (M + 1) * U * np.diag(A).max()
    print(f"\nM={M} latent={latent} nugget={case['nugget']:.3g}: |Lc Lc' - (cov + nugget I)| {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("M", [130, 257])
@pytest.mark.parametrize("S", [3, 130])
def test_random_normals_against_the_factor(gp, M, S):
    """Z against Lc Xi in long double, Lc from the identity normals: per element (M + 2) u (|Lc| |Xi|), the bound of an
    inner product of at most M terms (Higham, section 3.1) with room for the final rounding."""
    case = run_factor(gp, M, False)
    xi = np.random.default_rng(M + S).standard_normal((M, S))
    train(gp, 300, "defaults", zero_y=True)
    try:
        Z, mean = gp.sample_joint(case["Xd"], case["nd"], xi, nugget=case["nugget"])
        Z2, _ = gp.sample_joint(case["Xd"], case["nd"], xi, nugget=case["nugget"])
    finally:
        tb.set_defaults(gp)
    want = case["Lc"].astype(LD) @ xi.astype(LD)
    bound = (M + 2) * U * (np.abs(case["Lc"]) @ np.abs(xi))
    err = np.abs(Z - want).astype(float)
    print(f"\nM={M} S={S}: worst error over its bound {(err / bound).max():.3g}")
    assert Z.shape == (M, S) and np.all(mean == 0.0) and np.all(err <= bound) and np.array_equal(Z, Z2)


def test_the_mean_is_added_once(gp):
    """With the data's own y: Z is, in bytes, the mean plus the realisation of the y = 0 context; the mean is that of
    predict_joint and of predict_block."""
    N, M, nd, S = 300, 130, 8, 5
    Xd = blocks(N, 3, M, nd)
    xi = np.random.default_rng(5).standard_normal((M, S))
    train(gp, N, "defaults", zero_y=True)
    Z0, _ = gp.sample_joint(Xd, nd, xi)
    X, y = train(gp, N, "defaults")
    Z, mean = gp.sample_joint(Xd, nd, xi)
    jm, _ = gp.predict_joint(Xd, nd, want_cov=False)
    bm, _ = gp.predict_block(Xd, nd, want_var=False)
    Zl, _ = gp.sample_joint(Xd, nd, xi, nugget=1e-9, latent=True)
    tb.set_defaults(gp)
    assert np.array_equal(mean, jm) and np.array_equal(Z, mean[:, None] + Z0)
    assert np.abs(mean - bm).max() <= BOUND * np.abs(y).max()
    assert np.all(np.isfinite(Zl)) and not np.array_equal(Zl, Z)
    # one column of normals as a vector
    z1, _ = gp.sample_joint(Xd, nd, xi[:, 0])
    assert z1.shape == (M, 1) and np.array_equal(z1[:, 0], Z[:, 0])


def test_a_singular_covariance(gp):
    """Every block repeats block 0: the latent covariance has rank one.  Without a nugget a factorisation in floating
    point may stop (GPAK_ENOTPD: Z is NaN, the text names the column) or run through on rounding (finite Z); both are
    legitimate, nothing else is, and the mean is valid either way.  With a nugget of 1e-6 of the variance it succeeds."""
    N, M, nd = 300, 130, 8
    Xd0 = blocks(N, 3, M, nd)
    Xd = np.asfortranarray(np.tile(Xd0[:nd], (M, 1)))
    xi = np.asfortranarray(np.random.default_rng(3).standard_normal((M, 4)))
    X, y = train(gp, N, "defaults")
    lib, h = gp._lib, gp._h
    bm, bv = gp.predict_block(Xd, nd, latent=True)
    Z, mean = np.zeros((M, 4), order="F"), np.zeros(M)
    rc = lib.gpak_sample_joint(h, p(Xd), M, nd, 3, p(xi), 4, 0.0, p(Z), p(mean), gpak.JOINT_LATENT)
    text = gp.last_error()
    print(f"\nrank-one covariance without a nugget: status {rc}" + (f" ({text})" if rc else ""))
    assert rc in (gpak.OK, gpak.ENOTPD)
    if rc == gpak.OK:
        assert np.all(np.isfinite(Z))
    else:
        assert np.all(np.isnan(Z)) and "column" in text and "training" not in text
    assert np.all(np.isfinite(mean)) and np.abs(mean - bm).max() <= BOUND * np.abs(y).max()
    Z2, mean2 = np.zeros((M, 4), order="F"), np.zeros(M)
    rc2 = lib.gpak_sample_joint(h, p(Xd), M, nd, 3, p(xi), 4, 1e-6 * bv.max(), p(Z2), p(mean2), gpak.JOINT_LATENT)
    assert rc2 == gpak.OK and np.all(np.isfinite(Z2)) and np.array_equal(mean2, mean)
    # every block is the same block: its realisations agree to the nugget's scale
    assert np.abs(Z2 - Z2[0]).max() <= 1e-2 * np.sqrt(bv.max()) * np.abs(xi).max() * np.sqrt(M)
    tb.set_defaults(gp)


# ---- 4. statuses -----------------------------------------------------------------------------------------------------------
def test_statuses(gp):
    X, y = data(512, 3)
    M, nd, S = 37, 8, 2
    Xd = np.asfortranarray(blocks(512, 3, M, nd))
    gp.set_train(X, y)
    tb.set_defaults(gp)
    lib, h = gp._lib, gp._h
    mean, cov = np.zeros(M), np.zeros((M, M), order="F")
    xi, Z = np.asfortranarray(np.ones((M, S))), np.zeros((M, S), order="F")
    J, SJ = lib.gpak_predict_joint, lib.gpak_sample_joint
    assert J(h, p(Xd), 0, nd, 3, p(mean), p(cov), 0) == gpak.EINVAL
    assert J(h, p(Xd), M, 0, 3, p(mean), p(cov), 0) == gpak.EINVAL
    assert J(h, p(Xd), M, nd, 4, p(mean), p(cov), 0) == gpak.EINVAL
    assert J(h, None, M, nd, 3, p(mean), p(cov), 0) == gpak.EINVAL
    assert J(h, p(Xd), M, nd, 3, None, p(cov), 0) == gpak.EINVAL
    assert J(h, p(Xd), M, nd, 3, p(mean), None, 0) == gpak.OK              # the covariance may be NULL
    assert SJ(h, p(Xd), 0, nd, 3, p(xi), S, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, 0, 3, p(xi), S, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 3, p(xi), 0, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 3, p(xi), S, -1e-9, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 4, p(xi), S, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, None, M, nd, 3, p(xi), S, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 3, None, S, 0.0, p(Z), p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 3, p(xi), S, 0.0, None, p(mean), 0) == gpak.EINVAL
    assert SJ(h, p(Xd), M, nd, 3, p(xi), S, 0.0, p(Z), None, 0) == gpak.OK  # the mean may be NULL
    with pytest.raises(gpak.GpakError) as ei:
        gp.predict_joint(Xd[:-1], nd)
    assert ei.value.status == gpak.EINVAL
    with pytest.raises(gpak.GpakError) as ei:
        gp.sample_joint(Xd, nd, np.ones((M + 1, S)))
    assert ei.value.status == gpak.EINVAL
    # the training factor fails: every output is NaN and the text says which factor it was
    gp.set_params(np.array(tb.E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    assert J(h, p(Xd), M, nd, 3, p(mean), p(cov), 0) == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(cov)) and "training factor" in gp.last_error()
    mean[:] = 0.0
    assert SJ(h, p(Xd), M, nd, 3, p(xi), S, 0.0, p(Z), p(mean), 0) == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(Z)) and "training factor" in gp.last_error()
    tb.set_defaults(gp)
    m3, c3 = gp.predict_joint(Xd, nd)                                       # recovery at valid parameters
    assert np.all(np.isfinite(m3)) and np.all(np.diag(c3) > synth.DEFAULT_SN2 / nd)
    multi = gpak.Gpak(devices=[0, 0])
    try:
        multi.set_train(X[:256], y[:256])
        tb.set_defaults(multi)
        for call in (lambda: multi.predict_joint(Xd, nd), lambda: multi.sample_joint(Xd, nd, xi)):
            with pytest.raises(gpak.GpakError) as ei:
                call()
            assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        multi.close()


# ---- 5. the calls only read --------------------------------------------------------------------------------------------------
def test_joint_calls_leave_the_context_state_alone(gp):
    N, M, nd = 513, 130, 8
    X, y = data(N, 3)
    Xd = blocks(N, 3, M, nd)
    Xte = synth.test_points(100)
    xi = np.random.default_rng(9).standard_normal((M, 3))
    gp.set_train(X, y)
    tb.set_defaults(gp)

    def state():
        loo = gp.loo()
        pm, pv = gp.posteriorMeanVar(Xte)
        bm, bv = gp.predict_block(Xd, nd)
        return [np.array([gp.logLikelihood()]), gp.GradLL(), gp.GradLL_exact(), loo[0], loo[1], pm, pv, bm, bv]

    before = state()
    first = gp.predict_joint(Xd, nd)
    sfirst = gp.sample_joint(Xd, nd, xi)
    after = state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    second, ssecond = gp.predict_joint(Xd, nd), gp.sample_joint(Xd, nd, xi)
    assert all(np.array_equal(a, b) for a, b in zip(first + sfirst, second + ssecond))
    # fresh parameters, no explicit factor call: fresh results; and back
    gp.set_params(np.array(tb.THETA2), 0.35, 0.05, gpak.DIST_DIRECT)
    other = gp.predict_joint(Xd, nd)
    assert not np.array_equal(other[0], first[0]) and not np.array_equal(other[1], first[1])
    want = joint_ref.joint(X, y, Xd, nd, COMPS["theta2"][1], 0.35, 0.0, 0.05, want_prior=False)
    assert np.abs(other[1] - want["latent"] - 0.05 / nd * np.eye(M)).max() <= BOUND * tb.prior_variance("theta2")
    tb.set_defaults(gp)
    third, sthird = gp.predict_joint(Xd, nd), gp.sample_joint(Xd, nd, xi)
    assert all(np.array_equal(a, b) for a, b in zip(first + sfirst, third + sthird))
    assert gp.timing()["predict_ms"] > 0
    f32 = gpak.Gpak(0, precision=gpak.F32)   # the joint calls are fp64 whatever the context's precision
    try:
        f32.set_train(X, y)
        tb.set_defaults(f32)
        fm, fc = f32.predict_joint(Xd, nd)
        fz, _ = f32.sample_joint(Xd, nd, xi)
        pv = tb.prior_variance("defaults")
        print(f"\nGPAK_F32 context: same bytes mean {np.array_equal(fm, first[0])}, covariance {np.array_equal(fc, first[1])}, "
              f"realisations {np.array_equal(fz, sfirst[0])}")
        assert np.abs(fm - first[0]).max() <= BOUND * np.abs(y).max() and np.abs(fc - first[1]).max() <= BOUND * pv
        assert np.abs(fz - sfirst[0]).max() <= BOUND * np.abs(y).max()
    finally:
        f32.close()


# ---- 6. what the feature is for, without a CPU reference -----------------------------------------------------------------------
def test_variance_of_the_average_of_all_blocks_at_n_8192(gp):
    """1' C 1 / M^2 (latent) is the latent variance of the ONE block made of all M * nd points."""
    N, M, nd = 8192, 300, 8
    X, y = data(N, 3)
    Xd = blocks(N, 3, M, nd)
    gp.set_train(X, y)
    tb.set_defaults(gp)
    mean, lat = gp.predict_joint(Xd, nd, latent=True)
    ms = gp.timing()["predict_ms"]
    bm, bl = gp.predict_block(Xd, nd, latent=True)
    am, al = gp.predict_block(Xd, M * nd, latent=True)
    pv = tb.prior_variance("defaults")
    ed = np.abs(np.diag(lat) - bl).max() / pv
    ea = abs(lat.sum() / (M * M) - al[0]) / pv
    em = abs(mean.mean() - am[0]) / np.abs(y).max()
    print(f"\nN={N}: diagonal against predict_block {ed:.3g}, variance of the average of all blocks {lat.sum() / (M * M):.6g} "
          f"against the one big block {al[0]:.6g}: {ea:.3g} of the prior variance; its mean {em:.3g} of max|y|; "
          f"sum of the block variances / M^2 would give {np.diag(lat).sum() / (M * M):.3g}; predict_ms {ms:.2f}")
    assert np.all(bl > 0.0) and al[0] > 0.0
    assert ed <= BOUND and ea <= BOUND and em <= BOUND


# ---- 7. the command line -----------------------------------------------------------------------------------------------------
def test_cli_sim_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then sim on 50 nodes at 2 x 2 x 2 with the normals in a file.  The
    standardisation of this set is the identity, so the file's columns are sample_joint's mean and realisations at the
    file's six digits."""
    import make_golden_lbfgs
    tb.build()
    N, M, S = 512, 50, 3
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(51)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (M, 3))
    yb = np.linspace(-0.5, 0.5, M)
    tb.write_csv(tmp_path / "nodes.txt", centres, yb)
    xi = rng.standard_normal((M, S))
    np.savetxt(tmp_path / "xi.txt", xi, fmt="%.17g")
    exe, model = os.path.join(tb.HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    size, disc = ["--block-size", "0.08,0.06,0.04"], ["--block-disc", "2,2,2"]
    files = [str(tmp_path / "nodes.txt"), model, str(tmp_path / "train.txt")]
    subprocess.run([exe, "-v", "1", *size, *disc, "--realisations", str(S), "--xi", str(tmp_path / "xi.txt"), "sim", *files],
                   cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert open(model + "_sim.txt").readline() == "# NodeNo, Y, Ymean, Sim1, Sim2, Sim3, Inputs\n"
    rows = np.loadtxt(model + "_sim.txt", comments="#")
    assert rows.shape == (M, 3 + S + 3) and np.array_equal(rows[:, 0], np.arange(1, M + 1))     # input order

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    Xd, nd = gpak.block_points(centres, (0.08, 0.06, 0.04), (2, 2, 2))
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    Z, mean = gp.sample_joint(Xd, nd, xi)
    tb.set_defaults(gp)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b))

    assert close(rows[:, 1], yb) and close(rows[:, 2], mean) and close(rows[:, 3:3 + S], Z) and close(rows[:, 3 + S:], centres)
    # points (no --block-size / --block-disc) from a seed: two runs write the same file, another seed another one
    outs = []
    for name, seed in (("a.txt", "7"), ("b.txt", "7"), ("c.txt", "8")):
        subprocess.run([exe, "-v", "0", "--realisations", "2", "--seed", seed, "--nugget", "1e-9", "--latent", "sim", *files,
                        str(tmp_path / name)], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
        outs.append(open(tmp_path / name).read())
    assert outs[0] == outs[1] and outs[0] != outs[2]
    pts = np.loadtxt(tmp_path / "a.txt", comments="#")
    assert pts.shape == (M, 3 + 2 + 3) and np.all(np.isfinite(pts))
