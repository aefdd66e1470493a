"""CPU tests (-m "not gpu") of block-support prediction:

1. tests/block_ref.py (the NumPy reference gpak_predict_block is compared with on the GPU) against the full posterior
   covariance of the discretisation points averaged over each block, and at one point per block against the CPU checker's
   predict;
2. the block variance is below the mean of the block's point variances;
3. the host's discretisation (gp_ss_ak_amd/host/block_points.hpp, compiled alone) equals gpak.block_points exactly;
4. the `block` verb of the command line refuses what it cannot do, before any device is opened.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
PARAMS = {"defaults": ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
          "theta2": ([(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
          "expans+rbf+bias+white": ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016)}
DISC = {8: (2, 2, 2), 27: (3, 3, 3), 64: (4, 4, 4)}
BOUND = 1e-10   # of the prior variance for variances, of max|y| for means; the worst seen at these sizes is 5.8e-14


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def block_points():
    """gpak.block_points without loading the device library (gp_ss_ak_amd.gpak only loads it in Gpak())."""
    from gp_ss_ak_amd import gpak
    return gpak.block_points


def prior_variance(terms, bias, white):
    return bias + white + sum(p[{xref.EXPANS: 6, xref.EXP: 1, xref.RBF: 2}[k]] ** 2 for k, p in terms)


def centres_in_box(X, M, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(X.min(axis=0), X.max(axis=0), (M, X.shape[1]))


@pytest.mark.parametrize("N,nd,name", [(200, 8, "defaults"), (200, 27, "theta2"), (200, 64, "defaults"),
                                       (513, 8, "theta2"), (513, 27, "defaults"), (513, 64, "theta2"),
                                       (200, 8, "expans+rbf+bias+white")])
def test_reference_matches_the_averaged_full_posterior(N, nd, name):
    X, y = synth.drillholes(N)
    terms, bias, white, sn2 = PARAMS[name]
    M = 12
    Xd, n = block_points()(centres_in_box(X, M, N + nd), (0.1, 0.1, 0.05), DISC[nd])
    assert n == nd
    got = block_ref.block_predict(X, y, Xd, nd, terms, bias, white, sn2)
    mu, S = block_ref.full_posterior(X, y, Xd, terms, bias, white, sn2)
    want_mean = mu.reshape(M, nd).mean(axis=1)
    want_lat = np.array([S[b * nd:(b + 1) * nd, b * nd:(b + 1) * nd].mean() for b in range(M)])
    em = np.abs(got["mean"] - want_mean).max() / np.abs(y).max()
    ev = np.abs(got["latent"] - want_lat).max() / prior_variance(terms, bias, white)
    print(f"\nN={N} nd={nd} {name}: mean {em:.3g} of max|y|, latent variance {ev:.3g} of the prior variance")
    assert em <= BOUND and ev <= BOUND
    assert np.array_equal(got["var"], got["latent"] + sn2 / nd)


@pytest.mark.parametrize("N", [200, 513])
def test_reference_at_one_point_per_block_is_the_cpu_checkers_predict(orc, N):
    """compat = 0: the checker's predictive variance includes sn2, as var_b does at nd = 1."""
    X, y = synth.drillholes(N)
    e, bias, sn2 = np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2
    Xte = np.asfortranarray(centres_in_box(X, 40, N))
    Xte[3] = X[5]
    got = block_ref.block_predict(X, y, Xte, 1, [(xref.EXPANS, E)], bias, 0.0, sn2)
    info, alpha, L = orc.nlz_lean(orc.gram(X, X, e, bias, orc.DIST_DIRECT), y, sn2)
    assert not info.chol_fail
    m, v = orc.predict(X, Xte, e, bias, sn2, alpha, L, orc.DIST_DIRECT, compat=0)
    em = np.abs(got["mean"] - m).max() / np.abs(y).max()
    ev = np.abs(got["var"] - v).max() / prior_variance([(xref.EXPANS, E)], bias, 0.0)
    print(f"\nN={N}: mean {em:.3g} of max|y|, variance {ev:.3g} of the prior variance")
    assert em <= BOUND and ev <= BOUND


@pytest.mark.parametrize("N,M,size,nd", [(200, 37, (0.1, 0.1, 0.05), 8), (513, 20, (0.2, 0.2, 0.1), 27),
                                         (513, 20, (0.2, 0.2, 0.1), 64)])
def test_block_variance_is_below_the_mean_point_variance(N, M, size, nd):
    X, y = synth.drillholes(N)
    terms, bias, white, sn2 = PARAMS["defaults"]
    centres = centres_in_box(X, M, 7 * N + nd)
    centres[M // 2] = X[5]
    Xd, _ = block_points()(centres, size, DISC[nd])
    blk = block_ref.block_predict(X, y, Xd, nd, terms, bias, white, sn2)
    pts = block_ref.block_predict(X, y, Xd, 1, terms, bias, white, sn2)
    margin = (pts["latent"].reshape(M, nd).mean(axis=1) - blk["latent"]) / prior_variance(terms, bias, white)
    print(f"\nN={N} nd={nd}: the latent block variance is below the mean latent point variance by {margin.min():.3g} .. "
          f"{margin.max():.3g} of the prior variance")
    assert np.all(margin > 0.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("block_points") / "block_points_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HOST,
                           os.path.join(ROOT, "tests", "block_points_driver.cpp"), "-o", exe])

    def run(centres, size, disc):
        M, d = centres.shape
        text = "\n".join(" ".join(f"{v:.17g}" for v in row) for row in centres)
        out = subprocess.run([exe, str(M), str(d), *[f"{v:.17g}" for v in size], *[str(v) for v in disc]], input=text.encode(),
                             stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        return np.array([[float(v) for v in line.split()] for line in out[1:]]), int(out[0])

    return run


@pytest.mark.parametrize("disc", [(1, 1, 1), (2, 2, 2), (3, 2, 1)])
@pytest.mark.parametrize("d", [3, 4])
def test_host_discretisation_equals_the_python_helper(driver, disc, d):
    rng = np.random.default_rng(11 * d + disc[0])
    centres = rng.uniform(-1000.0, 1000.0, (9, d))
    size = (25.0, 12.5, 0.3)
    want, nd = block_points()(centres, size, disc)
    got, nd_host = driver(centres, size, disc)
    restated, nd_ref = block_ref.block_points(centres, size, disc)
    assert nd == nd_host == nd_ref == disc[0] * disc[1] * disc[2]
    assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(restated, want)
    if d == 4:
        assert np.array_equal(want[:, 3], np.repeat(centres[:, 3], nd))
    # cell centres: every block's points average to its centre and span less than the block
    assert np.abs(want[:, :3].reshape(9, nd, 3).mean(axis=1) - centres[:, :3]).max() <= 1e-12
    assert np.all(np.ptp(want[:, :3].reshape(9, nd, 3), axis=1) < np.array(size))


@pytest.mark.parametrize("args,msg", [
    (["--gpus", "2", "--block-size", "1,1,1", "--block-disc", "2,2,2", "block", "blocks.txt", "model", "train.txt"], "single-GPU context"),
    (["--block-size", "1,1", "block", "blocks.txt", "model", "train.txt"], "--block-size takes dx,dy,dz"),
    (["--block-disc", "2,0,2", "block", "blocks.txt", "model", "train.txt"], "--block-disc takes three counts"),
    (["block"], "not enough input parameters"),
    (["block", "blocks.txt", "model"], "not enough input parameters"),
])
def test_cli_refuses_bad_block_invocations(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()
