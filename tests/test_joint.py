"""CPU tests (-m "not gpu") of the joint posterior of block averages and of conditional simulation:

1. tests/joint_ref.py (the NumPy reference gpak_predict_joint is compared with on the GPU) against
   block_ref.block_predict on its diagonal and block_ref.full_posterior at one point per block; symmetric; positive
   semi-definite to rounding;
2. the header declares the two entry points, the built library exports them and gpak.Gpak has the two methods;
3. the `sim` verb of the command line refuses what it cannot do, before any device is opened;
4. the host's normal generator (gp_ss_ak_amd/host/sim_normals.hpp, compiled alone) is a function of its seed.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import joint_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
# the seven compositions of tests/test_block_gpu.py: name -> (input columns, terms, bias, white, sn2)
COMPS = {
    "defaults": (3, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "theta2": (3, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "d4-defaults": (4, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "d4-theta2": (4, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "expans+exp": (3, [(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.0, 0.016),
    "rbf": (3, [(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03),
    "expans+rbf+bias+white": (3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016),
}
DISC = {1: (1, 1, 1), 2: (1, 1, 2), 8: (2, 2, 2)}
BOUND = 1e-10   # of the prior variance for covariances, of max|y| for means


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def prior_variance(terms, bias, white):
    return bias + white + sum(p[{xref.EXPANS: 6, xref.EXP: 1, xref.RBF: 2}[k]] ** 2 for k, p in terms)


def blocks(X, M, nd, seed):
    from gp_ss_ak_amd import gpak
    rng = np.random.default_rng(seed)
    centres = rng.uniform(X.min(axis=0), X.max(axis=0), (M, X.shape[1]))
    Xd, n = gpak.block_points(centres, (0.1, 0.1, 0.05), DISC[nd])
    assert n == nd
    Xd[(M - 1) * nd] = X[5]            # a point on a training sample
    if nd >= 2:
        Xd[1] = Xd[0]                  # a point repeated inside a block
    return Xd


CASES = [(N, M, nd, comp) for comp in COMPS for N, M, nd in ((64, 1, 8), (64, 5, 1), (64, 40, 2), (300, 5, 8), (300, 40, 1))]
CASES += [(300, 1, 2, "defaults"), (300, 40, 8, "defaults"), (64, 40, 8, "expans+rbf+bias+white"), (300, 5, 2, "expans+rbf+bias+white")]


@pytest.mark.parametrize("N,M,nd,comp", CASES, ids=[f"N{n}-M{m}-nd{k}-{c}" for n, m, k, c in CASES])
def test_reference_is_pinned(N, M, nd, comp):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    Xd = blocks(X, M, nd, 100 * N + 10 * M + nd)
    got = joint_ref.joint(X, y, Xd, nd, terms, bias, white, sn2)
    pv = prior_variance(terms, bias, white)
    lat = got["latent"]
    # the diagonal is the block path's latent variance (nowhere clamped here: asserted)
    blk = block_ref.block_predict(X, y, Xd, nd, terms, bias, white, sn2)
    assert np.all(np.diag(lat) > 0.0)
    ed = np.abs(np.diag(lat) - blk["latent"]).max() / pv
    em = np.abs(got["mean"] - blk["mean"]).max() / np.abs(y).max()
    # symmetric, positive semi-definite to rounding
    es = np.abs(lat - lat.T).max() / pv
    ev = np.linalg.eigvalsh((lat + lat.T) / 2).min() / np.diag(lat).max()
    # the prior in long double against the stacked double Gram matrix the posterior was formed from
    Kd = xref.gram(Xd, terms, bias).reshape(M, nd, M, nd).mean(axis=(1, 3)) + white / nd * np.eye(M)
    ep = float(np.abs(got["prior"] - Kd).max()) / pv
    print(f"\nN={N} M={M} nd={nd} {comp}: diagonal {ed:.3g}, mean {em:.3g}, asymmetry {es:.3g}, prior {ep:.3g}, "
          f"smallest eigenvalue {ev:.3g} of the largest variance")
    assert ed <= BOUND and em <= BOUND and es <= BOUND and ep <= BOUND and ev >= -1e-10
    assert got["prior"].dtype == np.longdouble
    # the same quantity with the averages taken first (what the GPU tests use for their largest sets)
    alt = joint_ref.joint(X, y, Xd, nd, terms, bias, white, sn2, want_prior=False, method="blocks")
    assert np.abs(alt["latent"] - lat).max() / pv <= BOUND and np.abs(alt["mean"] - got["mean"]).max() / np.abs(y).max() <= BOUND
    if nd == 1:   # the full posterior of the points, White on its diagonal
        mu, S = block_ref.full_posterior(X, y, Xd, terms, bias, white, sn2)
        assert np.abs(lat - S).max() / pv <= BOUND and np.abs(got["mean"] - mu).max() / np.abs(y).max() <= BOUND


def test_white_sits_on_the_block_diagonal_only():
    """Two blocks that share every point: white / nd on the diagonal, nothing between them."""
    cols, terms, bias, white, sn2 = COMPS["expans+rbf+bias+white"]
    X, y = synth.drillholes(64)
    Xd = blocks(X, 2, 8, 3)
    Xd[8:] = Xd[:8]
    with_w = joint_ref.joint(X, y, Xd, 8, terms, bias, white, sn2)
    prior0 = joint_ref.prior_long(Xd, 8, terms, bias, 0.0)
    assert np.allclose(np.asarray(with_w["prior"] - prior0, dtype=float), white / 8 * np.eye(2), rtol=0, atol=1e-15)
    lat = with_w["latent"]
    assert abs((lat[0, 0] - lat[0, 1]) - white / 8) <= 1e-12


# ---- what the parent commit does not have -------------------------------------------------------------------------------
def header_functions():
    import re
    txt = open(os.path.join(ROOT, "include", "gpak.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gpak_[a-z0-9_]+)\s*\(", txt))


def test_header_declares_and_library_exports_the_joint_calls():
    assert {"gpak_predict_joint", "gpak_sample_joint"} <= header_functions()
    assert {"gpak_predict_joint", "gpak_sample_joint"} <= set(_lib.SYMBOLS)
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "gpak_predict_joint") and hasattr(lib, "gpak_sample_joint")
    assert not hasattr(lib, "gpak_joint_prior")      # the prior alone is a flag bit, not an entry point


def test_python_class_has_the_joint_methods():
    from gp_ss_ak_amd import gpak
    assert callable(gpak.Gpak.predict_joint) and callable(gpak.Gpak.sample_joint)
    assert gpak.JOINT_LATENT == 1 and gpak.JOINT_PRIOR == 2


SIM = ["--realisations", "3", "--seed", "1"]


@pytest.mark.parametrize("args,msg", [
    (["sim"], "not enough input parameters"),
    ([*SIM, "sim", "nodes.txt", "model"], "not enough input parameters"),
    (["--gpus", "2", *SIM, "sim", "nodes.txt", "model", "train.txt"], "single-GPU context"),
    (["--seed", "1", "sim", "nodes.txt", "model", "train.txt"], "sim needs --realisations S with S > 0"),
    (["--realisations", "0", "--seed", "1", "sim", "nodes.txt", "model", "train.txt"], "sim needs --realisations S with S > 0"),
    (["--realisations", "3", "sim", "nodes.txt", "model", "train.txt"], "exactly one of --seed n and --xi file"),
    ([*SIM, "--xi", "xi.txt", "sim", "nodes.txt", "model", "train.txt"], "exactly one of --seed n and --xi file"),
    ([*SIM, "--block-size", "1,1,1", "sim", "nodes.txt", "model", "train.txt"], "--block-size and --block-disc together"),
    ([*SIM, "--block-disc", "2,2,2", "sim", "nodes.txt", "model", "train.txt"], "--block-size and --block-disc together"),
    ([*SIM, "--nugget", "-1", "sim", "nodes.txt", "model", "train.txt"], "--nugget takes a non-negative value"),
])
def test_cli_refuses_bad_sim_invocations(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


def test_cli_refuses_an_xi_file_of_the_wrong_shape(tmp_path):
    """Read before the model or any device: 4 nodes and S = 3 against a 4 x 2 and a 3 x 3 file."""
    build()
    with open(tmp_path / "nodes.txt", "w") as f:
        f.write("# x, y, z, grade\n" + "".join(f"{i}\t{2 * i}\t{3 * i}\t0.5\n" for i in range(4)))
    for name, rows, colsn in (("narrow.txt", 4, 2), ("short.txt", 3, 3)):
        np.savetxt(tmp_path / name, np.ones((rows, colsn)))
        r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--realisations", "3", "--xi", str(tmp_path / name), "sim",
                            str(tmp_path / "nodes.txt"), str(tmp_path / "model"), str(tmp_path / "train.txt")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path)
        assert r.returncode != 0
        assert "--xi needs an M x S matrix" in r.stderr.decode()


@pytest.fixture(scope="module")
def normals(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim_normals") / "sim_normals_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HOST,
                           os.path.join(ROOT, "tests", "sim_normals_driver.cpp"), "-o", exe])

    def run(seed, n):
        out = subprocess.run([exe, str(seed), str(n)], stdout=subprocess.PIPE, check=True).stdout.decode().split()
        return np.array([float(v) for v in out])

    return run


def test_host_normals_are_a_function_of_the_seed(normals):
    a, b, c = normals(7, 2001), normals(7, 2001), normals(8, 2001)
    assert a.shape == (2001,) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(normals(7, 10), a[:10])                    # a prefix, whatever the count
    assert np.all(np.isfinite(a))
    # standard normal to what 2001 draws can show (standard errors 0.022 and 0.032: four of them)
    assert abs(a.mean()) < 0.09 and abs(a.var() - 1.0) < 0.13
