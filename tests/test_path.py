"""CPU tests (-m "not gpu") of simulation at any node count (gpak_condition / gpak_sample_path, `sim --method path`):
1. tests/path_ref.py, the reference of the GPU tests, restates Matheron's rule: the linear map from unit normals to the
   realisations has the latent posterior covariance of joint_ref; with the spectral prior, the closed form;
2. the host's frequency generator (gp_ss_ak_amd/host/sim_spectral.hpp, compiled alone) draws from the spectral measure of
   every profile, and is a function of its seed;
3. headers, binding and library list the same symbols; the headers are plain C;
4. the command line refuses what `sim --method path` cannot take before a context exists.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import exact_grad_ref as xref  # noqa: E402
import joint_ref  # noqa: E402
import path_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
LD = np.longdouble
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
# name -> (input columns, terms, bias, white, sn2)
COMPS = {
    "defaults": (3, [(xref.EXPANS, list(synth.DEFAULT_EXPANS))], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "d4-theta2": (4, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "expans+rbf+bias+white": (3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016),
    "exp+rbf": (3, [(xref.EXP, [0.5, 0.9]), (xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03),
}
N, M = 40, 15


def prior_variance(comp):
    _, terms, bias, white, _ = COMPS[comp]
    return bias + white + sum(p[{xref.EXPANS: 6, xref.EXP: 1, xref.RBF: 2}[k]] ** 2 for k, p in terms)


def model(comp, nd):
    cols, terms, bias, white, sn2 = COMPS[comp]
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    rng = np.random.default_rng(40 + nd)
    centres = rng.uniform(X.min(axis=0), X.max(axis=0), (M, cols))
    Xd, n = gpak.block_points(centres, (0.1, 0.1, 0.05), {1: (1, 1, 1), 8: (2, 2, 2)}[nd])
    assert n == nd
    Xd[(M - 1) * nd] = X[5]                                # a node point on a training sample
    return path_ref.Model(X, y, Xd, nd, terms, bias, white, sn2), X, y, Xd


# ---- 1. the restatement is Matheron's rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("comp,nd", [(c, nd) for c in COMPS for nd in (1, 8)], ids=[f"{c}-nd{nd}" for c in COMPS for nd in (1, 8)])
def test_conditioned_exact_prior_has_the_posterior_covariance(comp, nd):
    """Prior draws from the Cholesky factor of the exact joint prior of [node averages; noisy observations], one unit normal
    per realisation: Z - mean is the map T from the normals to the realisations, and T T' the latent covariance of
    joint_ref to 1e-10 of the prior variance."""
    cols, terms, bias, white, sn2 = COMPS[comp]
    m, X, y, Xd = model(comp, nd)
    Lc = path_ref.exact_prior_factor(m)
    Z, mean = m.condition(Lc[M:], Lc[:M])
    T = Z - mean[:, None]
    want = joint_ref.joint(X, y, Xd, nd, terms, bias, white, sn2, want_prior=False)
    err = float(np.abs(T @ T.T - want["latent"]).max()) / prior_variance(comp)
    em = float(np.abs(mean - want["mean"]).max()) / float(np.abs(y).max())
    print(f"\n{comp} nd={nd}: T T' against the latent covariance {err:.3g} of the prior variance, mean {em:.3g} of max|y|")
    assert err <= 1e-10 and em <= 1e-10
    # the map is linear in the draw and affine in y: zero draws give the mean
    Z0, _ = m.condition(np.zeros((N, 2)), np.zeros((M, 2)))
    assert float(np.abs(Z0 - mean[:, None]).max()) == 0.0


@pytest.mark.parametrize("comp,nd", [(c, nd) for c in COMPS for nd in (1, 8)], ids=[f"{c}-nd{nd}" for c in COMPS for nd in (1, 8)])
def test_conditioned_spectral_prior_has_the_closed_form_covariance(comp, nd):
    """The same with the spectral prior (24 features spread over the terms, one of order 1e4): T T' is
    K^** - G K^x* - K^*x G' + G (K^xx + (sn2 + white) I) G' with K^ from cosines of differences."""
    cols, terms, bias, white, sn2 = COMPS[comp]
    m, X, y, Xd = model(comp, nd)
    rng = np.random.default_rng(3)
    F = 24
    ft = np.arange(F) % len(terms)
    om = rng.standard_normal((F, 4)) / np.abs(rng.standard_normal((F, 1)))
    if cols == 3:
        om[:, 3] = 0.0
    om[5] *= 1e4 / np.abs(om[5]).max()
    S = 2 * F + 1 + N
    I = np.eye(S)
    Z, mean = m.sample_path(ft, om, I[:2 * F], I[2 * F], I[2 * F + 1:])
    T = Z - mean[:, None]
    err = float(np.abs(T @ T.T - m.spectral_cov(ft, om)).max()) / prior_variance(comp)
    print(f"\n{comp} nd={nd}: T T' against the closed form {err:.3g} of the prior variance")
    assert err <= 1e-10


# ---- 2. the generator --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spectral(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spectral") / "spectral_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "spectral_driver.cpp"),
                           "-o", exe])

    def run(*args):
        return subprocess.run([exe, *[str(a) for a in args]], stdout=subprocess.PIPE, check=True).stdout

    return run


@pytest.mark.parametrize("profile,iw", [(0, 0.0), (1, 0.9), (1, 2.5)], ids=["expsqrt", "rbf-iw0.9", "rbf-iw2.5"])
@pytest.mark.parametrize("dim", [3, 4])
def test_frequencies_reproduce_the_profile(spectral, profile, iw, dim):
    """F = 16384 frequencies, 200 lags: max |K^(h) - k(h)| <= 5 / sqrt(F) per unit variance (Hoeffding: 4e-4 over the lags)."""
    F = 16384
    out = spectral("freq", 11 + dim, F, dim, profile, iw)
    rows = np.array([[float(v) for v in line.split()] for line in out.decode().splitlines()])
    assert rows.shape == (F, 5) and np.all(rows[:, 0] == 0)
    om = rows[:, 1:]
    if dim == 3:
        assert np.all(om[:, 3] == 0.0)
    rng = np.random.default_rng(5)
    h = rng.standard_normal((200, 4))
    h[:, dim:] = 0.0
    h *= (rng.uniform(0.0, 4.0, 200) / np.linalg.norm(h, axis=1))[:, None]       # lags of length 0 .. 4
    Khat = np.cos(h @ om.T).mean(axis=1)
    r = np.linalg.norm(h, axis=1)
    k = np.exp(-r) if profile == 0 else np.exp(-0.5 * iw * r * r)
    err = float(np.abs(Khat - k).max())
    print(f"\nprofile {profile} iw {iw} dim {dim}: max |K^ - k| = {err:.4f} against {5 / np.sqrt(F):.4f}")
    assert err <= 5 / np.sqrt(F)
    assert spectral("freq", 11 + dim, F, dim, profile, iw) == out                  # the same seed: the same bytes
    assert spectral("freq", 12 + dim, F, dim, profile, iw) != out


def test_stream_is_the_sequence_of_the_sim_normals(spectral):
    v = np.array([float(t) for t in spectral("stream", 7, 1001).decode().split()])
    assert v.shape == (2002,) and np.array_equal(v[:1001], v[1001:])


# ---- 3. headers, binding, library ------------------------------------------------------------------------------------------
def header_functions(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gpak_[a-z0-9_]+)\s*\(", txt))


def test_headers_binding_and_library_list_the_same_symbols():
    call, dev = header_functions("gpak_condition.h"), header_functions("gpak_dev_condition.h")
    assert call == set(_lib.CONDITION_SYMBOLS) == {"gpak_condition", "gpak_sample_path"}
    assert dev == set(_lib.DEV_CONDITION_SYMBOLS) and "gpak_dev_kmm" in dev
    assert not (call | dev) & header_functions("gpak.h")              # gpak.h does not declare or include them
    assert "gpak_condition.h" not in open(os.path.join(ROOT, "include", "gpak.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in call | dev:
        assert hasattr(lib, name), name
    assert [n for n, _ in _lib.ConditionSummary._fields_] == ["solve_ms", "prior_ms", "product_ms", "batches", "fused"]
    assert callable(gpak.Gpak.condition) and callable(gpak.Gpak.sample_path) and gpak.COND_UNFUSED == 1
    # NULL arguments are refused without a device
    vp = ctypes.c_void_p
    lib.gpak_condition.argtypes = [vp, vp, ctypes.c_long, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp]
    assert lib.gpak_condition(None, None, 1, 1, 3, None, None, 1, None, None, 0, None) == gpak.EINVAL
    lib.gpak_dev_kmm.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_double,
                                 ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_long, vp, ctypes.c_long, vp]
    assert lib.gpak_dev_kmm(None, None, 256, 1, 1, None, 128, 1, None, 0.0, 1, None, 1, 1, None, 0, None, 1, None) == gpak.EINVAL
    # the slabs are a function of the padded sample count alone
    assert [lib.gpak_dev_kmm_slabs(n) for n in (1, 300, 512, 513, 1000, 32768)] == [1, 1, 1, 2, 2, 16]
    assert [lib.gpak_dev_kmm_slab_len(n) for n in (300, 1000, 32768)] == [512, 512, 2048]


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_condition.h"\n#include "gpak_dev_condition.h"\n'
                   'int main(void){gpak_condition_summary s; s.fused = GPAK_COND_UNFUSED; (void)s; '
                   'if (gpak_dev_kmm(0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'if (gpak_sample_path(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_condition(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


# ---- 4. the command line: everything is refused before a context exists (no model file is ever read) ----------------------
def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


FILES = ["nodes.txt", "model", "train.txt"]


@pytest.mark.parametrize("args,msg", [
    (["--realisations", "3", "--xi", "xi.txt", "sim", "--method", "path", *FILES], "drop --xi"),
    (["--realisations", "3", "--seed", "1", "--xi", "xi.txt", "sim", "--method", "path", *FILES], "drop --xi"),
    (["--realisations", "3", "--seed", "1", "--nugget", "0.1", "sim", "--method", "path", *FILES], "drop --nugget"),
    (["--realisations", "3", "--seed", "1", "--nugget", "0", "sim", "--method", "path", *FILES], "drop --nugget"),
    (["--realisations", "3", "sim", "--method", "path", *FILES], "sim --method path needs --seed n"),
    (["--gpus", "2", "--realisations", "3", "--seed", "1", "sim", "--method", "path", *FILES], "single-GPU context"),
    (["--realisations", "3", "--seed", "1", "sim", "--method", "paths", *FILES], "--method takes joint or path"),
    (["--realisations", "3", "--seed", "1", "sim", "--method", "path", "--features", "0", *FILES], "--features takes the number"),
    (["sim", "--method", "path", "--seed", "1", *FILES], "sim needs --realisations S with S > 0"),
    (["sim", "--method", "path", "--seed", "1", "--realisations", "3", "nodes.txt", "model"], "not enough input parameters"),
])
def test_cli_refuses_what_the_path_method_cannot_take(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode(), r.stderr.decode()


def test_cli_path_method_passes_its_checks_up_to_the_model(tmp_path):
    """With correct files the verb gets as far as the model file, which is not there."""
    build()
    with open(tmp_path / "nodes.txt", "w") as f:
        f.write("# x, y, z, grade\n" + "".join(f"{i}\t{2 * i}\t{3 * i}\t0.5\n" for i in range(5)))
    with open(tmp_path / "train.txt", "w") as f:
        f.write("# x, y, z, grade\n" + "".join(f"{i}\t{2 * i}\t{3 * i}\t{0.5 * i}\n" for i in range(10)))
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--block-size", "1,1,1", "--block-disc", "2,2,2", "sim", "-np", "--method", "path",
                        "--features", "256", "--realisations", "4", "--seed", "1", *FILES], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode != 0 and "--" not in err and "model" in err, err
