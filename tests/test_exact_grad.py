"""CPU tests (-m "not gpu") of the exact-gradient feature:

1. tests/exact_grad_ref.py (the NumPy restatement gpak_grad_exact is compared with on the GPU) against
   Richardson-extrapolated central differences of the CPU checker's nlZ;
2. Opt_Algs::ProjectedLBFGSOptimise (host_selftest --opt-exact) against its Python port on an analytic objective;
3. the `--gradient` option of the command line refuses what it cannot do.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_grad_ref as xref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

DEFAULTS = (list(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2)
THETA2 = ([0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9], 0.35, 0.05)


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def fd_gradient(orc, X, y, terms, bias, sn2):
    """(4 c(h/2) - c(h)) / 3 of the central differences c at h = 1e-4: truncation O(h^4)."""
    sizes = [len(p) for _, p in terms]
    flat = np.concatenate([np.asarray(p, dtype=float) for _, p in terms] + [[bias, sn2]])

    def nlz(v):
        tt, o = [], 0
        for (k, _), n in zip(terms, sizes):
            tt.append((k, v[o:o + n]))
            o += n
        if len(tt) == 1 and tt[0][0] == 0:
            K = orc.gram(X, X, tt[0][1], v[o], orc.DIST_DIRECT)
        else:
            K = orc.gram_hyb(X, X, tt, v[o], 0.0, orc.DIST_DIRECT)
        info, _, _ = orc.nlz_lean(K, y, v[o + 1], want_L=False)
        assert not info.chol_fail
        return info.nlz

    def central(i, h):
        a, b = flat.copy(), flat.copy()
        a[i] += h
        b[i] -= h
        return (nlz(a) - nlz(b)) / (2 * h)

    return np.array([(4 * central(i, 5e-5) - central(i, 1e-4)) / 3 for i in range(len(flat))])


CASES = [(N, cols, name) for N in (64, 256) for cols in (3, 4) for name in ("defaults", "theta2")] + [(64, 3, "hyb")]


@pytest.mark.parametrize("N,cols,name", CASES)
def test_restatement_is_the_derivative_of_the_oracle_objective(orc, N, cols, name):
    """Bounds: 1e-8 of the largest entry overall and 1e-6 of the largest of entries 0-7 -- the truncation of the
    extrapolated differences with about 25 x margin (measured <= 4e-10 and <= 1.4e-8)."""
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    if name == "hyb":
        terms, bias, sn2 = [(xref.EXPANS, DEFAULTS[0]), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.016
    else:
        e, bias, sn2 = DEFAULTS if name == "defaults" else THETA2
        terms = [(xref.EXPANS, e)]
    g = xref.grad_exact(X, y, terms, bias, sn2)
    fd = fd_gradient(orc, X, y, terms, bias, sn2)
    err = np.abs(g - fd)
    print(f"\nN={N} d={cols} {name}: max|g - fd| / max|g| = {err.max() / np.abs(g).max():.3g}, "
          f"entries 0-7: {err[:8].max() / np.abs(g[:8]).max():.3g}\n  g  = {g}\n  fd = {fd}")
    assert err.max() <= 1e-8 * np.abs(g).max()
    assert err[:8].max() <= 1e-6 * np.abs(g[:8]).max()
    if cols == 3:
        assert g[7] == 0.0                                   # InversewidthR has nothing to act on
    if name == "defaults":
        assert abs(g[0]) <= 1e-6 * np.abs(g).max()           # Lx = Ly: the metric does not depend on AngleX
    if name == "theta2":
        assert abs(g[0]) > 1e-6 * np.abs(g).max()


def quad_objective(variant):
    cfg = {0: ([1.5, 0.9, 2.5, 0.3, 4.0, 1.1], [1.0, 3.0, 0.5, 2.0, 0.25, 1.5], [2.0, 7.0, -1.0, 0.5, 3.0, 5.5]),
           1: ([0.5] * 6, [0.2, 0.4, 0.6, 0.8, 1.0, 1.2], [1.0, 2.0, 3.0, 4.0, 5.0, 5.9]),
           2: ([5.5, 0.01, 3.0, 3.0, 0.2, 2.2], [2.0, 0.1, 1.0, 1.0, 3.0, 0.7], [8.0, -2.0, 3.1, 2.9, 0.1, 2.0])}
    x0, w, c = cfg[variant]

    def fg(x):
        x = [float(v) for v in x]
        f, g = 0.0, [0.0] * 6
        for i in range(6):
            f += w[i] * (x[i] - c[i]) * (x[i] - c[i]) + 0.01 * x[i] * x[i] * x[i] * x[i]
            g[i] = 2 * w[i] * (x[i] - c[i]) + 0.04 * x[i] * x[i] * x[i]
        for i in range(5):
            f += 0.05 * x[i] * x[i + 1]
            g[i] += 0.05 * x[i + 1]
            g[i + 1] += 0.05 * x[i]
        return f, np.array(g)

    return x0, fg


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_projected_driver_matches_its_python_port(variant):
    """host_selftest --opt-exact: QuadModel of the existing --opt mode, variable 2 named like an angle (kept linear),
    the others optimised in their logarithm.  Same iteration and evaluation counts, objectives to 1e-12 relative."""
    build()
    x0, fg = quad_objective(variant)
    maxit = 25
    xr, hist, nfev = xref.projected_lbfgs(lambda x: fg(x)[0], lambda x: fg(x)[1], x0,
                                          [i == 2 for i in range(6)], maxit)
    out = subprocess.check_output([os.path.join(HOST, "host_selftest"), "--opt-exact", str(maxit), str(variant)]).decode()
    lines = out.splitlines()
    ch = [float(l.split("-logL:")[1]) for l in lines if l.startswith("Iteration")]
    xf = [float(v) for v in [l for l in lines if l.startswith("FINAL")][0].split()[1:]]
    nf = int([l for l in lines if l.startswith("NFEV")][0].split()[1])
    print(f"\nvariant {variant}: {len(ch)} iterations, {nf} evaluations, objective {fg(x0)[0]:.6g} -> {ch[-1]:.12g}")
    assert len(ch) == len(hist) and nf == nfev
    assert all(abs(a - b) <= 1e-12 * abs(a) for a, b in zip(hist, ch))
    assert np.abs(np.array(xf) - xr).max() <= 1e-10
    assert all(b < a for a, b in zip([fg(x0)[0]] + ch, ch))          # Armijo: every kept objective is a decrease
    assert all(1e-4 * (1 - 1e-15) <= v <= 6.0 * (1 + 1e-15) for v in xf)
    assert len(ch) >= 5 and nf >= len(ch) + 1


@pytest.mark.parametrize("args,msg", [
    (["--gradient", "bogus", "train", "x.txt"], "--gradient takes reference or exact"),
    (["--gradient", "exact", "--gpus", "2", "train", "x.txt"], "one GPU only"),
    (["--gpus", "2", "--gradient", "exact", "train", "x.txt"], "one GPU only"),
])
def test_cli_refuses_bad_gradient_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()
