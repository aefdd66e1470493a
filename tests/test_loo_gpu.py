"""GPU tests (-m gpu) of gpak_loo and of `gp_ss_ak cv`.

The reference is tests/loo_ref.py (NumPy, one Cholesky), itself pinned against brute-force refits and the CPU checker's
predict in tests/test_loo.py; at sizes where it is out of reach, entry i is compared with the device's own prediction
of x_i from the other N - 1 samples.  Bound throughout: the project's 1e-8 (alpha, mean,
variance), means relative to max|y|, variances relative per element.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
BOUND = 1e-8

# (id, N, input columns, terms, bias, white, sn2)
CASES = []
for _n in (64, 200, 513, 1000, 2500):   # 200: padded to 256; 513: one row past a 512-column chunk, padded to 640
    CASES.append((f"N{_n}-defaults", _n, 3, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2))
    CASES.append((f"N{_n}-theta2", _n, 3, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05))
for _n in (300, 512):
    CASES.append((f"N{_n}-d4-defaults", _n, 4, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2))
    CASES.append((f"N{_n}-d4-theta2", _n, 4, [(xref.EXPANS, THETA2)], 0.35, 0.0, 0.05))
CASES.append(("N512-expans+exp", 512, 3, [(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.0, 0.016))
CASES.append(("N512-rbf", 512, 3, [(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03))
CASES.append(("N512-expans+rbf+bias+white", 512, 3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016))


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(g, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        g.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def errors(y, mean, var, want_mean, want_var):
    return np.abs(mean - want_mean).max() / np.abs(y).max(), (np.abs(var - want_var) / want_var).max()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_loo_matches_numpy_restatement(gp, case):
    name, N, cols, terms, bias, white, sn2 = case
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    wm, wv = loo_ref.loo(loo_ref.add_white(xref.gram(X, terms, bias), white), y, sn2)
    want = loo_ref.summary(y, wm, wv)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    mean, var, s = gp.loo()
    em, ev = errors(y, mean, var, wm, wv)
    es = max(abs(s[k] - want[k]) / abs(want[k]) for k in ("mse", "mssr", "log_pl"))
    print(f"\n{name}: mean {em:.3g} of max|y|, variance {ev:.3g} relative, summary {es:.3g} relative; "
          f"mse {s['mse']:.6g} mssr {s['mssr']:.6g} log_pl {s['log_pl']:.6g} passes {s['passes']}")
    assert s["status"] == gpak.OK
    assert em <= BOUND and ev <= BOUND and es <= BOUND
    if white != 0.0:   # LOO works where the gradients refuse
        with pytest.raises(gpak.GpakError) as ei:
            gp.GradLL_exact(13)
        assert ei.value.status == gpak.ENOTIMPL
        set_defaults(gp)


def same_bytes(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and all(a[2][k] == b[2][k] for k in ("mse", "mssr", "log_pl")))


def test_result_does_not_depend_on_the_pass_count(gp):
    """N = 1000: 8 row tiles.  One pass, 8 passes of one tile, 3 passes of 3 / 3 / 2 tiles, and one pass in the gradient's
    workspace: the same bytes."""
    X, y = synth.drillholes(1000)
    gp.set_train(X, y)               # releases the gradient's workspaces
    set_defaults(gp)
    runs = []
    try:
        for rows, passes in ((0, 1), (128, 8), (384, 3)):
            gp.set_option(gpak.OPT_LOO_ROWS, rows)
            runs.append(gp.loo())
            assert runs[-1][2]["passes"] == passes
        gp.GradLL_exact()            # allocates dG
        runs.append(gp.loo())
        assert runs[-1][2]["passes"] == 1
    finally:
        gp.set_option(gpak.OPT_LOO_ROWS, 0)
    for k, r in enumerate(runs[1:], 1):
        dm = np.abs(r[0] - runs[0][0]).max()
        dv = (np.abs(r[1] - runs[0][1]) / runs[0][1]).max()
        print(f"\nvariant {k} against one pass: mean differs by {dm:.3g}, variance by {dv:.3g} relative")
    assert all(same_bytes(r, runs[0]) for r in runs[1:])


def test_loo_leaves_the_context_state_alone(gp):
    X, y = synth.drillholes(700)
    gp.set_train(X, y)
    set_defaults(gp)
    nlz = gp.logLikelihood()
    g_ref, g_exact = gp.GradLL(), gp.GradLL_exact()
    first = gp.loo()
    assert first[2]["ms"] > 0 and first[2]["passes"] == 1
    assert gp.logLikelihood() == nlz
    assert same_bytes(gp.loo(), first)                                   # two calls: the same bytes
    assert np.array_equal(gp.GradLL(), g_ref) and np.array_equal(gp.GradLL_exact(), g_exact)   # shared workspace
    assert same_bytes(gp.loo(), first)
    # loo() alone after fresh parameters brings gram / factor / alpha up to date
    set_defaults(gp)
    assert same_bytes(gp.loo(), first) and gp.logLikelihood() == nlz
    # without the gradient's workspace, in slabs
    gp.set_train(X, y)
    set_defaults(gp)
    gp.set_option(gpak.OPT_LOO_ROWS, 256)
    try:
        sl = gp.loo()
    finally:
        gp.set_option(gpak.OPT_LOO_ROWS, 0)
    assert sl[2]["passes"] == 3 and same_bytes(sl, first)
    assert np.array_equal(gp.GradLL_exact(), g_exact) and gp.logLikelihood() == nlz


@pytest.mark.parametrize("N,left_out", [(8192, (0, 4095, 8191)), (32768, (0, 32767))])
def test_loo_against_prediction_on_the_reduced_set(gp, N, left_out):
    """Entry i of loo() on the full set against posteriorMeanVar at x_i after set_train without sample i (compat = 0 adds
    sn2).  The first row has the longest sum of squares, the last a single term."""
    X, y = synth.drillholes(N)
    gp.set_train(X, y)
    set_defaults(gp)
    mean, var, s = gp.loo()
    print(f"\nN={N}: loo {s['ms']:.1f} ms in {s['passes']} pass(es); mse {s['mse']:.6g} mssr {s['mssr']:.6g}")
    try:
        for i in left_out:
            keep = np.arange(N) != i
            gp.set_train(X[keep], y[keep])
            set_defaults(gp)
            m, v = gp.posteriorMeanVar(X[i:i + 1], compat=0)
            em, ev = abs(m[0] - mean[i]) / np.abs(y).max(), abs(v[0] - var[i]) / v[0]
            print(f"  i={i}: mean {em:.3g} of max|y|, variance {ev:.3g} relative")
            assert em <= BOUND and ev <= BOUND
    finally:
        set_defaults(gp)


def test_statuses(gp):
    fresh = gpak.Gpak(0)
    try:
        with pytest.raises(gpak.GpakError) as ei:
            fresh.loo()
        assert ei.value.status == gpak.ESTATE
        with pytest.raises(gpak.GpakError) as ei:
            fresh.set_option(gpak.OPT_LOO_ROWS, 100)
        assert ei.value.status == gpak.EINVAL
        with pytest.raises(gpak.GpakError) as ei:
            fresh.set_option(gpak.OPT_LOO_ROWS, -128)
        assert ei.value.status == gpak.EINVAL
    finally:
        fresh.close()
    X, y = synth.drillholes(512)
    gp.set_train(X, y)
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    mean, var, s = gp.loo()
    assert s["status"] == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var)) and all(np.isnan(s[k]) for k in ("mse", "mssr", "log_pl"))
    set_defaults(gp)
    good = gp.loo()                                                     # recovery at valid parameters
    assert good[2]["status"] == gpak.OK and np.all(np.isfinite(good[0])) and np.all(good[1] > synth.DEFAULT_SN2)
    f32 = gpak.Gpak(0, precision=gpak.F32)                              # LOO is fp64 whatever the context's precision
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        assert same_bytes(f32.loo(), good)
    finally:
        f32.close()
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X[:256], y[:256])
        set_defaults(m)
        with pytest.raises(gpak.GpakError) as ei:
            m.loo()
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def test_cli_cv_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then cv on the same file.  The standardisation of this set is the identity, so
    the file's columns are loo()'s mean and the square root of its variance (Control::postData_var returns a standard
    deviation, as in _predict.txt), at the file's six digits."""
    import make_golden_lbfgs
    build()
    N = 512
    Xs, ys = make_golden_lbfgs.prepared(N)
    write_csv(tmp_path / "train.txt", Xs, ys)
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    out = subprocess.run([exe, "-v", "1", "cv", "-np", str(tmp_path / "train.txt"), model], cwd=tmp_path, input=b"",
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    quiet = subprocess.run([exe, "-v", "0", "cv", str(tmp_path / "train.txt"), model, str(tmp_path / "other.txt")], cwd=tmp_path,
                           input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    assert open(tmp_path / "other.txt").read() == open(model + "_loo.txt").read()
    assert open(model + "_loo.txt").readline() == "# SampleNo, Y, Yloo, VarYloo, Inputs\n"
    rows = np.loadtxt(model + "_loo.txt", comments="#")
    assert rows.shape == (N, 7) and np.array_equal(rows[:, 0], np.arange(1, N + 1))     # input order

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    mean, var, s = gp.loo()
    set_defaults(gp)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b))

    assert close(rows[:, 1], ys) and close(rows[:, 2], mean) and close(rows[:, 3], np.sqrt(var)) and close(rows[:, 4:], Xs)
    printed = {k: float(out.split(k)[1].split()[0]) for k in ("Mean Square Error of leave-one-out:", "Var MSE Train:",
                                                               "Mean standardised squared residual:", "Log pseudo-likelihood:",
                                                               "LOO ms:")}
    file_mse = float(np.mean((rows[:, 1] - rows[:, 2]) ** 2))
    print(f"\ncv: {printed}; mean of the file's squared residuals {file_mse:.6g}; loo() {s}")
    assert abs(printed["Mean Square Error of leave-one-out:"] - file_mse) <= 1e-4 * file_mse   # both from 6-digit columns
    assert abs(printed["Mean Square Error of leave-one-out:"] - s["mse"]) <= 1e-5 * s["mse"]
    assert abs(printed["Mean standardised squared residual:"] - s["mssr"]) <= 1e-5 * s["mssr"]
    assert abs(printed["Log pseudo-likelihood:"] - s["log_pl"]) <= 1e-5 * abs(s["log_pl"])
    assert abs(printed["Var MSE Train:"] - np.var(ys)) <= 1e-5 * np.var(ys) and printed["LOO ms:"] > 0
    assert [float(v) for v in quiet.split()] == [printed[k] for k in list(printed)[:4]]   # -v 0: the bare numbers
