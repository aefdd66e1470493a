"""GPU tests (-m gpu) of gpak_grad_exact and of `gp_ss_ak --gradient exact train`.

The reference for the gradient is tests/exact_grad_ref.py (NumPy, full dK/dtheta matrices), itself pinned against finite
differences of the CPU checker's nlZ in tests/test_exact_grad.py; at sizes where that restatement is out of reach the
device gradient is checked against differences of the device's own objective along fixed directions.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import exact_grad_ref as xref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
IS_ANGLE = [True, False, True, False, True, False, False, False, False, False]
X0 = E + [synth.DEFAULT_BIAS, synth.DEFAULT_SN2]

# (id, N, input columns, terms, bias, sn2)
CASES = []
for _n in (64, 200, 512, 1000, 2500):
    CASES.append((f"N{_n}-defaults", _n, 3, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2))
    CASES.append((f"N{_n}-theta2", _n, 3, [(xref.EXPANS, THETA2)], 0.35, 0.05))
for _n in (512, 1000):
    CASES.append((f"N{_n}-d4-defaults", _n, 4, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2))
    CASES.append((f"N{_n}-d4-theta2", _n, 4, [(xref.EXPANS, THETA2)], 0.35, 0.05))
CASES.append(("N512-expans+exp", 512, 3, [(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.016))
CASES.append(("N512-expans+rbf+bias", 512, 3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.016))
CASES.append(("N512-rbf", 512, 3, [(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.03))
CASES.append(("N512-d4-exp+rbf+bias", 512, 4, [(xref.EXP, [0.7, 0.6]), (xref.RBF, [0.5, 0.9, 0.5])], 0.1, 0.02))


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(gp, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        gp.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        gp.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exact_gradient_matches_numpy_restatement(gp, case):
    """Bound 1e-8 (the project's gradient tolerance) per group: the kernel blocks' entries relative
    to their largest, the bias entry and the sn2 entry each relative to itself -- one overall scale would let the sn2
    entry (10^3 times the others) hide the rest."""
    name, N, cols, terms, bias, sn2 = case
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    want = xref.grad_exact(X, y, terms, bias, sn2)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2)
    nlz = gp.logLikelihood()
    got = gp.GradLL_exact(len(want))
    assert gp.logLikelihood() == nlz                                  # factor, alpha and nlZ stay valid
    nk = len(want) - 2
    ek = np.abs(got[:nk] - want[:nk]).max() / np.abs(want[:nk]).max()
    eb = abs(got[nk] - want[nk]) / abs(want[nk])
    es = abs(got[nk + 1] - want[nk + 1]) / abs(want[nk + 1])
    print(f"\n{name}: kernel block {ek:.3g}, bias {eb:.3g}, sn2 {es:.3g} (relative)\n  got  {got}\n  want {want}")
    assert ek <= 1e-8 and eb <= 1e-8 and es <= 1e-8
    if cols == 3 and terms[0][0] == xref.EXPANS:
        assert got[7] == 0.0
    assert np.array_equal(gp.GradLL_exact(len(want)), got)            # fixed-order reduction: repeatable bit for bit
    with pytest.raises(gpak.GpakError) as ei:
        gp.GradLL_exact(len(want) + 1)
    assert ei.value.status == gpak.EINVAL


V1 = np.ones(10) / np.sqrt(10.0)
V2 = np.array([1.0, -2.0, 3.0, -1.0, 2.0, -3.0, 1.0, 0.0, 2.0, 0.0])
V2 = V2 / np.linalg.norm(V2)


@pytest.mark.parametrize("N", [8192, 32768])
def test_exact_gradient_against_differences_of_the_device_objective(gp, N):
    """g.v for two fixed unit directions (V1: all ten parameters alike; V2: kernel parameters and bias only, so that the
    sn2 entry cannot carry it) against (4 c(h/2) - c(h)) / 3 of the central differences of gpak_nlz along v, h = 1e-4.
    Bound 1e-6 of |g|_inf: the noise floor of the differences is eps |nlZ| / h ~ 7e-8 absolute on entries >= 10^3."""
    X, y = synth.drillholes(N)
    gp.set_train(X, y)
    x0 = np.array(X0)

    def nlz(x):
        gp.set_params(x[:8], float(x[8]), float(x[9]), gpak.DIST_DIRECT)
        return gp.logLikelihood()

    f0 = nlz(x0)
    g = gp.GradLL_exact()
    assert gp.logLikelihood() == f0
    for name, v in (("V1", V1), ("V2", V2)):
        c = [(nlz(x0 + h * v) - nlz(x0 - h * v)) / (2 * h) for h in (1e-4, 5e-5)]
        fd = (4 * c[1] - c[0]) / 3
        err = abs(float(g @ v) - fd)
        print(f"\nN={N} {name}: g.v = {float(g @ v):.12g}, differences {fd:.12g}, |err| / |g|inf = {err / np.abs(g).max():.3g}")
        assert err <= 1e-6 * np.abs(g).max()
    print(f"  g = {g}\n  grad_ms = {gp.timing()['grad_ms']:.2f}")


def test_reference_gradient_and_objective_are_untouched(gp):
    N = 700
    X, y = synth.drillholes(N)
    gp.set_train(X, y)
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    nlz = gp.logLikelihood()
    before = gp.GradLL()
    exact = gp.GradLL_exact()
    assert gp.timing()["grad_ms"] > 0
    after = gp.GradLL()
    assert np.array_equal(before, after) and gp.logLikelihood() == nlz
    assert not np.allclose(exact, before, rtol=1e-3)                  # they are different quantities
    # a fresh evaluation at the same parameters: gpak_grad_exact alone brings gram / factor / alpha up to date
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    assert np.array_equal(gp.GradLL_exact(), exact) and gp.logLikelihood() == nlz
    # a White child: not built (a context cannot tell a White of 0 from none)
    gp.set_kernel([(gpak.KERN_EXPANS, E)], 0.2, 0.1, 0.016, gpak.DIST_DIRECT)
    with pytest.raises(gpak.GpakError) as ei:
        gp.GradLL_exact()
    assert ei.value.status == gpak.ENOTIMPL and "White" in str(ei.value)
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def test_multi_gpu_context_refuses_the_exact_gradient():
    X, y = synth.drillholes(256)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X, y)
        m.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
        with pytest.raises(gpak.GpakError) as ei:
            m.GradLL_exact()
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def run_train(tmp_path, tag, Xs, ys, maxit, extra_args=()):
    d = tmp_path / tag
    d.mkdir()
    write_csv(d / "train.txt", Xs, ys)
    tr = d / "trace.txt"
    env = dict(os.environ, GPAK_MAX_ITERS=str(maxit), GPAK_OPT_TRACE=str(tr))
    env.pop("GPAK_OPT", None)
    cmd = [os.path.join(HOST, "gp_ss_ak"), "-v", "1", "-np", *extra_args, "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS",
           str(d / "train.txt"), str(d / "model")]
    out = subprocess.run(cmd, env=env, cwd=d, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    stats = np.loadtxt(str(d / "model") + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)     # the standardisation was the identity
    rows = [[float(v) for v in line.split()] for line in open(tr)]
    printed = [float(line.split("-logL:")[1]) for line in out.splitlines() if line.startswith("Iteration:")]
    return rows, printed, open(d / "model").read()


def test_cli_exact_mode_trains_where_the_reference_mode_stalls(gp, tmp_path):
    """N = 512, 12 iterations, both modes.  The port (exact_grad_ref.projected_lbfgs) is driven by the SAME device
    objective and gradient through the Python binding, on bit-identical inputs."""
    import make_golden_lbfgs
    build()
    N, maxit = 512, 12
    Xs, ys = make_golden_lbfgs.prepared(N)
    ref_rows, _, _ = run_train(tmp_path, "reference", Xs, ys, maxit)
    rows, printed, model = run_train(tmp_path, "exact", Xs, ys, maxit, ("--gradient", "exact"))
    ref_rows2, _, _ = run_train(tmp_path, "reference2", Xs, ys, maxit, ("--gradient", "reference"))
    assert ref_rows2 == ref_rows                                      # the default IS the reference mode
    obj, evals = [r[1] for r in rows], [int(r[2]) for r in rows]
    print(f"\nexact     {obj}\n  evals   {evals}\nreference {[r[1] for r in ref_rows]}\n  evals   {[int(r[2]) for r in ref_rows]}")
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and len(rows) <= maxit
    assert all(b < a for a, b in zip(obj, obj[1:])) and len(set(obj)) >= 8
    assert obj[-1] < ref_rows[-1][1]
    assert 2 * evals[-1] <= int(ref_rows[-1][2])
    for p, o in zip(printed, obj):
        assert abs(p - o) <= 1e-5 * abs(o)
    assert "KernelName=ExpAns" in model

    gp.set_train(Xs, ys)

    def fun(x):
        gp.set_params(np.array(x[:8], dtype=float), float(x[8]), float(x[9]), gpak.DIST_DIRECT)
        return gp.logLikelihood()

    port = []
    xref.projected_lbfgs(fun, lambda x: gp.GradLL_exact(), X0, IS_ANGLE, maxit, trace=port)
    assert [n for _, n, _ in port] == evals
    assert all(abs(h - o) <= 1e-8 * abs(h) for (h, _, _), o in zip(port, obj))
    assert all(np.abs(xk - np.array(r[3:])).max() <= 1e-7 for (_, _, xk), r in zip(port, rows))
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def test_cli_exact_mode_at_8192_vs_oracle_fixture(tmp_path):
    """tests/golden/golden_exact_lbfgs_N8192.json (make_golden_exact.py: the port over the CPU checker's objective and the
    NumPy gradient, no HIP).  Objectives to 1e-7 relative and equal evaluation counts through every row up to the first
    whose counts differ; that row must not come before row 4."""
    import make_golden_lbfgs
    build()
    with open(os.path.join(ROOT, "tests", "golden", "golden_exact_lbfgs_N8192.json")) as fh:
        z = json.load(fh)
    N, ref = z["N"], z["rows"]
    assert len({r["objective"] for r in ref}) >= 5
    Xs, ys = make_golden_lbfgs.prepared(N)
    rows, _, _ = run_train(tmp_path, "exact", Xs, ys, z["maxit"], ("--gradient", "exact"))
    obj, evals = [r[1] for r in rows], [int(r[2]) for r in rows]
    print(f"\nN={N} CLI    {obj}\n  evals  {evals}\n  oracle {[r['objective'] for r in ref]}\n  evals  {[r['evaluations'] for r in ref]}")
    agree = 0
    for row, r in zip(rows, ref):
        if int(row[2]) != r["evaluations"]:
            break
        assert abs(row[1] - r["objective"]) <= 1e-7 * abs(r["objective"])
        agree += 1
    assert agree >= min(3, len(ref))                                  # the first differing row is row 4 or later
    assert all(b < a for a, b in zip(obj, obj[1:]))
