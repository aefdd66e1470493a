"""GPU tests (-m gpu) of gpak_loo_grad and of `gp_ss_ak --objective loo train`.

The reference for the gradient is tests/loo_grad_ref.py (NumPy: the weight matrix W of the pseudo-likelihood from one
Cholesky factor, contracted with the full dK/dtheta matrices by exact_grad_ref.grad_exact), itself pinned against central
differences of loo_ref's log_pl in tests/test_loo_grad.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ctx_sequences as cs  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import loo_grad_model as lgm  # noqa: E402
import loo_grad_ref as lref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

MODEL_CACHE = {}
E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]

# (id, N, input columns, terms, bias, sn2): the compositions of tests/test_exact_grad_gpu.py.  200: padded to 256;
# 513: one row past a 512-column chunk, padded to 640; 2500: K > 2048 in the product, several chunks
CASES = []
for _n in (64, 200, 513, 1000, 2500):
    CASES.append((f"N{_n}-defaults", _n, 3, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2))
    CASES.append((f"N{_n}-theta2", _n, 3, [(xref.EXPANS, THETA2)], 0.35, 0.05))
CASES.append(("N512-d4-defaults", 512, 4, [(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2))
CASES.append(("N512-d4-theta2", 512, 4, [(xref.EXPANS, THETA2)], 0.35, 0.05))
CASES.append(("N512-expans+exp", 512, 3, [(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.016))
CASES.append(("N512-expans+rbf+bias", 512, 3, [(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.016))
CASES.append(("N512-rbf", 512, 3, [(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.03))


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(g, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        g.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def same_summary(a, b):
    return all(a[k] == b[k] for k in ("mse", "mssr", "log_pl", "passes"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_loo_gradient_matches_numpy_restatement(gp, case):
    """Per group, as the exact gradient: the kernel blocks' entries <= 1e-8 of their largest, the sn2 entry <= 1e-8 of
    itself, InversewidthR exactly 0 for 3 columns.  The bias entry is 1/2 sum W, which cancels by about 10^8 (about 0.01
    against 1/2 sum |W| ~ 10^6): it is bounded by 1e-8 |want| + 1e-15 * 1/2 sum_ij |W_ij| with W from the restatement --
    the second term is about 9 units of roundoff on the sum's own condition.  Both units are printed."""
    name, N, cols, terms, bias, sn2 = case
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    want, W = lref.grad_loo(X, y, terms, bias, sn2, want_w=True)
    half_abs = 0.5 * float(np.abs(W).sum())
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2)
    nlz = gp.logLikelihood()
    got, s = gp.loo_grad(len(want))
    assert s["status"] == gpak.OK and gp.logLikelihood() == nlz       # factor, alpha and nlZ stay valid
    nk = len(want) - 2
    ek = np.abs(got[:nk] - want[:nk]).max() / np.abs(want[:nk]).max()
    eb = abs(got[nk] - want[nk])
    es = abs(got[nk + 1] - want[nk + 1]) / abs(want[nk + 1])
    print(f"\n{name}: kernel block {ek:.3g}, sn2 {es:.3g} (relative); bias entry {want[nk]:.6g}: error {eb / abs(want[nk]):.3g} "
          f"of itself, {eb / half_abs:.3g} of 1/2 sum|W| = {half_abs:.6g}\n  got  {got}\n  want {want}")
    assert ek <= 1e-8 and es <= 1e-8
    assert eb <= 1e-8 * abs(want[nk]) + 1e-15 * half_abs
    if cols == 3 and terms[0][0] == xref.EXPANS:
        assert got[7] == 0.0
    again, s2 = gp.loo_grad(len(want))                                # fixed-order reductions: repeatable bit for bit
    assert np.array_equal(again, got) and same_summary(s, s2)
    assert same_summary(s, gp.loo()[2]) and s["passes"] == 1          # the summary is gpak_loo's
    assert abs(-s["log_pl"] - lref.objective(X, y, terms, bias, sn2)) <= 1e-8 * abs(s["log_pl"])
    with pytest.raises(gpak.GpakError) as ei:
        gp.loo_grad(len(want) + 1)
    assert ei.value.status == gpak.EINVAL


def snapshot(gp):
    mean, var, s = gp.loo()
    return (gp.logLikelihood(), gp.GradLL(), gp.GradLL_exact(), mean, var, {k: s[k] for k in ("mse", "mssr", "log_pl", "passes")})


def same_snapshot(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and np.array_equal(a[4], b[4]) and a[5] == b[5])


def test_state_before_and_after_a_loo_gradient(gp):
    """logLikelihood(), GradLL(), GradLL_exact() and loo() return the same bytes before and after a loo_grad() -- which
    leaves H and W in the two workspaces they read -- and loo_grad() the same bytes before and after them."""
    X, y = synth.drillholes(700)
    gp.set_train(X, y)                       # releases the gradient's workspaces: loo() runs in its own slab first
    set_defaults(gp)
    before = snapshot(gp)
    g1, s1 = gp.loo_grad()
    assert gp.timing()["grad_ms"] > 0 and s1["ms"] > 0
    after = snapshot(gp)
    g2, s2 = gp.loo_grad()
    assert same_snapshot(before, after)
    assert np.array_equal(g1, g2) and same_summary(s1, s2)
    # the other order: loo_grad() directly after each of the calls whose workspaces it overwrites
    for call in (gp.GradLL, gp.GradLL_exact, gp.loo, gp.logLikelihood):
        call()
        g3, s3 = gp.loo_grad()
        assert np.array_equal(g1, g3) and same_summary(s1, s3)
    assert same_snapshot(before, snapshot(gp))
    # after set_train, loo_grad() as the very first call brings gram / factor / alpha up to date
    gp.set_train(X, y)
    set_defaults(gp)
    g4, s4 = gp.loo_grad()
    assert np.array_equal(g1, g4) and same_summary(s1, s4)
    assert same_snapshot(before, snapshot(gp))


def test_statuses(gp):
    X, y = synth.drillholes(300)
    fresh = gpak.Gpak(0)
    try:
        with pytest.raises(gpak.GpakError) as ei:
            fresh.loo_grad()
        assert ei.value.status == gpak.ESTATE
    finally:
        fresh.close()
    gp.set_train(X, y)
    set_defaults(gp)
    want, ws = gp.loo_grad()
    for ng in (9, 11):
        with pytest.raises(gpak.GpakError) as ei:
            gp.loo_grad(ng)
        assert ei.value.status == gpak.EINVAL
    # a White child: the exact gradient's refusal, word for word
    gp.set_kernel([(gpak.KERN_EXPANS, E)], 0.2, 0.1, 0.016, gpak.DIST_DIRECT)
    with pytest.raises(gpak.GpakError) as ei:
        gp.loo_grad()
    assert ei.value.status == gpak.ENOTIMPL and "compositions with a White child are not built" in str(ei.value)
    # not positive definite: NaN everywhere, then recovery at valid parameters
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    g, s = gp.loo_grad()
    assert s["status"] == gpak.ENOTPD and np.all(np.isnan(g))
    assert all(np.isnan(s[k]) for k in ("mse", "mssr", "log_pl"))
    set_defaults(gp)
    g, s = gp.loo_grad()
    assert s["status"] == gpak.OK and np.array_equal(g, want) and same_summary(s, ws)
    # fp64 also in a GPAK_F32 context
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        g, s = f32.loo_grad()
        assert np.array_equal(g, want) and same_summary(s, ws)
    finally:
        f32.close()


def test_multi_gpu_context_refuses_the_loo_gradient():
    X, y = synth.drillholes(256)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X, y)
        m.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
        with pytest.raises(gpak.GpakError) as ei:
            m.loo_grad()
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


def test_long_lived_context_against_fresh_ones_and_the_model():
    """loo_grad_model.SEQUENCE on one long-lived context, in the manner of tests/test_ctx_sequences.py.  Every step that
    returns numbers is compared (a) bit for bit, NaN equal to NaN and statuses equal, with a FRESH context that received
    only set_train, the current kernel call and that one method, and (b) with the stateless model under the bounds of the
    method's own GPU test; the count of factorisations since set_train is LooGradCaching's, the restatement of api.hip's
    validity logic -- in particular a refused call factors nothing."""
    want = lgm.run(lambda: lgm.LooGradModel(lgm.cm.F64, MODEL_CACHE))
    counts = lgm.run(lambda: lgm.LooGradCaching(lgm.cm.F64, MODEL_CACHE))
    recs = lgm.run(lambda: gpak.Gpak(0), lambda: gpak.Gpak(0))
    assert len(recs) == len(want) == len(lgm.SEQUENCE)
    compared, worst = 0, (0.0, None)
    for rec, w, c, (method, kw, due) in zip(recs, want, counts, lgm.SEQUENCE):
        where = f"step {rec['i']} ({method} {kw})"
        if method in cs.SETTERS:
            continue
        if method == "timing":
            assert int(rec["res"][1][0][0]) == int(c["res"][1][0][0]), f"{where}: factorisations since set_train"
            continue
        assert rec["res"][0] == due, (where, rec["res"][0])
        assert cs.same_bits(rec["res"], rec["fresh"]), f"{where}: not bit-equal to a fresh context"
        errs = lgm.errors(w, rec["res"], w["res"], MODEL_CACHE)
        ratio = cs.worst(errs)
        if ratio > worst[0]:
            worst = (ratio, where)
        assert ratio <= 1.0, f"{where}: {ratio:.3g} bounds off the model: {errs}"
        compared += 1
    print(f"\n{compared} compared steps, worst error / bound against the model {worst[0]:.3g} ({worst[1]})")
    assert compared == sum(m not in cs.SETTERS and m != "timing" for m, _, _ in lgm.SEQUENCE)


def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def run_train(tmp_path, tag, Xs, ys, maxit, extra_args=()):
    """`train` in a directory of its own: (trace rows, printed objectives, {file name: bytes} of everything it wrote)."""
    d = tmp_path / tag
    d.mkdir()
    write_csv(d / "train.txt", Xs, ys)
    env = dict(os.environ, GPAK_MAX_ITERS=str(maxit), GPAK_OPT_TRACE=str(d / "trace.txt"))
    env.pop("GPAK_OPT", None)
    cmd = [os.path.join(HOST, "gp_ss_ak"), "-v", "1", "-np", *extra_args, "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS",
           "train.txt", "model"]
    out = subprocess.run(cmd, env=env, cwd=d, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    stats = np.loadtxt(str(d / "model") + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)     # the standardisation was the identity
    rows = [[float(v) for v in line.split()] for line in open(d / "trace.txt")]
    printed = [float(line.split("-logL:")[1]) for line in out.splitlines() if line.startswith("Iteration:")]
    files = {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.name != "train.txt"}
    return rows, printed, files, d


def model_parameters(text):
    body = text.splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    return e, bias, sn2


def cv_log_pl(d):
    out = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "-v", "1", "cv", "-np", "train.txt", "model"], cwd=d, input=b"",
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    return float(out.split("Log pseudo-likelihood:")[1].split()[0])


def test_cli_trains_on_the_loo_objective(gp, tmp_path):
    """N = 512, the prepared set of make_golden_lbfgs, 6 iterations.  The objective column of `--objective loo` falls
    strictly and ends at -log_pl of loo() at the model file's parameters; `cv` of that model prints a log pseudo-likelihood
    above the one it prints for a model trained the default way for as many iterations; and `train` without the option
    writes what it writes with `--objective nlz`, in both --gradient modes."""
    import make_golden_lbfgs
    build()
    N, maxit = 512, 6
    Xs, ys = make_golden_lbfgs.prepared(N)
    rows, printed, files, d_loo = run_train(tmp_path, "loo", Xs, ys, maxit, ("--objective", "loo"))
    obj = [r[1] for r in rows]
    print(f"\n--objective loo: {obj}\n  evaluations {[int(r[2]) for r in rows]}")
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and 2 <= len(rows) <= maxit
    assert all(b < a for a, b in zip(obj, obj[1:]))
    for p, o in zip(printed, obj):
        assert abs(p - o) <= 1e-5 * abs(o)
    model = files["model"].decode()
    assert "KernelName=ExpAns" in model
    e, bias, sn2 = model_parameters(model)
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    final = -gp.loo()[2]["log_pl"]
    set_defaults(gp)
    assert abs(obj[-1] - final) <= 1e-5 * abs(final)

    ref_rows, _, ref_files, d_ref = run_train(tmp_path, "default", Xs, ys, maxit)
    pl_loo, pl_ref = cv_log_pl(d_loo), cv_log_pl(d_ref)
    print(f"  cv: log pseudo-likelihood {pl_loo} after --objective loo, {pl_ref} after the default train")
    assert abs(pl_loo + obj[-1]) <= 1e-4 * abs(obj[-1])               # cv prints six digits
    assert pl_loo > pl_ref

    # the default mode is untouched: without the option, with `--objective nlz`, in both --gradient modes
    for tag, args, want_rows, want_files in (
            ("nlz", ("--objective", "nlz"), ref_rows, ref_files),
            ("nlz-reference", ("--objective", "nlz", "--gradient", "reference"), ref_rows, ref_files)):
        r, _, f, _ = run_train(tmp_path, tag, Xs, ys, maxit, args)
        assert r == want_rows and f == want_files
    ex_rows, _, ex_files, _ = run_train(tmp_path, "exact", Xs, ys, maxit, ("--gradient", "exact"))
    r, _, f, _ = run_train(tmp_path, "nlz-exact", Xs, ys, maxit, ("--objective", "nlz", "--gradient", "exact"))
    assert r == ex_rows and f == ex_files
    assert ex_rows != ref_rows and rows != ex_rows
