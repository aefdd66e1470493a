"""GPU tests (-m gpu) of gpak_cv_groups_grad and of `gp_ss_ak --objective lgo train --groups`.

The reference for the gradient is tests/lgo_grad_ref.py (NumPy: the weight matrix W of the grouped criterion from one
Cholesky factor, contracted with the full dK/dtheta matrices by exact_grad_ref.grad_exact), itself pinned against central
differences of cvg_ref's log_pl in tests/test_cv_groups_grad.py.  The bounds are those of tests/test_loo_grad_gpu.py.
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
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import lgo_grad_model as ggm  # noqa: E402
import lgo_grad_ref as gref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

MODEL_CACHE = {}
E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
DEFAULTS = ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, synth.DEFAULT_SN2)
SUMMARY = ("mse", "mssr", "msmd", "log_pl", "groups", "max_size")


def one_group(n):
    return np.zeros(n, dtype=int)


# (id, N, input columns, grouping, (terms, bias, sn2)): the smallest shapes at which the two new kernels can go wrong
CASES = [
    ("N64-one-group", 64, 3, one_group, DEFAULTS),                       # s = 64, one bin, one row tile
    ("N200-holes", 200, 3, cvg_ref.holes, DEFAULTS),                     # 128 and 72: two bins, rows padded to 256
    ("N513-holes", 513, 3, cvg_ref.holes, DEFAULTS),                     # the last group: one row in its own tile
    ("N513-random37", 513, 3, cvg_ref.random_groups, DEFAULTS),          # columns scattered over all row tiles; bins of several groups
    ("N1000-sizes-1-2-127-128", 1000, 3, cvg_ref.mixed_sizes, DEFAULTS),
    ("N1000-singletons", 1000, 3, cvg_ref.singletons, DEFAULTS),         # 8 bins, the last one 104 wide
    ("N2500-holes-defaults", 2500, 3, cvg_ref.holes, DEFAULTS),          # K > 2048 in the product
    ("N2500-holes-theta2", 2500, 3, cvg_ref.holes, ([(xref.EXPANS, THETA2)], 0.35, 0.05)),
    ("N300-d4-holes", 300, 4, cvg_ref.holes, DEFAULTS),
    ("N512-expans+exp", 512, 3, cvg_ref.random_groups, ([(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.016)),
    ("N512-expans+rbf+bias", 512, 3, cvg_ref.random_groups, ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.016)),
    ("N512-rbf", 512, 3, cvg_ref.holes, ([(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.03)),
]


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(g, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        g.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def data(N, cols=3):
    return synth.drillholes4(N) if cols == 4 else synth.drillholes(N)


def same_summary(a, b):
    return all(a[k] == b[k] for k in SUMMARY)


def gradient_errors(got, want, half_abs):
    """(kernel blocks relative to their largest entry, sn2 entry relative, bias error, bias bound)"""
    nk = len(want) - 2
    ek = np.abs(got[:nk] - want[:nk]).max() / np.abs(want[:nk]).max()
    es = abs(got[nk + 1] - want[nk + 1]) / abs(want[nk + 1])
    return ek, es, abs(got[nk] - want[nk]), 1e-8 * abs(want[nk]) + 1e-15 * half_abs


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_group_gradient_matches_numpy_restatement(gp, case):
    """Per block, as the leave-one-out gradient: the kernel blocks' entries <= 1e-8 of their largest, the sn2 entry <= 1e-8
    of itself, InversewidthR exactly 0 for 3 columns; the bias entry, 1/2 sum W, which cancels heavily, <= 1e-8 |want| +
    1e-15 * 1/2 sum_ij |W_ij| with W from the restatement.  Both units are printed.  Then: a second call returns the same
    bytes; the summary is gpak_cv_groups' on the same context, byte for byte; -log_pl is the restatement's objective;
    logLikelihood() is unchanged; renumbered labels (another column order of H, other bins) agree within the bounds."""
    name, N, cols, grouping, (terms, bias, sn2) = case
    X, y = data(N, cols)
    labels = grouping(N)
    want, W = gref.grad_lgo(X, y, terms, bias, sn2, labels, want_w=True)
    half_abs = 0.5 * float(np.abs(W).sum())
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2)
    try:
        nlz = gp.logLikelihood()
        got, s = gp.cv_groups_grad(labels, len(want))
        assert s["status"] == gpak.OK and gp.logLikelihood() == nlz   # factor, alpha and nlZ stay valid
        ek, es, eb, bb = gradient_errors(got, want, half_abs)
        nk = len(want) - 2
        print(f"\n{name}: kernel block {ek:.3g}, sn2 {es:.3g} (relative); bias entry {want[nk]:.6g}: error {eb / abs(want[nk]):.3g} "
              f"of itself, {eb / half_abs:.3g} of 1/2 sum|W| = {half_abs:.6g}; ms {s['ms']:.3f}\n  got  {got}\n  want {want}")
        assert ek <= 1e-8 and es <= 1e-8
        assert eb <= bb
        if cols == 3 and terms[0][0] == xref.EXPANS:
            assert got[7] == 0.0
        again, s2 = gp.cv_groups_grad(labels, len(want))              # fixed-order reductions: repeatable bit for bit
        assert np.array_equal(again, got) and same_summary(s, s2)
        cs_ = gp.cv_groups(labels)[3]                                 # the summary is gpak_cv_groups'
        assert same_summary(s, cs_) and s["ms"] > 0 and np.array_equal(s["labels"], cs_["labels"])
        objective = gref.objective(X, y, terms, bias, sn2, labels)
        print(f"  -log_pl {-s['log_pl']:.12g}, restatement {objective:.12g}")
        assert abs(-s["log_pl"] - objective) <= 1e-8 * abs(objective)
        other, s3 = gp.cv_groups_grad(int(labels.max()) - labels, len(want))
        ek, es, eb, bb = gradient_errors(other, want, half_abs)
        print(f"  renumbered: kernel block {ek:.3g}, sn2 {es:.3g}, bias {eb / half_abs:.3g} of 1/2 sum|W|; same bytes "
              f"{np.array_equal(other, got)}")
        assert ek <= 1e-8 and es <= 1e-8 and eb <= bb
        assert abs(s3["log_pl"] - s["log_pl"]) <= 1e-8 * abs(s["log_pl"])
        if name == "N1000-singletons":                                 # groups of one sample: gpak_loo_grad
            lg, ls = gp.loo_grad(len(want))
            ek, es, eb, bb = gradient_errors(got, lg, half_abs)
            print(f"  against loo_grad(): kernel block {ek:.3g}, sn2 {es:.3g}, bias {eb / half_abs:.3g} of 1/2 sum|W|")
            assert ek <= 1e-8 and es <= 1e-8 and eb <= bb
            assert abs(ls["log_pl"] - s["log_pl"]) <= 1e-8 * abs(s["log_pl"])
        with pytest.raises(gpak.GpakError) as ei:
            gp.cv_groups_grad(labels, len(want) + 1)
        assert ei.value.status == gpak.EINVAL
    finally:
        set_defaults(gp)


def snapshot(gp, labels):
    mean, var, s = gp.loo()
    lg, ls = gp.loo_grad()
    cm_, cv_, cl, cg = gp.cv_groups(labels)
    return (gp.logLikelihood(), gp.GradLL(), gp.GradLL_exact(), mean, var, {k: s[k] for k in ("mse", "mssr", "log_pl", "passes")},
            lg, {k: ls[k] for k in ("mse", "mssr", "log_pl", "passes")}, cm_, cv_, cl, {k: cg[k] for k in SUMMARY})


def same_snapshot(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_state_before_and_after_a_group_gradient(gp):
    """logLikelihood(), GradLL(), GradLL_exact(), loo(), loo_grad() and cv_groups() return the same bytes before and after a
    cv_groups_grad() -- which leaves H and W in the two workspaces they read -- and cv_groups_grad() the same bytes directly
    after each of them, and as the very first call after set_train."""
    N = 700
    X, y = synth.drillholes(N)
    labels = cvg_ref.random_groups(N)
    gp.set_train(X, y)                       # releases the gradient's workspaces: cv_groups() runs in its own buffer first
    set_defaults(gp)
    before = snapshot(gp, labels)
    g1, s1 = gp.cv_groups_grad(labels)
    assert gp.timing()["grad_ms"] > 0 and s1["ms"] > 0
    after = snapshot(gp, labels)
    g2, s2 = gp.cv_groups_grad(labels)
    assert same_snapshot(before, after)
    assert np.array_equal(g1, g2) and same_summary(s1, s2)
    for call in (gp.GradLL, gp.GradLL_exact, gp.loo, gp.loo_grad, lambda: gp.cv_groups(labels), gp.logLikelihood):
        call()
        g3, s3 = gp.cv_groups_grad(labels)
        assert np.array_equal(g1, g3) and same_summary(s1, s3)
    assert same_snapshot(before, snapshot(gp, labels))
    gp.set_train(X, y)
    set_defaults(gp)
    g4, s4 = gp.cv_groups_grad(labels)
    assert np.array_equal(g1, g4) and same_summary(s1, s4)
    assert same_snapshot(before, snapshot(gp, labels))


def test_statuses(gp):
    N = 300
    X, y = synth.drillholes(N)
    labels = cvg_ref.holes(N, 100)
    fresh = gpak.Gpak(0)
    try:
        fresh.N = N                          # the binding sizes its label check by N; the library has no training set
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_groups_grad(labels)
        assert ei.value.status == gpak.ESTATE
        fresh.set_train(X, y)
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_groups_grad(labels)
        assert ei.value.status == gpak.ESTATE                              # no parameters
    finally:
        fresh.close()
    gp.set_train(X, y)
    set_defaults(gp)
    want, ws = gp.cv_groups_grad(labels)
    for ng in (9, 11):
        with pytest.raises(gpak.GpakError) as ei:
            gp.cv_groups_grad(labels, ng)
        assert ei.value.status == gpak.EINVAL and "gpak_cv_groups_grad" in str(ei.value)
    # the label errors of gpak_cv_groups, under this entry's name: a group of 129; an unused label (through the library)
    with pytest.raises(gpak.GpakError) as ei:
        gp.cv_groups_grad(cvg_ref.holes(N, 129))
    assert ei.value.status == gpak.EINVAL and "gpak_cv_groups_grad: group 0 has more than 128 samples" in str(ei.value)
    import ctypes as C
    group = np.ascontiguousarray(np.where(labels == 1, 3, labels), dtype=np.int32)      # labels 0, 2, 3 of 4: 1 unused
    g = np.zeros(10)
    rc = gp._lib.gpak_cv_groups_grad(gp._h, group.ctypes.data_as(C.POINTER(C.c_int)), 4, g.ctypes.data_as(C.POINTER(C.c_double)),
                                     10, None)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == "gpak_cv_groups_grad: label 1 is not used"
    rc = gp._lib.gpak_cv_groups_grad(gp._h, None, 4, g.ctypes.data_as(C.POINTER(C.c_double)), 10, None)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == "gpak_cv_groups_grad: group is NULL"
    assert gp._lib.gpak_cv_groups_grad(gp._h, group.ctypes.data_as(C.POINTER(C.c_int)), 4, None, 10, None) == gpak.EINVAL
    # a White child: the exact gradient's refusal, word for word
    gp.set_kernel([(gpak.KERN_EXPANS, E)], 0.2, 0.1, 0.016, gpak.DIST_DIRECT)
    with pytest.raises(gpak.GpakError) as ei:
        gp.cv_groups_grad(labels)
    assert ei.value.status == gpak.ENOTIMPL and "compositions with a White child are not built" in str(ei.value)
    # not positive definite: NaN everywhere, then recovery at valid parameters
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    g, s = gp.cv_groups_grad(labels)
    assert s["status"] == gpak.ENOTPD and np.all(np.isnan(g))
    assert all(np.isnan(s[k]) for k in ("mse", "mssr", "msmd", "log_pl"))
    set_defaults(gp)
    g, s = gp.cv_groups_grad(labels)
    assert s["status"] == gpak.OK and np.array_equal(g, want) and same_summary(s, ws)
    # fp64 also in a GPAK_F32 context
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        g, s = f32.cv_groups_grad(labels)
        assert np.array_equal(g, want) and same_summary(s, ws)
    finally:
        f32.close()


def test_multi_gpu_context_refuses_the_group_gradient():
    X, y = synth.drillholes(256)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X, y)
        m.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
        with pytest.raises(gpak.GpakError) as ei:
            m.cv_groups_grad(cvg_ref.holes(256))
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


def test_long_lived_context_against_fresh_ones_and_the_model():
    """lgo_grad_model.SEQUENCE on one long-lived context, in the manner of tests/test_loo_grad_gpu.py.  Every step that
    returns numbers is compared (a) bit for bit, NaN equal to NaN and statuses equal, with a FRESH context that received
    only set_train, the current kernel call and that one method, and (b) with the stateless model under the bounds of the
    method's own GPU test; the count of factorisations since set_train is GroupGradCaching's, the restatement of api.hip's
    validity logic -- in particular a refused call factors nothing."""
    want = ggm.run(lambda: ggm.GroupGradModel(ggm.cm.F64, MODEL_CACHE))
    counts = ggm.run(lambda: ggm.GroupGradCaching(ggm.cm.F64, MODEL_CACHE))
    recs = ggm.run(lambda: gpak.Gpak(0), lambda: gpak.Gpak(0))
    assert len(recs) == len(want) == len(ggm.SEQUENCE)
    compared, worst = 0, (0.0, None)
    for rec, w, c, (method, kw, due) in zip(recs, want, counts, ggm.SEQUENCE):
        where = f"step {rec['i']} ({method} {kw})"
        if method in cs.SETTERS:
            continue
        if method == "timing":
            assert int(rec["res"][1][0][0]) == int(c["res"][1][0][0]), f"{where}: factorisations since set_train"
            continue
        assert rec["res"][0] == due, (where, rec["res"][0])
        assert cs.same_bits(rec["res"], rec["fresh"]), f"{where}: not bit-equal to a fresh context"
        errs = ggm.errors(w, rec["res"], w["res"], MODEL_CACHE)
        ratio = cs.worst(errs)
        if ratio > worst[0]:
            worst = (ratio, where)
        assert ratio <= 1.0, f"{where}: {ratio:.3g} bounds off the model: {errs}"
        compared += 1
    print(f"\n{compared} compared steps, worst error / bound against the model {worst[0]:.3g} ({worst[1]})")
    assert compared == sum(m not in cs.SETTERS and m != "timing" for m, _, _ in ggm.SEQUENCE)


def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def run_train(tmp_path, tag, Xs, ys, maxit, extra_args=(), labels=None):
    """`train` in a directory of its own: (trace rows, printed objectives, {file name: bytes} of everything it wrote)."""
    d = tmp_path / tag
    d.mkdir()
    write_csv(d / "train.txt", Xs, ys)
    inputs, verb_args = {"train.txt"}, []
    if labels is not None:
        with open(d / "groups.txt", "w") as f:
            f.write("# hole\n" + "".join(f"{int(v)}\n" for v in labels))
        inputs.add("groups.txt")
        verb_args = ["--groups", "groups.txt"]
    env = dict(os.environ, GPAK_MAX_ITERS=str(maxit), GPAK_OPT_TRACE=str(d / "trace.txt"))
    env.pop("GPAK_OPT", None)
    cmd = [os.path.join(HOST, "gp_ss_ak"), "-v", "1", "-np", *extra_args, "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS",
           *verb_args, "train.txt", "model"]
    out = subprocess.run(cmd, env=env, cwd=d, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    stats = np.loadtxt(str(d / "model") + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)     # the standardisation was the identity
    rows = [[float(v) for v in line.split()] for line in open(d / "trace.txt")]
    printed = [float(line.split("-logL:")[1]) for line in out.splitlines() if line.startswith("Iteration:")]
    files = {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.name not in inputs}
    return rows, printed, files, d


def model_parameters(text):
    body = text.splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    return e, bias, sn2


def cv_groups_log_density(d, labels):
    with open(d / "groups.txt", "w") as f:
        f.write("".join(f"{int(v)}\n" for v in labels))
    out = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "-v", "1", "cv", "-np", "--groups", "groups.txt", "train.txt", "model"],
                         cwd=d, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    return float(out.split("Log predictive density of the groups:")[1].split()[0])


def test_cli_trains_on_the_group_objective(gp, tmp_path):
    """N = 512, the prepared set of make_golden_lbfgs, holes of 32 samples (labels i // 32), 6 iterations.  The objective
    column of `--objective lgo train --groups` falls strictly and ends at -log_pl of cv_groups() at the model file's
    parameters; `cv --groups` of that model prints the same value, to the six digits it prints, and a log density above the
    one it prints for a model trained the default way for as many iterations.  That last assertion was first checked on the
    CPU alone: exact_grad_ref.projected_lbfgs over lgo_grad_ref (objective and gradient) against lbfgs_ref.lbfgs_optimise
    over the checker's reference sequence, on this data, these labels and 6 iterations each, give log densities 392.07
    against 351.73 -- the restatements satisfy it, so it is kept.  `train` without the option writes what it writes with
    `--objective nlz`, in both --gradient modes, and `--objective loo` still ends at -log_pl of loo()."""
    import make_golden_lbfgs
    build()
    N, maxit = 512, 6
    Xs, ys = make_golden_lbfgs.prepared(N)
    labels = np.arange(N) // 32
    rows, printed, files, d_lgo = run_train(tmp_path, "lgo", Xs, ys, maxit, ("--objective", "lgo"), labels)
    obj = [r[1] for r in rows]
    print(f"\n--objective lgo: {obj}\n  evaluations {[int(r[2]) for r in rows]}")
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and 2 <= len(rows) <= maxit
    assert all(b < a for a, b in zip(obj, obj[1:]))
    for p, o in zip(printed, obj):
        assert abs(p - o) <= 1e-5 * abs(o)
    model = files["model"].decode()
    assert "KernelName=ExpAns" in model
    e, bias, sn2 = model_parameters(model)
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    final = -gp.cv_groups(labels)[3]["log_pl"]
    assert abs(obj[-1] - final) <= 1e-5 * abs(final)

    ref_rows, _, ref_files, d_ref = run_train(tmp_path, "default", Xs, ys, maxit)
    pl_lgo, pl_ref = cv_groups_log_density(d_lgo, labels), cv_groups_log_density(d_ref, labels)
    print(f"  cv --groups: log predictive density {pl_lgo} after --objective lgo, {pl_ref} after the default train")
    assert abs(-pl_lgo - final) <= 5e-6 * abs(final)                   # cv prints six digits: half a unit of the sixth
    assert pl_lgo > pl_ref

    # the default mode is untouched: without the option, with `--objective nlz`, in both --gradient modes
    for tag, args in (("nlz", ("--objective", "nlz")), ("nlz-reference", ("--objective", "nlz", "--gradient", "reference"))):
        r, _, f, _ = run_train(tmp_path, tag, Xs, ys, maxit, args)
        assert r == ref_rows and f == ref_files
    ex_rows, _, ex_files, _ = run_train(tmp_path, "exact", Xs, ys, maxit, ("--gradient", "exact"))
    r, _, f, _ = run_train(tmp_path, "nlz-exact", Xs, ys, maxit, ("--objective", "nlz", "--gradient", "exact"))
    assert r == ex_rows and f == ex_files
    assert ex_rows != ref_rows and rows != ex_rows
    # --objective loo: another trajectory, still its own criterion
    loo_rows, _, loo_files, _ = run_train(tmp_path, "loo", Xs, ys, maxit, ("--objective", "loo"))
    assert loo_rows != rows and loo_rows != ex_rows
    e, bias, sn2 = model_parameters(loo_files["model"].decode())
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    loo_final = -gp.loo()[2]["log_pl"]
    set_defaults(gp)
    assert abs(loo_rows[-1][1] - loo_final) <= 1e-5 * abs(loo_final)
