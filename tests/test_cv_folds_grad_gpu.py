"""GPU tests (-m gpu) of gpak_cv_folds_grad, of gpak_dev_mix_cols alone and of `gp_ss_ak --objective lgo train --folds /
--kfold`.

The reference for the gradient is tests/lgo_grad_ref.py, which has no limit on a group's size and is pinned against
central differences on groups above 128 samples in tests/test_cv_folds_grad.py.  The bounds are those of
tests/test_cv_groups_grad_gpu.py.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cvf_cases as cc  # noqa: E402
import cvf_mix_worker  # noqa: E402
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import lgo_grad_ref as gref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

E = cc.E
SUMMARY = ("mse", "mssr", "msmd", "log_pl", "groups", "max_size")
BY_ID = {c[0]: c for c in cc.CASES}
# one over a tile, exactly two tiles, scattered members, a larger group before a smaller one in the reused workspaces, both
# paths in one call, K > 1024 in the mix; the composition with a White child is refused and has its own test
CASES = [BY_ID[k] for k in ("N200-129+71", "N513-2-random-folds", "N700-256+257+187", "N1000-5-random-folds",
                            "N1000-1+128+129+300+442", "N1000-442+300+129+128+1", "N1100-i-mod-3", "N2000-1300+700",
                            "N300-d4-129+171", "N700-rbf")]
CASES.append(("N513-2-folds-expans+rbf+bias", 513, 3, cc.random_folds(2),
              ([(xref.EXPANS, cc.THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.0, 0.016)))


def set_composition(g, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        g.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def same_summary(a, b):
    return all(a[k] == b[k] for k in SUMMARY)


def gradient_errors(got, want, half_abs):
    """(kernel blocks relative to their largest entry, sn2 entry relative, bias error, bias bound)"""
    nk = len(want) - 2
    ek = np.abs(got[:nk] - want[:nk]).max() / np.abs(want[:nk]).max()
    es = abs(got[nk + 1] - want[nk + 1]) / abs(want[nk + 1])
    return ek, es, abs(got[nk] - want[nk]), 1e-8 * abs(want[nk]) + 1e-15 * half_abs


def worst_ratio(ek, es, eb, bb):
    return max(ek / 1e-8, es / 1e-8, eb / bb)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fold_gradient_matches_numpy_restatement(gp, case):
    """Per block, the bounds of the leave-group-out gradient: the kernel blocks' entries <= 1e-8 of their largest, the sn2
    entry <= 1e-8 of itself, InversewidthR exactly 0 for 3 columns, the bias entry <= 1e-8 |want| + 1e-15 * 1/2 sum |W|.
    The worst error / bound is printed.  Then: a second call returns the same bytes; the summary is gpak_cv_folds' on the
    same context, field by field; -log_pl is the restatement's objective; logLikelihood() is unchanged; renumbered labels
    and no_batch=True (every group down the one-at-a-time path and through the wide mix) stay within the bounds."""
    name, N, cols, grouping, (terms, bias, white, sn2) = case
    assert white == 0.0
    X, y = cc.data(N, cols)
    labels = grouping(N)
    want, W = gref.grad_lgo(X, y, terms, bias, sn2, labels, want_w=True)
    half_abs = 0.5 * float(np.abs(W).sum())
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2)
    try:
        nlz = gp.logLikelihood()
        got, s = gp.cv_folds_grad(labels, len(want))
        assert s["status"] == gpak.OK and gp.logLikelihood() == nlz   # factor, alpha and nlZ stay valid
        errs = gradient_errors(got, want, half_abs)
        ek, es, eb, bb = errs
        nk = len(want) - 2
        print(f"\n{name}: worst error / bound {worst_ratio(*errs):.3g}: kernel block {ek:.3g}, sn2 {es:.3g} (relative); bias entry "
              f"{want[nk]:.6g}: error {eb / half_abs:.3g} of 1/2 sum|W| = {half_abs:.6g}; ms {s['ms']:.3f}\n  got  {got}\n  want {want}")
        assert ek <= 1e-8 and es <= 1e-8
        assert eb <= bb
        if cols == 3 and terms[0][0] == xref.EXPANS:
            assert got[7] == 0.0
        again, s2 = gp.cv_folds_grad(labels, len(want))               # fixed-order reductions: repeatable bit for bit
        assert np.array_equal(again, got) and same_summary(s, s2)
        cf = gp.cv_folds(labels)[3]                                   # the summary is gpak_cv_folds'
        assert same_summary(s, cf) and s["ms"] > 0 and np.array_equal(s["labels"], cf["labels"])
        objective = gref.objective(X, y, terms, bias, sn2, labels)
        print(f"  -log_pl {-s['log_pl']:.12g}, restatement {objective:.12g}")
        assert abs(-s["log_pl"] - objective) <= 1e-8 * abs(objective)
        other, s3 = gp.cv_folds_grad(int(labels.max()) - labels, len(want))
        errs = gradient_errors(other, want, half_abs)
        print(f"  renumbered: worst error / bound {worst_ratio(*errs):.3g}")
        assert errs[0] <= 1e-8 and errs[1] <= 1e-8 and errs[2] <= errs[3]
        assert abs(s3["log_pl"] - s["log_pl"]) <= 1e-8 * abs(s["log_pl"])
        nb, s4 = gp.cv_folds_grad(labels, len(want), no_batch=True)
        errs = gradient_errors(nb, want, half_abs)
        print(f"  no_batch: worst error / bound {worst_ratio(*errs):.3g}")
        assert errs[0] <= 1e-8 and errs[1] <= 1e-8 and errs[2] <= errs[3]
        assert same_summary(s4, gp.cv_folds(labels, no_batch=True)[3])
    finally:
        set_defaults(gp)


@pytest.mark.parametrize("grouping", [cvg_ref.holes, cvg_ref.random_groups], ids=["holes", "random37"])
def test_all_small_labellings_give_the_bytes_of_the_group_gradient(gp, grouping):
    N = 513
    X, y = synth.drillholes(N)
    labels = grouping(N)
    gp.set_train(X, y)
    set_defaults(gp)
    a, sa = gp.cv_groups_grad(labels)
    b, sb = gp.cv_folds_grad(labels)
    assert np.array_equal(a, b) and same_summary(sa, sb) and not np.any(np.isnan(a))


LABELS_700 = cc.contiguous(300, 129, 271)


def snapshot(gp, labels, small):
    mean, var, s = gp.loo()
    lg, ls = gp.loo_grad()
    cm_, cv_, cl, cg = gp.cv_groups(small)
    gg, gs = gp.cv_groups_grad(small)
    fm, fv, fl, fs = gp.cv_folds(labels)
    return (gp.logLikelihood(), gp.GradLL(), gp.GradLL_exact(), mean, var, {k: s[k] for k in ("mse", "mssr", "log_pl", "passes")},
            lg, {k: ls[k] for k in ("mse", "mssr", "log_pl", "passes")}, cm_, cv_, cl, {k: cg[k] for k in SUMMARY},
            gg, {k: gs[k] for k in SUMMARY}, fm, fv, fl, {k: fs[k] for k in SUMMARY})


def same_snapshot(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_state_before_and_after_a_fold_gradient(gp):
    """logLikelihood(), GradLL(), GradLL_exact(), loo(), loo_grad(), cv_groups(), cv_groups_grad() and cv_folds() return the
    same bytes before and after a cv_folds_grad() -- which leaves H and W in the two workspaces they read and its mix's
    result where cv_folds() packs -- and cv_folds_grad() the same bytes directly after each of them, and as the very first
    call after set_train."""
    N = 700
    X, y = synth.drillholes(N)
    labels, small = LABELS_700(N), cvg_ref.random_groups(N)
    gp.set_train(X, y)
    set_defaults(gp)
    before = snapshot(gp, labels, small)
    g1, s1 = gp.cv_folds_grad(labels)
    assert gp.timing()["grad_ms"] > 0 and s1["ms"] > 0
    after = snapshot(gp, labels, small)
    g2, s2 = gp.cv_folds_grad(labels)
    assert same_snapshot(before, after)
    assert np.array_equal(g1, g2) and same_summary(s1, s2)
    for call in (gp.logLikelihood, gp.GradLL, gp.GradLL_exact, gp.loo, gp.loo_grad, lambda: gp.cv_groups(small),
                 lambda: gp.cv_groups_grad(small), lambda: gp.cv_folds(labels)):
        call()
        g3, s3 = gp.cv_folds_grad(labels)
        assert np.array_equal(g1, g3) and same_summary(s1, s3)
    assert same_snapshot(before, snapshot(gp, labels, small))
    gp.set_train(X, y)
    set_defaults(gp)
    g4, s4 = gp.cv_folds_grad(labels)
    assert np.array_equal(g1, g4) and same_summary(s1, s4)
    assert same_snapshot(before, snapshot(gp, labels, small))


def test_statuses(gp):
    N = 300
    X, y = synth.drillholes(N)
    labels = cc.contiguous(129, 171)(N)
    fresh = gpak.Gpak(0)
    try:
        fresh.N = N                          # the binding sizes its label check by N; the library has no training set
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_folds_grad(labels)
        assert ei.value.status == gpak.ESTATE and "gpak_cv_folds_grad" in str(ei.value)
        fresh.set_train(X, y)
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_folds_grad(labels)
        assert ei.value.status == gpak.ESTATE and "gpak_cv_folds_grad" in str(ei.value)   # no parameters
    finally:
        fresh.close()
    gp.set_train(X, y)
    set_defaults(gp)
    want, ws = gp.cv_folds_grad(labels)
    for ng in (9, 11):
        with pytest.raises(gpak.GpakError) as ei:
            gp.cv_folds_grad(labels, ng)
        assert ei.value.status == gpak.EINVAL and "gpak_cv_folds_grad" in str(ei.value)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    g = np.zeros(10)
    group = np.ascontiguousarray(labels, dtype=np.int32)
    rc = gp._lib.gpak_cv_folds_grad(gp._h, group.ctypes.data_as(ip), 2, g.ctypes.data_as(dp), 10, None, 2)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == \
        "gpak_cv_folds_grad: flags = 2 has bits other than GPAK_CV_FOLDS_NO_BATCH"
    unused = np.ascontiguousarray(np.where(labels == 1, 3, labels), dtype=np.int32)      # labels 0 and 3 of 4
    rc = gp._lib.gpak_cv_folds_grad(gp._h, unused.ctypes.data_as(ip), 4, g.ctypes.data_as(dp), 10, None, 0)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == "gpak_cv_folds_grad: label 1 is not used"
    rc = gp._lib.gpak_cv_folds_grad(gp._h, None, 2, g.ctypes.data_as(dp), 10, None, 0)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == "gpak_cv_folds_grad: group is NULL"
    rc = gp._lib.gpak_cv_folds_grad(gp._h, group.ctypes.data_as(ip), 2, None, 10, None, 0)
    assert rc == gpak.EINVAL and gp._lib.gpak_last_error(gp._h).decode() == "gpak_cv_folds_grad: g is NULL"
    # a White child: the exact gradient's refusal, word for word
    gp.set_kernel([(gpak.KERN_EXPANS, E)], 0.2, 0.1, 0.016, gpak.DIST_DIRECT)
    with pytest.raises(gpak.GpakError) as ei:
        gp.cv_folds_grad(labels)
    assert ei.value.status == gpak.ENOTIMPL and "compositions with a White child are not built" in str(ei.value)
    assert "gpak_cv_folds_grad" in str(ei.value)
    # not positive definite: NaN everywhere, then recovery at valid parameters
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    g, s = gp.cv_folds_grad(labels)
    assert s["status"] == gpak.ENOTPD and np.all(np.isnan(g))
    assert all(np.isnan(s[k]) for k in ("mse", "mssr", "msmd", "log_pl"))
    set_defaults(gp)
    g, s = gp.cv_folds_grad(labels)
    assert s["status"] == gpak.OK and np.array_equal(g, want) and same_summary(s, ws)
    # fp64 also in a GPAK_F32 context
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        g, s = f32.cv_folds_grad(labels)
        assert np.array_equal(g, want) and same_summary(s, ws)
    finally:
        f32.close()


def test_multi_gpu_context_refuses_the_fold_gradient():
    X, y = synth.drillholes(256)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X, y)
        m.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
        with pytest.raises(gpak.GpakError) as ei:
            m.cv_folds_grad(cc.contiguous(129, 127)(256))
        assert ei.value.status == gpak.ENOTIMPL and "gpak_cv_folds_grad" in str(ei.value)
    finally:
        m.close()


# ---- the mix kernel alone ---------------------------------------------------------------------------------------------
_MIX = {}


def mix_records():
    """One worker process for all the shapes (torch holds the buffers: its HIP runtime must come up before the library's)."""
    if not _MIX:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cvf_mix_worker.py")], cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        _MIX["rc"], _MIX["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _MIX[rec["name"]] = rec
    return _MIX


@pytest.mark.parametrize("shape", cvf_mix_worker.SHAPES, ids=[s[0] for s in cvf_mix_worker.SHAPES])
def test_mix_cols_alone(shape):
    """gpak_dev_mix_cols on caller-owned buffers (tests/cvf_mix_worker.py): the mixed columns within (m + 2) u |H| |Q| of the
    long-double product; every other column of H, all of Q and cols, every guard band and skew row bit-identical; the same
    bytes from a second call; the refusals; with even and with odd ldq / ldz.  And the check bites: against a reference
    with two columns swapped the same ratio is beyond 1e6."""
    recs = mix_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[shape[0]]
    print(f"\n{rec}")
    assert rec["m"] == shape[1] and rec["mp"] % 128 == 0
    if shape[0] == "m=300-scattered":
        assert rec["tiles_hit"] == cvf_mix_worker.NP // 128
    for tag in ("even", "odd"):
        r = rec[tag]
        assert r["ldq"] % 2 == (tag == "odd") and r["ldz"] % 2 == (tag == "odd")
        assert r["ratio"] <= 1.0, (tag, r)
        for k in ("rc", "other_columns_and_skew_rows", "H_guards", "Q_untouched", "Z_guards", "Z_skew_rows", "cols_untouched",
                  "repeatable"):
            assert r[k] is True, (tag, k, r)
    if shape[1] >= 2:
        assert rec["bites"] > 1e6


# ---- the command line -----------------------------------------------------------------------------------------------
def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def run_train(tmp_path, tag, Xs, ys, maxit, extra_args=(), verb_args=(), labels=None):
    """`train` in a directory of its own: (trace rows, printed objectives, {file name: bytes} of everything it wrote)."""
    d = tmp_path / tag
    d.mkdir()
    write_csv(d / "train.txt", Xs, ys)
    inputs = {"train.txt"}
    if labels is not None:
        with open(d / "folds.txt", "w") as f:
            f.write("# fold\n" + "".join(f"{int(v)}\n" for v in labels))
        inputs.add("folds.txt")
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


def cv_log_density(d, *verb_args):
    out = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "-v", "1", "cv", "-np", *verb_args, "train.txt", "model"],
                         cwd=d, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    return float(out.split("Log predictive density of the groups:")[1].split()[0])


def test_cli_trains_on_the_fold_objective(gp, tmp_path):
    """N = 512, the prepared set of make_golden_lbfgs, three folds i % 3 (171 / 171 / 170 samples: every one above the
    batched kernels' 128) through --folds, 6 iterations.  The objective column falls strictly and ends at -log_pl of
    cv_folds() at the model file's parameters; `cv --folds` of that model prints the same value, to the six digits it
    prints, and a log density above the one it prints for a model trained the default way for as many iterations.  That
    last assertion is kept because the restatements satisfy it: projected_lbfgs over lgo_grad_ref against lbfgs_ref over
    the checker's reference sequence, 6 iterations each, give 395.91 against 366.93 on these labels.  One --kfold 4 --seed 1
    run ends at -log_pl of `cv --kfold 4 --seed 1` on its own model.  `train` without the options, with --objective nlz,
    --objective loo and --objective lgo --groups, is deterministic and follows another trajectory."""
    import make_golden_lbfgs
    subprocess.check_call(["make", "-s", "-C", HOST])
    N, maxit = 512, 6
    Xs, ys = make_golden_lbfgs.prepared(N)
    labels = np.arange(N) % 3
    lgo = ("--objective", "lgo")
    rows, printed, files, d_f = run_train(tmp_path, "folds", Xs, ys, maxit, lgo, ("--folds", "folds.txt"), labels)
    obj = [r[1] for r in rows]
    print(f"\n--objective lgo train --folds: {obj}\n  evaluations {[int(r[2]) for r in rows]}")
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and 2 <= len(rows) <= maxit
    assert all(b < a for a, b in zip(obj, obj[1:]))
    for p, o in zip(printed, obj):
        assert abs(p - o) <= 1e-5 * abs(o)
    model = files["model"].decode()
    assert "KernelName=ExpAns" in model
    e, bias, sn2 = model_parameters(model)
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    final = -gp.cv_folds(labels)[3]["log_pl"]
    set_defaults(gp)
    assert abs(obj[-1] - final) <= 1e-5 * abs(final)

    ref_rows, _, ref_files, d_ref = run_train(tmp_path, "default", Xs, ys, maxit, (), (), labels)
    pl_f, pl_ref = cv_log_density(d_f, "--folds", "folds.txt"), cv_log_density(d_ref, "--folds", "folds.txt")
    print(f"  cv --folds: log predictive density {pl_f} after train --folds, {pl_ref} after the default train")
    assert abs(-pl_f - final) <= 5e-6 * abs(final)                     # cv prints six digits: half a unit of the sixth
    assert pl_f > pl_ref

    krows, _, kfiles, d_k = run_train(tmp_path, "kfold", Xs, ys, maxit, lgo, ("--kfold", "4", "--seed", "1"))
    pl_k = cv_log_density(d_k, "--kfold", "4", "--seed", "1")
    print(f"  --kfold 4 --seed 1: {[r[1] for r in krows]}; cv --kfold 4 --seed 1 prints {pl_k}")
    assert abs(-pl_k - krows[-1][1]) <= 1e-5 * abs(pl_k)
    assert krows != rows

    # the other modes: untouched by the options' presence in the parser
    r, _, f, _ = run_train(tmp_path, "nlz", Xs, ys, maxit, ("--objective", "nlz"))
    assert r == ref_rows and f == {k: v for k, v in ref_files.items()}
    loo_rows, _, _, _ = run_train(tmp_path, "loo", Xs, ys, maxit, ("--objective", "loo"))
    holes = np.arange(N) // 32
    g_rows, _, g_files, d_g = run_train(tmp_path, "groups", Xs, ys, maxit, lgo, ("--groups", "folds.txt"), holes)
    assert loo_rows != rows and g_rows != rows and loo_rows != ref_rows
    e, bias, sn2 = model_parameters(g_files["model"].decode())
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    g_final = -gp.cv_groups(holes)[3]["log_pl"]
    set_defaults(gp)
    assert abs(g_rows[-1][1] - g_final) <= 1e-5 * abs(g_final)
