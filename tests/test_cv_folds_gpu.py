"""GPU tests (-m gpu) of gpak_cv_folds, gpak_dev_pack_rows and `gp_ss_ak cv --folds / --kfold`.

The reference is tests/cvg_ref.py::cv_groups (NumPy, one Cholesky, no limit on a group), pinned against brute-force refits
on the same groupings in tests/test_cv_folds.py; at N = 8192, where it is out of reach, a fold is compared with the
device's own joint prediction of it from the other samples.  Bound throughout: the project's 1e-8,
means relative to max|y|, variances relative per element, log densities and summary values relative.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cvf_cases as cc  # noqa: E402
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

BOUND, SUMMARY, E = cc.BOUND, cc.SUMMARY, cc.E


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def set_composition(g, terms, bias, sn2, white=0.0):
    if len(terms) == 1 and terms[0][0] == xref.EXPANS and white == 0.0:
        g.set_params(np.array(terms[0][1], dtype=float), bias, sn2, gpak.DIST_DIRECT)
    else:
        g.set_kernel(terms, bias, white, sn2, gpak.DIST_DIRECT)


def set_defaults(g):
    g.set_params(np.array(E), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def same_bytes(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in range(3)) and all(a[3][k] == b[3][k] for k in SUMMARY)
            and a[3]["groups"] == b[3]["groups"] and a[3]["max_size"] == b[3]["max_size"])


def figures(y, got, want):
    """(mean, variance, logp, worst of the four summary values): the figures every comparison with the restatement bounds"""
    mean, var, logp, s = got
    em, ev, el = cvg_ref.errors(y, (mean, var, logp), want)
    ws = cvg_ref.summary(y, *want)
    return em, ev, el, max(abs(s[k] - ws[k]) / abs(ws[k]) for k in SUMMARY)


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_cv_folds_matches_numpy_restatement(gp, case):
    name, N, cols, grouping, (terms, bias, white, sn2) = case
    X, y = cc.data(N, cols)
    labels = grouping(N)
    want = cvg_ref.cv_groups(loo_ref.add_white(xref.gram(X, terms, bias), white), y, sn2, labels)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    try:
        got = gp.cv_folds(labels)
    finally:
        set_defaults(gp)
    s = got[3]
    em, ev, el, es = figures(y, got, want)
    sizes = np.bincount(labels)
    print(f"\n{name}: sizes {sizes.tolist()}; mean {em:.3g} of max|y|, variance {ev:.3g} relative, logp {el:.3g} relative, "
          f"summary {es:.3g}; mse {s['mse']:.6g} mssr {s['mssr']:.6g} msmd {s['msmd']:.6g} log_pl {s['log_pl']:.6g} ms {s['ms']:.3f}")
    assert s["status"] == gpak.OK and s["groups"] == sizes.size and s["max_size"] == sizes.max() and s["ms"] > 0
    assert np.array_equal(s["labels"], np.arange(sizes.size))
    assert em <= BOUND and ev <= BOUND and el <= BOUND and es <= BOUND


def test_one_group_of_everything_is_the_prior(gp):
    """N = 640, one fold: nothing is left to condition on, so the answer is the prior N(0, K + sn2 I)."""
    N = 640
    X, y = cc.data(N)
    terms, bias, white, sn2 = cc.DEFAULTS
    Ky = xref.gram(X, terms, bias) + sn2 * np.eye(N)
    Lc = np.linalg.cholesky(Ky)
    z = np.linalg.solve(Lc, y)
    lp = -0.5 * float(z @ z) - float(np.sum(np.log(np.diag(Lc)))) - 0.5 * N * math.log(2 * math.pi)
    gp.set_train(X, y)
    set_defaults(gp)
    mean, var, logp, s = gp.cv_folds(np.zeros(N, dtype=int))
    em = np.abs(mean).max() / np.abs(y).max()
    ev = (np.abs(var - np.diag(Ky)) / np.diag(Ky)).max()
    el = abs(logp[0] - lp) / abs(lp)
    print(f"\none group of {N}: |mean| {em:.3g} of max|y|, variance {ev:.3g} relative, logp {el:.3g} relative ({lp:.6g})")
    assert s["status"] == gpak.OK and s["groups"] == 1 and s["max_size"] == N
    assert em <= BOUND and ev <= BOUND and el <= BOUND


def test_both_paths_agree_on_the_same_groups(gp):
    """Groups of 1, 2, 127 and 128 through the batched kernels and one at a time: two fp64 computations with different
    orders of summation, so the bound is the 1e-8 both are held to."""
    N = 1000
    X, y = cc.data(N)
    labels = cvg_ref.mixed_sizes(N)
    gp.set_train(X, y)
    set_defaults(gp)
    a, b = gp.cv_folds(labels), gp.cv_folds(labels, no_batch=True)
    em, ev, el = cvg_ref.errors(y, b[:3], a[:3])
    es = max(abs(a[3][k] - b[3][k]) / abs(a[3][k]) for k in SUMMARY)
    print(f"\nbatched against one at a time: mean {em:.3g} of max|y|, variance {ev:.3g}, logp {el:.3g}, summary {es:.3g} relative; "
          f"ms {a[3]['ms']:.2f} / {b[3]['ms']:.2f}")
    assert a[3]["status"] == b[3]["status"] == gpak.OK
    assert em <= BOUND and ev <= BOUND and el <= BOUND and es <= BOUND


def test_singletons_one_at_a_time_are_leave_one_out(gp):
    N = 300
    X, y = cc.data(N)
    gp.set_train(X, y)
    set_defaults(gp)
    lm, lv, ls = gp.loo()
    mean, var, logp, s = gp.cv_folds(np.arange(N), no_batch=True)
    em = np.abs(mean - lm).max() / np.abs(y).max()
    ev = (np.abs(var - lv) / lv).max()
    es = max(abs(s[k] - ls[k]) / abs(ls[k]) for k in ("mse", "mssr", "log_pl"))
    print(f"\nsingletons one at a time against loo(): mean {em:.3g} of max|y|, variance {ev:.3g} relative, summary {es:.3g}; ms {s['ms']:.2f}")
    assert s["status"] == gpak.OK and s["groups"] == N and s["max_size"] == 1
    assert em <= BOUND and ev <= BOUND and es <= BOUND


def test_small_groups_give_the_bytes_of_cv_groups(gp):
    N = 1000
    X, y = cc.data(N)
    gp.set_train(X, y)
    set_defaults(gp)
    for labels in (cvg_ref.mixed_sizes(N), cvg_ref.random_groups(N), cvg_ref.holes(N)):
        assert same_bytes(gp.cv_folds(labels), gp.cv_groups(labels))


def test_same_bytes_whatever_holds_G_and_whatever_the_other_groups(gp):
    """Two calls; G in the call's own buffer against G in the gradient's workspace; a GPAK_F32 context; renumbered and
    arbitrary labels; and a large group's numbers whether the other samples are one group or holes of 64."""
    N = 1000
    X, y = cc.data(N)
    labels = cc.contiguous(1, 128, 129, 300, 442)(N)
    gp.set_train(X, y)                 # releases the gradient's workspaces: G goes to the call's own buffer
    set_defaults(gp)
    first = gp.cv_folds(labels)
    assert same_bytes(gp.cv_folds(labels), first)
    gp.GradLL_exact()                  # allocates dG
    assert same_bytes(gp.cv_folds(labels), first)
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        assert same_bytes(f32.cv_folds(labels), first)
    finally:
        f32.close()
    G = int(labels.max()) + 1
    p = np.random.default_rng(5).permutation(G)
    mean, var, logp, s = gp.cv_folds(p[labels])
    assert np.array_equal(mean, first[0]) and np.array_equal(var, first[1]) and np.array_equal(logp[p], first[2])
    assert all(abs(s[k] - first[3][k]) <= 1e-12 * abs(first[3][k]) for k in SUMMARY)   # another order of the groups
    odd = 7 * labels.astype(np.int64) - 1000
    again = gp.cv_folds(odd)
    assert same_bytes(again, first) and np.array_equal(again[3]["labels"], 7 * np.arange(G) - 1000)
    # the group of 300 (samples 258 .. 557): alone against ONE other group, and against holes of 64
    I = np.flatnonzero(labels == 3)
    two = np.ones(N, dtype=int)
    two[I] = 0
    holes = 1 + np.arange(N) // 64
    holes[I] = 0
    a, b = gp.cv_folds(two), gp.cv_folds(holes)
    for run in (a, b):
        assert np.array_equal(run[0][I], first[0][I]) and np.array_equal(run[1][I], first[1][I]) and run[2][0] == first[2][3]


def test_cv_folds_leaves_the_context_state_alone(gp):
    N = 700
    X, y = cc.data(N)
    Xte = synth.test_points(16)
    labels = cc.contiguous(256, 257, 187)(N)
    holes = cvg_ref.holes(N)

    def lsame(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(a[2][k] == b[2][k] for k in ("mse", "mssr", "log_pl"))

    # what the calls return on a context that has not run cv_folds on this training set
    gp.set_train(X, y)
    set_defaults(gp)
    nlz, pm, loo0, cvg0 = gp.logLikelihood(), gp.posteriorMeanVar(Xte), gp.loo(), gp.cv_groups(holes)
    g_ref, g_exact, lg = gp.GradLL(), gp.GradLL_exact(), gp.loo_grad()[0]
    gp.set_train(X, y)
    set_defaults(gp)
    assert gp.logLikelihood() == nlz
    t0 = gp.timing()
    first = gp.cv_folds(labels)
    t1 = gp.timing()
    assert all(t0[k] == t1[k] for k in t0)                                    # no field of gpak_timing changes
    assert same_bytes(gp.cv_groups(holes), cvg0)                              # the scratch and dLoo are shared
    assert gp.logLikelihood() == nlz and lsame(gp.loo(), loo0)
    assert np.array_equal(gp.GradLL_exact(), g_exact)
    assert np.array_equal(gp.GradLL(), g_ref) and np.array_equal(gp.loo_grad()[0], lg)
    assert all(np.array_equal(a, b) for a, b in zip(gp.posteriorMeanVar(Xte), pm))
    assert same_bytes(gp.cv_folds(labels), first)                             # now in the gradient's workspace
    assert same_bytes(gp.cv_groups(holes), cvg0)
    assert np.array_equal(gp.GradLL(), g_ref) and np.array_equal(gp.GradLL_exact(), g_exact)
    assert lsame(gp.loo(), loo0) and gp.logLikelihood() == nlz
    # cv_folds alone after fresh parameters brings gram / factor / alpha up to date
    set_defaults(gp)
    assert same_bytes(gp.cv_folds(labels), first) and gp.logLikelihood() == nlz


def test_cv_folds_against_joint_prediction_on_the_reduced_set(gp):
    """N = 8192, 4 random folds.  Fold 0 (2048 scattered samples) against set_train without the fold + predict_joint at
    its points (noise included); the diagonal and the log density are computed here from that covariance."""
    N = 8192
    X, y = cc.data(N)
    gp.set_train(X, y)
    set_defaults(gp)
    labels = cc.random_folds(4)(N)
    mean, var, logp, s = gp.cv_folds(labels)
    split = (C.c_double * 5)()
    assert gp._lib.gpak_cv_folds_last_split(gp._h, split) == gpak.OK
    print(f"\nN={N}, 4 random folds: {s['ms']:.2f} ms (substitution {split[0]:.2f}, batched {split[1]:.2f}, pack {split[2]:.2f}, "
          f"product {split[3]:.2f}, factor + inverse + finish {split[4]:.2f})")
    assert s["status"] == gpak.OK and s["max_size"] == 2048
    try:
        I = np.flatnonzero(labels == 0)
        keep = np.ones(N, dtype=bool)
        keep[I] = False
        gp.set_train(X[keep], y[keep])
        set_defaults(gp)
        m, Cv = gp.predict_joint(X[I], 1, want_cov=True)
        Lc = np.linalg.cholesky(Cv)
        z = np.linalg.solve(Lc, y[I] - m)
        lp = -0.5 * float(z @ z) - float(np.sum(np.log(np.diag(Lc)))) - 0.5 * I.size * math.log(2 * math.pi)
        em = np.abs(mean[I] - m).max() / np.abs(y).max()
        ev = (np.abs(var[I] - np.diag(Cv)) / np.diag(Cv)).max()
        el = abs(logp[0] - lp) / abs(lp)
        print(f"  fold 0: mean {em:.3g} of max|y|, variance {ev:.3g} relative, logp {el:.3g} relative ({lp:.6g})")
        assert em <= BOUND and ev <= BOUND and el <= BOUND
    finally:
        set_defaults(gp)


def raw(g, group, n_groups, N, flags=0, folds=True):
    """gpak_cv_folds (or gpak_cv_groups) itself, with arguments the binding would never pass."""
    mean, var, logp = np.zeros(N), np.zeros(N), np.zeros(max(n_groups, 1))
    s = _lib.CvGroupsSummary()
    ptr = None if group is None else np.ascontiguousarray(group, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = C.POINTER(C.c_double)
    args = [g._h, ptr, int(n_groups), mean.ctypes.data_as(dp), var.ctypes.data_as(dp), logp.ctypes.data_as(dp), C.byref(s)]
    rc = g._lib.gpak_cv_folds(*args, int(flags)) if folds else g._lib.gpak_cv_groups(*args)
    return rc, g.last_error()


def test_statuses(gp):
    fresh = gpak.Gpak(0)
    try:
        with pytest.raises(gpak.GpakError) as ei:
            fresh.N = 4
            fresh.cv_folds(np.arange(4))
        assert ei.value.status == gpak.ESTATE
        X4, y4 = cc.data(64)
        fresh.set_train(X4, y4)
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_folds(np.zeros(64, dtype=int))
        assert ei.value.status == gpak.ESTATE                              # no parameters
    finally:
        fresh.close()
    N = 512
    X, y = cc.data(N)
    gp.set_train(X, y)
    set_defaults(gp)                                                       # nothing is factored yet
    ev0 = gp.timing()["evaluations"]
    holes = cvg_ref.holes(N)
    big = holes.copy()
    big[128] = 0                                                           # group 0: 129 samples
    for group, n_groups, flags, text in ((None, 4, 0, "NULL"), (holes, 0, 0, "n_groups"), (holes, N + 1, 0, "n_groups"),
                                         (np.where(np.arange(N) == 7, -1, holes), 4, 0, "sample 7"),
                                         (np.where(np.arange(N) == 9, 4, holes), 4, 0, "sample 9"),
                                         (holes, 5, 0, "label 4"), (holes, 4, 2, "flags = 2")):
        rc, msg = raw(gp, group, n_groups, N, flags)
        print(f"\n{text}: status {rc}, '{msg}'")
        assert rc == gpak.EINVAL and text in msg and msg.startswith("gpak_cv_folds: ")
    rc, msg = raw(gp, big, 4, N, folds=False)                              # the limit of gpak_cv_groups stands
    assert rc == gpak.EINVAL and "group 0 has more than 128 samples" in msg and msg.startswith("gpak_cv_groups: ")
    assert gp.timing()["evaluations"] == ev0                               # refused before anything is factored
    rc, msg = raw(gp, big, 4, N)
    assert rc == gpak.OK, msg                                              # the same labelling here
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    mean, var, logp, s = gp.cv_folds(big)
    assert s["status"] == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var)) and np.all(np.isnan(logp)) and all(np.isnan(s[k]) for k in SUMMARY)
    set_defaults(gp)
    good = gp.cv_folds(big)                                                # recovery at valid parameters
    assert good[3]["status"] == gpak.OK and np.all(np.isfinite(good[0])) and np.all(good[1] > synth.DEFAULT_SN2)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X[:256], y[:256])
        set_defaults(m)
        with pytest.raises(gpak.GpakError) as ei:
            m.cv_folds(cvg_ref.holes(256))
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


# ---- the pack kernel alone ----------------------------------------------------------------------------------------------
import cvf_pack_worker  # noqa: E402

_PACK = {}


def pack_records():
    """One worker process for all the shapes (torch holds the buffers: its HIP runtime must come up before the library's)."""
    if not _PACK:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cvf_pack_worker.py")], cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        _PACK["rc"], _PACK["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _PACK[rec["name"]] = rec
    return _PACK


@pytest.mark.parametrize("shape", cvf_pack_worker.SHAPES, ids=[s[0] for s in cvf_pack_worker.SHAPES])
def test_pack_rows_alone(shape):
    """gpak_dev_pack_rows on caller-owned buffers against NumPy indexing (tests/cvf_pack_worker.py): a copy, so bit
    equality; the zero rows are +0.0; the guard bands and skew rows of P and all of G keep their bits; with 16-byte and
    with 8-byte stores."""
    recs = pack_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[shape[0]]
    print(f"\n{rec}")
    assert rec["m"] == shape[2] and rec["mp"] % 128 == 0 and rec["G_untouched"]
    for tag in ("vec", "scalar"):
        assert all(rec[tag].values()), (tag, rec[tag])


# ---- the command line -----------------------------------------------------------------------------------------------
def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def test_cli_cv_folds_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then cv --folds with two folds of 256 and cv --kfold 4 --seed 3 on the same file.
    The standardisation of this set is the identity, so the file's columns are cv_folds()'s mean and the square root of its
    variance at the model file's six-digit parameters; cv without options writes what it wrote before."""
    import make_golden_lbfgs
    build()
    N = 512
    Xs, ys = make_golden_lbfgs.prepared(N)
    write_csv(tmp_path / "train.txt", Xs, ys)
    two = 10 * (np.arange(N) % 2) - 7                       # any integers: -7 and 3, 256 samples each, interleaved
    with open(tmp_path / "folds.txt", "w") as f:
        f.write("# fold of each sample\n" + "\n".join(str(v) for v in two) + "\n")
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b))

    names = ("Mean Square Error of k-fold:", "Var MSE Train:", "Mean standardised squared residual:",
             "Mean squared Mahalanobis residual:", "Log predictive density of the groups:", "Folds:", "CV ms:")
    try:
        for option, k in ((["--folds", str(tmp_path / "folds.txt")], 2), (["--kfold", "4", "--seed", "3"], 4)):
            out = subprocess.run([exe, "-v", "1", "cv", "-np", *option, str(tmp_path / "train.txt"), model],
                                 cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
            quiet = subprocess.run([exe, "-v", "0", "cv", *option, str(tmp_path / "train.txt"), model, str(tmp_path / "other.txt")],
                                   cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
            assert open(tmp_path / "other.txt").read() == open(model + "_folds.txt").read()
            assert open(model + "_folds.txt").readline() == "# SampleNo, Fold, Y, Ycv, StdYcv, Inputs\n"
            assert not os.path.exists(model + "_loo.txt") and not os.path.exists(model + "_lgo.txt")
            rows = np.loadtxt(model + "_folds.txt", comments="#")
            assert rows.shape == (N, 8) and np.array_equal(rows[:, 0], np.arange(1, N + 1))
            fold = rows[:, 1].astype(int)
            if k == 2:
                assert np.array_equal(fold, two)
            else:                                            # a valid 4-fold assignment
                sizes = np.bincount(fold, minlength=4)
                assert set(fold.tolist()) == {0, 1, 2, 3} and sizes.max() - sizes.min() <= 1
                assert not np.array_equal(fold, np.arange(N) % 4)
            mean, var, logp, s = gp.cv_folds(fold)
            assert close(rows[:, 2], ys) and close(rows[:, 3], mean) and close(rows[:, 4], np.sqrt(var)) and close(rows[:, 5:], Xs)
            printed = {n: float(out.split(n)[1].split()[0]) for n in names}
            assert [out.index(n) for n in names] == sorted(out.index(n) for n in names)      # the seven lines, in this order
            print(f"\ncv {' '.join(option[:1])}: {printed}; cv_folds() {s}")
            assert abs(printed[names[0]] - s["mse"]) <= 1e-5 * s["mse"]
            assert abs(printed[names[1]] - np.var(ys)) <= 1e-5 * np.var(ys)
            assert abs(printed[names[2]] - s["mssr"]) <= 1e-5 * s["mssr"]
            assert abs(printed[names[3]] - s["msmd"]) <= 1e-5 * s["msmd"]
            assert abs(printed[names[4]] - s["log_pl"]) <= 1e-5 * abs(s["log_pl"])
            assert printed[names[5]] == k and printed[names[6]] > 0
            assert [float(v) for v in quiet.split()] == [printed[n] for n in names[:5]]       # -v 0: the bare numbers
        lm, lv, ls = gp.loo()
    finally:
        set_defaults(gp)
    # cv without options: the leave-one-out file, as before
    subprocess.run([exe, "-v", "0", "cv", str(tmp_path / "train.txt"), model], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert open(model + "_loo.txt").readline() == "# SampleNo, Y, Yloo, VarYloo, Inputs\n"
    loo_rows = np.loadtxt(model + "_loo.txt", comments="#")
    assert loo_rows.shape == (N, 7) and close(loo_rows[:, 2], lm) and close(loo_rows[:, 3], np.sqrt(lv))
