"""GPU tests (-m gpu) of gpak_cv_groups and of `gp_ss_ak cv --groups`.

The reference is tests/cvg_ref.py (NumPy, one Cholesky), itself pinned against brute-force refits in
tests/test_cv_groups.py; at N = 8192, where it is out of reach, a group is compared with the device's own joint
prediction of it from the other samples.  Bound throughout: the project's 1e-8, means relative to
max|y|, variances relative per element, log densities and summary values relative.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
BOUND = 1e-8
DEFAULTS = ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2)
SUMMARY = ("mse", "mssr", "msmd", "log_pl")

# (id, N, input columns, grouping, (terms, bias, white, sn2))
CASES = [
    ("N64-one-group", 64, 3, lambda n: np.zeros(n, dtype=int), DEFAULTS),
    ("N200-holes", 200, 3, cvg_ref.holes, DEFAULTS),                    # 128 and 72; padded to 256
    ("N513-holes", 513, 3, cvg_ref.holes, DEFAULTS),                    # the last group: one row in its own tile
    ("N513-random37", 513, 3, cvg_ref.random_groups, DEFAULTS),         # scattered over all row tiles
    ("N1000-sizes-1-2-127-128", 1000, 3, cvg_ref.mixed_sizes, DEFAULTS),
    ("N1000-singletons", 1000, 3, cvg_ref.singletons, DEFAULTS),
    ("N300-d4-holes", 300, 4, cvg_ref.holes, DEFAULTS),
    ("N512-expans+exp", 512, 3, cvg_ref.random_groups, ([(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.0, 0.016)),
    ("N512-rbf", 512, 3, cvg_ref.holes, ([(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03)),
    ("N512-expans+rbf+bias+white", 512, 3, cvg_ref.random_groups,
     ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016)),
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


def same_bytes(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in range(3)) and all(a[3][k] == b[3][k] for k in SUMMARY)
            and a[3]["groups"] == b[3]["groups"] and a[3]["max_size"] == b[3]["max_size"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cv_groups_matches_numpy_restatement(gp, case):
    name, N, cols, grouping, (terms, bias, white, sn2) = case
    X, y = data(N, cols)
    labels = grouping(N)
    want = cvg_ref.cv_groups(loo_ref.add_white(xref.gram(X, terms, bias), white), y, sn2, labels)
    ws = cvg_ref.summary(y, *want)
    gp.set_train(X, y)
    set_composition(gp, terms, bias, sn2, white)
    try:
        mean, var, logp, s = gp.cv_groups(labels)
    finally:
        set_defaults(gp)
    em, ev, el = cvg_ref.errors(y, (mean, var, logp), want)
    es = {k: abs(s[k] - ws[k]) / abs(ws[k]) for k in SUMMARY}
    print(f"\n{name}: mean {em:.3g} of max|y|, variance {ev:.3g} relative, logp {el:.3g} relative, summary "
          + ", ".join(f"{k} {v:.3g}" for k, v in es.items())
          + f"; mse {s['mse']:.6g} mssr {s['mssr']:.6g} msmd {s['msmd']:.6g} log_pl {s['log_pl']:.6g} "
          f"groups {s['groups']} max_size {s['max_size']} ms {s['ms']:.3f}")
    sizes = np.bincount(labels)
    assert s["status"] == gpak.OK and s["groups"] == sizes.size and s["max_size"] == sizes.max() and s["ms"] > 0
    assert np.array_equal(s["labels"], np.arange(sizes.size))
    assert em <= BOUND and ev <= BOUND and el <= BOUND and max(es.values()) <= BOUND


def test_singletons_are_leave_one_out(gp):
    N = 1000
    X, y = data(N)
    gp.set_train(X, y)
    set_defaults(gp)
    lm, lv, ls = gp.loo()
    mean, var, logp, s = gp.cv_groups(np.arange(N))
    em = np.abs(mean - lm).max() / np.abs(y).max()
    ev = (np.abs(var - lv) / lv).max()
    es = max(abs(s[k] - ls[k]) / abs(ls[k]) for k in ("mse", "mssr", "log_pl"))
    r2 = (y - lm) ** 2
    el = (np.abs(logp - (-0.5 * r2 / lv - 0.5 * np.log(lv) - 0.5 * math.log(2 * math.pi)))).max() / np.abs(logp).max()
    print(f"\nsingletons against loo(): mean {em:.3g} of max|y|, variance {ev:.3g} relative, summary {es:.3g}, logp {el:.3g}; "
          f"same bytes: mean {np.array_equal(mean, lm)}, variance {np.array_equal(var, lv)}")
    assert em <= BOUND and ev <= BOUND and es <= BOUND and el <= BOUND
    assert abs(s["msmd"] - s["mssr"]) <= 1e-12 * s["mssr"]      # one sample per group: the two residuals coincide


def test_same_bytes_whatever_holds_G(gp):
    """Two calls; G in the leave-one-out buffer against G in the gradient's workspace; a GPAK_F32 context; and the same
    numbers when the labels are renumbered."""
    N = 1000
    X, y = data(N)
    labels = cvg_ref.mixed_sizes(N)
    gp.set_train(X, y)                 # releases the gradient's workspaces: G goes to the call's own buffer
    set_defaults(gp)
    first = gp.cv_groups(labels)
    assert same_bytes(gp.cv_groups(labels), first)
    gp.GradLL_exact()                  # allocates dG
    assert same_bytes(gp.cv_groups(labels), first)
    f32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        f32.set_train(X, y)
        set_defaults(f32)
        assert same_bytes(f32.cv_groups(labels), first)
    finally:
        f32.close()
    G = int(labels.max()) + 1
    p = np.random.default_rng(5).permutation(G)
    mean, var, logp, s = gp.cv_groups(p[labels])
    assert np.array_equal(mean, first[0]) and np.array_equal(var, first[1]) and np.array_equal(logp[p], first[2])
    assert all(abs(s[k] - first[3][k]) <= 1e-12 * abs(first[3][k]) for k in SUMMARY)   # another order of the groups
    # arbitrary integers: the groups are numbered by sorted unique value
    odd = 7 * labels.astype(np.int64) - 1000
    again = gp.cv_groups(odd)
    assert same_bytes(again, first) and np.array_equal(again[3]["labels"], 7 * np.arange(G) - 1000)


def test_cv_groups_leaves_the_context_state_alone(gp):
    N = 700
    X, y = data(N)
    Xte = synth.test_points(16)
    labels = cvg_ref.holes(N)

    def lsame(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(a[2][k] == b[2][k] for k in ("mse", "mssr", "log_pl"))

    # what the calls return on a context that has never seen cv_groups
    gp.set_train(X, y)
    set_defaults(gp)
    nlz, pm, loo0 = gp.logLikelihood(), gp.posteriorMeanVar(Xte), gp.loo()
    g_ref, g_exact, lg = gp.GradLL(), gp.GradLL_exact(), gp.loo_grad()[0]
    # cv_groups with a buffer of its own (set_train released the gradient's), then everything else
    gp.set_train(X, y)
    set_defaults(gp)
    assert gp.logLikelihood() == nlz
    t0 = gp.timing()
    first = gp.cv_groups(labels)
    t1 = gp.timing()
    assert all(t0[k] == t1[k] for k in t0)                                    # no field of gpak_timing changes
    assert gp.logLikelihood() == nlz and lsame(gp.loo(), loo0)
    assert np.array_equal(gp.GradLL_exact(), g_exact)                         # allocates dG AND dBinv after cv_groups' buffer
    assert np.array_equal(gp.GradLL(), g_ref) and np.array_equal(gp.loo_grad()[0], lg)
    assert all(np.array_equal(a, b) for a, b in zip(gp.posteriorMeanVar(Xte), pm))
    assert same_bytes(gp.cv_groups(labels), first)                            # now in the gradient's workspace
    assert np.array_equal(gp.GradLL(), g_ref) and np.array_equal(gp.GradLL_exact(), g_exact)
    assert lsame(gp.loo(), loo0) and gp.logLikelihood() == nlz
    # cv_groups alone after fresh parameters brings gram / factor / alpha up to date
    set_defaults(gp)
    assert same_bytes(gp.cv_groups(labels), first) and gp.logLikelihood() == nlz


def test_cv_groups_against_joint_prediction_on_the_reduced_set(gp):
    """N = 8192.  Hole 0 (rows 0..127: the longest sums), hole 63 (the last tile) and a scattered group of 128 (every 64th
    row) against set_train without the group + predict_joint at the group's points (noise included); the diagonal and
    the log density are computed here from that covariance."""
    N = 8192
    X, y = data(N)
    gp.set_train(X, y)
    set_defaults(gp)
    hole = cvg_ref.holes(N)
    scattered = np.arange(0, N, 64)
    rest = np.setdiff1d(np.arange(N), scattered)
    lab2 = np.zeros(N, dtype=int)
    lab2[rest] = 1 + np.arange(rest.size) // 128
    run1, run2 = gp.cv_groups(hole), gp.cv_groups(lab2)
    print(f"\nN={N}: holes {run1[3]['ms']:.2f} ms, scattered {run2[3]['ms']:.2f} ms")
    try:
        for what, I, run, g in (("hole 0", np.flatnonzero(hole == 0), run1, 0), ("hole 63", np.flatnonzero(hole == 63), run1, 63),
                                ("every 64th row", scattered, run2, 0)):
            keep = np.ones(N, dtype=bool)
            keep[I] = False
            gp.set_train(X[keep], y[keep])
            set_defaults(gp)
            m, Cv = gp.predict_joint(X[I], 1, want_cov=True)
            Lc = np.linalg.cholesky(Cv)
            z = np.linalg.solve(Lc, y[I] - m)
            lp = -0.5 * float(z @ z) - float(np.sum(np.log(np.diag(Lc)))) - 0.5 * I.size * math.log(2 * math.pi)
            em = np.abs(run[0][I] - m).max() / np.abs(y).max()
            ev = (np.abs(run[1][I] - np.diag(Cv)) / np.diag(Cv)).max()
            el = abs(run[2][g] - lp) / abs(lp)
            print(f"  {what}: mean {em:.3g} of max|y|, variance {ev:.3g} relative, logp {el:.3g} relative ({lp:.6g})")
            assert em <= BOUND and ev <= BOUND and el <= BOUND
    finally:
        set_defaults(gp)


def raw(g, group, n_groups, N):
    """gpak_cv_groups itself, with labels the binding would never pass."""
    mean, var, logp = np.zeros(N), np.zeros(N), np.zeros(max(n_groups, 1))
    s = _lib.CvGroupsSummary()
    ptr = None if group is None else np.ascontiguousarray(group, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = C.POINTER(C.c_double)
    rc = g._lib.gpak_cv_groups(g._h, ptr, int(n_groups), mean.ctypes.data_as(dp), var.ctypes.data_as(dp),
                               logp.ctypes.data_as(dp), C.byref(s))
    return rc, g.last_error()


def test_statuses(gp):
    fresh = gpak.Gpak(0)
    try:
        with pytest.raises(gpak.GpakError) as ei:
            fresh.N = 4
            fresh.cv_groups(np.arange(4))
        assert ei.value.status == gpak.ESTATE
        X4, y4 = data(64)
        fresh.set_train(X4, y4)
        with pytest.raises(gpak.GpakError) as ei:
            fresh.cv_groups(np.zeros(64, dtype=int))
        assert ei.value.status == gpak.ESTATE                              # no parameters
    finally:
        fresh.close()
    N = 512
    X, y = data(N)
    gp.set_train(X, y)
    set_defaults(gp)                                                       # nothing is factored yet
    ev0 = gp.timing()["evaluations"]
    holes = cvg_ref.holes(N)
    big = holes.copy()
    big[128] = 0                                                           # group 0: 129 samples
    for group, n_groups, text in ((None, 4, "NULL"), (holes, 0, "n_groups"), (holes, N + 1, "n_groups"),
                                  (np.where(np.arange(N) == 7, -1, holes), 4, "sample 7"),
                                  (np.where(np.arange(N) == 9, 4, holes), 4, "sample 9"),
                                  (holes, 5, "label 4"), (big, 4, "group 0")):
        rc, msg = raw(gp, group, n_groups, N)
        print(f"\n{text}: status {rc}, '{msg}'")
        assert rc == gpak.EINVAL and text in msg
    assert gp.timing()["evaluations"] == ev0                               # refused before anything is factored
    gp.set_params(np.array(E), synth.DEFAULT_BIAS, -0.5, gpak.DIST_DIRECT)
    mean, var, logp, s = gp.cv_groups(holes)
    assert s["status"] == gpak.ENOTPD
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var)) and np.all(np.isnan(logp)) and all(np.isnan(s[k]) for k in SUMMARY)
    set_defaults(gp)
    good = gp.cv_groups(holes)                                             # recovery at valid parameters
    assert good[3]["status"] == gpak.OK and np.all(np.isfinite(good[0])) and np.all(good[1] > synth.DEFAULT_SN2)
    m = gpak.Gpak(devices=[0, 0])
    try:
        m.set_train(X[:256], y[:256])
        set_defaults(m)
        with pytest.raises(gpak.GpakError) as ei:
            m.cv_groups(cvg_ref.holes(256))
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        m.close()


def write_csv(path, X, y):
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


def test_cli_cv_groups_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then cv --groups with holes of 128 on the same file.  The standardisation of this
    set is the identity, so the file's columns are cv_groups()'s mean and the square root of its variance at the model
    file's six-digit parameters; cv without --groups writes what it wrote before."""
    import make_golden_lbfgs
    build()
    N = 512
    Xs, ys = make_golden_lbfgs.prepared(N)
    write_csv(tmp_path / "train.txt", Xs, ys)
    holes = 10 * cvg_ref.holes(N) - 7                       # any integers: -7, 3, 13, 23
    with open(tmp_path / "holes.txt", "w") as f:
        f.write("# hole of each sample\n" + "\n".join(str(v) for v in holes) + "\n")
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    out = subprocess.run([exe, "-v", "1", "cv", "-np", "--groups", str(tmp_path / "holes.txt"), str(tmp_path / "train.txt"), model],
                         cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    quiet = subprocess.run([exe, "-v", "0", "cv", "--groups", str(tmp_path / "holes.txt"), str(tmp_path / "train.txt"), model,
                            str(tmp_path / "other.txt")], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True).stdout.decode()
    assert open(tmp_path / "other.txt").read() == open(model + "_lgo.txt").read()
    assert open(model + "_lgo.txt").readline() == "# SampleNo, Group, Y, Ylgo, StdYlgo, Inputs\n"
    assert not os.path.exists(model + "_loo.txt")
    rows = np.loadtxt(model + "_lgo.txt", comments="#")
    assert rows.shape == (N, 8) and np.array_equal(rows[:, 0], np.arange(1, N + 1)) and np.array_equal(rows[:, 1], holes)

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    mean, var, logp, s = gp.cv_groups(holes)
    lm, lv, ls = gp.loo()
    set_defaults(gp)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-5 * np.abs(b))

    assert close(rows[:, 2], ys) and close(rows[:, 3], mean) and close(rows[:, 4], np.sqrt(var)) and close(rows[:, 5:], Xs)
    names = ("Mean Square Error of leave-group-out:", "Var MSE Train:", "Mean standardised squared residual:",
             "Mean squared Mahalanobis residual:", "Log predictive density of the groups:", "Groups:", "LGO ms:")
    printed = {k: float(out.split(k)[1].split()[0]) for k in names}
    assert [out.index(k) for k in names] == sorted(out.index(k) for k in names)          # the seven lines, in this order
    file_mse = float(np.mean((rows[:, 2] - rows[:, 3]) ** 2))
    print(f"\ncv --groups: {printed}; mean of the file's squared residuals {file_mse:.6g}; cv_groups() {s}")
    assert abs(printed[names[0]] - file_mse) <= 1e-4 * file_mse          # both from 6-digit columns
    assert abs(printed[names[0]] - s["mse"]) <= 1e-5 * s["mse"]
    assert abs(printed[names[1]] - np.var(ys)) <= 1e-5 * np.var(ys)
    assert abs(printed[names[2]] - s["mssr"]) <= 1e-5 * s["mssr"]
    assert abs(printed[names[3]] - s["msmd"]) <= 1e-5 * s["msmd"]
    assert abs(printed[names[4]] - s["log_pl"]) <= 1e-5 * abs(s["log_pl"])
    assert printed[names[5]] == 4 and printed[names[6]] > 0
    assert [float(v) for v in quiet.split()] == [printed[k] for k in names[:5]]           # -v 0: the bare numbers
    # cv without --groups: the leave-one-out file, as before
    subprocess.run([exe, "-v", "0", "cv", str(tmp_path / "train.txt"), model], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    assert open(model + "_loo.txt").readline() == "# SampleNo, Y, Yloo, VarYloo, Inputs\n"
    loo_rows = np.loadtxt(model + "_loo.txt", comments="#")
    assert loo_rows.shape == (N, 7) and close(loo_rows[:, 2], lm) and close(loo_rows[:, 3], np.sqrt(lv))
