"""CPU tests (-m "not gpu") of the leave-group-out gradient feature:

1. tests/lgo_grad_ref.py (the NumPy restatement gpak_cv_groups_grad is compared with on the GPU) against central differences
   of -log_pl of tests/cvg_ref.py;
2. the same restatement against a second float64 route to the weight matrix (np.linalg.inv, C_I formed directly);
3. with groups of one sample, against loo_grad_ref's weight matrix; the closed-form factor Q against C;
4. the greedy bins of the column mix: the library's helper against its Python restatement and its stated properties;
5. include/gpak_cv_groups_grad.h against the binding and the library, as tests/test_abi.py holds include/gpak.h;
6. `--objective lgo` and `train --groups` of the command line: what they accept and refuse, before any device is opened;
7. the call sequence of tests/lgo_grad_model.py on the stateless model and on the restatement of api.hip's validity logic.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import lgo_grad_ref as gref  # noqa: E402
import loo_grad_ref as lref  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
PARAMS = {"defaults": (E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2), "theta2": (THETA2, 0.35, 0.05)}
# id -> (N, input columns, labels)
SHAPES = {
    "N64-one-group": (64, 3, lambda N: np.zeros(N, dtype=int)),
    "N200-holes": (200, 3, cvg_ref.holes),
    "N300-d4-holes": (300, 4, cvg_ref.holes),
    "N512-random": (512, 3, cvg_ref.random_groups),
}
CASES = [(shape, name) for shape in SHAPES for name in ("defaults", "theta2")]


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def data(shape):
    N, cols, labels = SHAPES[shape]
    X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
    return X, y, labels(N), cols


_GRAD = {}


def restatement(shape, name):
    """(gradient, W) of the Cholesky route, computed once per case."""
    if (shape, name) not in _GRAD:
        X, y, labels, _ = data(shape)
        e, bias, sn2 = PARAMS[name]
        _GRAD[shape, name] = gref.grad_lgo(X, y, [(xref.EXPANS, e)], bias, sn2, labels, want_w=True)
    return _GRAD[shape, name]


@pytest.mark.parametrize("shape,name", CASES)
def test_restatement_matches_central_differences(shape, name):
    """The entries and steps of tests/test_loo_grad.py: one inverse width (entry 1) and Sigma (entry 6) with h = 1e-5, the
    bias (entry 8) with h = 1e-5, sn2 (entry 9) with h = 1e-6; with four columns InversewidthR (entry 7) as well.  Bound
    1e-7 of |g|inf: the truncation of a central difference is h^2 F''' / 6 and its rounding eps |F| / h ~ 1e-9 on entries
    >= 1."""
    X, y, labels, cols = data(shape)
    e, bias, sn2 = PARAMS[name]
    g, _ = restatement(shape, name)
    x0 = np.array(list(e) + [bias, sn2])

    def F(x):
        return gref.objective(X, y, [(xref.EXPANS, x[:8])], float(x[8]), float(x[9]), labels)

    worst = 0.0
    for k, h in [(1, 1e-5), (6, 1e-5), (8, 1e-5), (9, 1e-6)] + ([(7, 1e-5)] if cols == 4 else []):
        d = np.zeros(10)
        d[k] = h
        fd = (F(x0 + d) - F(x0 - d)) / (2 * h)
        err = abs(g[k] - fd) / np.abs(g).max()
        worst = max(worst, err)
        print(f"\n{shape} {name} entry {k}: restatement {g[k]:.12g}, differences {fd:.12g}, |err| / |g|inf = {err:.3g}")
    assert worst <= 1e-7
    if cols == 3:
        assert g[7] == 0.0


@pytest.mark.parametrize("shape,name", CASES)
def test_restatement_matches_a_second_float64_route(shape, name):
    """np.linalg.inv in place of every factor and C_I = sn2 S^-1 + e e' formed directly, without Q.  Kernel block <= 1e-10
    of its largest entry, the sn2 entry <= 1e-10 of itself.  The bias entry, 1/2 sum W, cancels heavily (see
    tests/test_loo_grad.py): printed in both units, bounded on the device (tests/test_cv_groups_grad_gpu.py)."""
    X, y, labels, _ = data(shape)
    e, bias, sn2 = PARAMS[name]
    g, W = restatement(shape, name)
    g2 = gref.grad_lgo(X, y, [(xref.EXPANS, e)], bias, sn2, labels, route="inv")
    ek = np.abs(g2[:8] - g[:8]).max() / np.abs(g[:8]).max()
    es = abs(g2[9] - g[9]) / abs(g[9])
    eb = abs(g2[8] - g[8])
    print(f"\n{shape} {name}: kernel block {ek:.3g}, sn2 {es:.3g} relative; bias entry {g[8]:.6g}: "
          f"{eb / abs(g[8]):.3g} of itself, {eb / (0.5 * np.abs(W).sum()):.3g} of 1/2 sum|W| = {0.5 * np.abs(W).sum():.6g}")
    assert ek <= 1e-10 and es <= 1e-10


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_singletons_give_the_leave_one_out_weights(name):
    """Groups of one sample: C_i = 2 c_i of loo_grad_ref and W is its W, within 1e-12 of max|W|."""
    N = 200
    X, y = synth.drillholes(N)
    e, bias, sn2 = PARAMS[name]
    K = xref.gram(X, [(xref.EXPANS, e)], bias)
    W = gref.weights(K, y, sn2, cvg_ref.singletons(N))
    Wl = lref.weights(K, y, sn2)
    gap = np.abs(W - Wl).max() / np.abs(Wl).max()
    print(f"\n{name}: |W - W_loo|max / |W_loo|max = {gap:.3g}")
    assert gap <= 1e-12


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_closed_form_q_is_a_factor_of_c(name):
    """Q_I Q_I' against C_I = sn2 S^-1 + e_I e_I' for every group of a mixed labelling, within 1e-12 of max|C_I|."""
    N = 300
    X, y = synth.drillholes(N)
    e, bias, sn2 = PARAMS[name]
    labels = cvg_ref.mixed_sizes(N, (1, 2, 37, 128))
    Ky = xref.gram(X, [(xref.EXPANS, e)], bias) + sn2 * np.eye(N)
    Kinv = np.linalg.inv(Ky)
    alpha = Kinv @ y
    worst = 0.0
    for I in cvg_ref.members(labels):
        Q, C, eI = gref.closed_form_q(sn2 * Kinv[np.ix_(I, I)], alpha[I], sn2)
        direct = np.linalg.inv(Kinv[np.ix_(I, I)])
        direct = direct + np.outer(direct @ alpha[I], direct @ alpha[I])
        worst = max(worst, np.abs(Q @ Q.T - C).max() / np.abs(C).max())
        assert np.abs(C - direct).max() <= 1e-9 * np.abs(direct).max()      # C itself: the definition, by another route
    print(f"\n{name}: worst |Q Q' - C|max / |C|max = {worst:.3g}")
    assert worst <= 1e-12


def library_bins(sizes):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.gpak_cvg_pack_bins.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    n = len(sizes)
    arr = (ctypes.c_int * n)(*[int(s) for s in sizes])
    first = (ctypes.c_int * (n + 1))()
    nb = lib.gpak_cvg_pack_bins(arr, n, first)
    return [first[b] for b in range(nb + 1)]


@pytest.mark.parametrize("labels", [
    cvg_ref.holes(200), cvg_ref.holes(513), cvg_ref.random_groups(513), cvg_ref.mixed_sizes(1000), cvg_ref.singletons(1000),
    cvg_ref.mixed_sizes(2000, (64, 65, 1, 128, 63)), np.zeros(64, dtype=int),
], ids=["holes200", "holes513", "random513", "mixed1000", "singletons1000", "mixed2000", "one-group"])
def test_bins_of_the_column_mix(labels):
    """The library's greedy packing (host code: no device) is the Python restatement, and has the properties the kernel's
    launch relies on: every bin at most 128 columns, groups whole and in order, adjacent bins more than 128 columns
    together -- so at most 2 N / 128 + 1 bins."""
    sizes = [m.size for m in cvg_ref.members(labels)]
    first = library_bins(sizes)
    assert first == gref.pack_bins(sizes)
    assert first[0] == 0 and first[-1] == len(sizes) and all(a < b for a, b in zip(first, first[1:]))
    widths = [sum(sizes[a:b]) for a, b in zip(first, first[1:])]
    assert sum(widths) == len(labels) and max(widths) <= 128 and min(widths) >= 1
    assert all(a + b > 128 for a, b in zip(widths, widths[1:]))
    assert len(widths) <= 2 * len(labels) // 128 + 1
    print(f"\n{len(sizes)} groups in {len(widths)} bins, widths {widths[:6]}{' ...' if len(widths) > 6 else ''}")


def test_header_binding_and_library_list_the_same_symbols():
    declared = header_functions("gpak_cv_groups_grad.h")
    assert declared == sorted(_lib.CV_GROUPS_GRAD_SYMBOLS) == ["gpak_cv_groups_grad"]
    for other in ("gpak.h", "gpak_loo_grad.h", "gpak_cv_groups.h", "gpak_cv_folds.h", "gpak_dev.h", "gpak_dist.h"):
        assert not set(declared) & set(header_functions(other)), other          # declared once
    assert "gpak_cv_groups_grad" not in open(os.path.join(ROOT, "include", "gpak.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    # a NULL context is refused without a device
    lib.gpak_cv_groups_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    g = (ctypes.c_double * 10)()
    assert lib.gpak_cv_groups_grad(None, None, 1, g, 10, None) == gpak.EINVAL


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_cv_groups_grad.h"\n'
                   'int main(void){gpak_cv_groups_summary s; (void)s; '
                   'return gpak_cv_groups_grad(0, 0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("args,msg", [
    (["--objective", "bogus", "train", "x.txt"], "--objective takes nlz or loo"),
    (["--objective", "lgo", "train", "x.txt"], "train --groups FILE"),
    (["train", "--groups", "g.txt", "x.txt"], "goes with --objective lgo"),
    (["--objective", "loo", "train", "--groups", "g.txt", "x.txt"], "goes with --objective lgo"),
    (["--objective", "lgo", "--gradient", "reference", "train", "--groups", "g.txt", "x.txt"], "drop --gradient reference"),
    (["--gradient", "reference", "--objective", "lgo", "train", "--groups", "g.txt", "x.txt"], "drop --gradient reference"),
    (["--objective", "lgo", "--gpus", "2", "train", "--groups", "g.txt", "x.txt"], "one GPU only"),
    (["-g", "2", "--objective", "lgo", "train", "--groups", "g.txt", "x.txt"], "one GPU only"),
    (["--objective", "lgo", "train", "--groups"], "--groups takes a file of labels"),
])
def test_cli_refuses_bad_group_objective_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


@pytest.mark.parametrize("args", [
    ["--objective", "lgo", "train", "--groups", "g.txt"],
    ["--objective", "lgo", "--gradient", "exact", "train", "--groups", "g.txt"],
    ["--gradient", "exact", "--objective", "lgo", "train", "--groups", "g.txt", "-np"],
    ["--objective", "lgo", "--objective", "nlz", "train"],
])
def test_cli_accepts_the_group_objective(args):
    """The option and its combinations pass the parser: `train` without a data file then stops at its own check, before
    any file is read or any device is opened."""
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert "There are not enough input parameters." in r.stderr.decode()


def write_rows(path, rows):
    with open(path, "w") as f:
        f.write("# comment\n")
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")


@pytest.mark.parametrize("labels,msg", [
    (list(range(9)), "holds 9 labels for 10 training samples"),
    ([0] * 9 + ["x"], "is not an integer label"),
])
def test_cli_checks_the_labels_before_a_context_exists(tmp_path, labels, msg):
    """The checks of `cv --groups`, in its words, on the labels of `train --groups`."""
    build()
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(10)])
    write_rows(tmp_path / "g.txt", [(v,) for v in labels])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--objective", "lgo", "train", "-np", "--groups", "g.txt", "train.txt", "model"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and msg in r.stderr.decode()


def test_cli_refuses_a_group_above_the_limit(tmp_path):
    build()
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(130)])
    write_rows(tmp_path / "g.txt", [(7,) for _ in range(130)])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--objective", "lgo", "train", "-np", "--groups", "g.txt", "train.txt", "model"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and "group 7 has more than 128 samples" in r.stderr.decode()


# ---- the call sequence on the models ------------------------------------------------------------------------------------
def test_sequence_on_the_models():
    """tests/lgo_grad_model.py: the stateless model and the restatement of api.hip's validity logic agree step for step,
    every step answers with the status the header promises, and a refused call factors nothing."""
    import ctx_sequences as cs
    import lgo_grad_model as ggm
    cache = {}
    want = ggm.run(lambda: ggm.GroupGradModel(ggm.cm.F64, cache))
    caching = ggm.run(lambda: ggm.GroupGradCaching(ggm.cm.F64, cache))
    asked = 0
    for w, c, (method, kw, due) in zip(want, caching, ggm.SEQUENCE):
        if method == "timing":
            continue
        assert w["res"][0] == due and cs.same_bits(w["res"], c["res"]), (w["i"], method, kw, w["res"][0], c["res"][0])
        asked += method == "cv_groups_grad"
    assert len(want) == len(caching) == len(ggm.SEQUENCE) and asked >= 12
    assert {w["res"][0] for w in want if w["method"] == "cv_groups_grad"} == {ggm.OK, ggm.ENOTPD, ggm.EINVAL, ggm.ESTATE, ggm.ENOTIMPL}
    # a refused call factors nothing; a failed factorisation is tried again at every question
    evals = [int(c["res"][1][0][0]) for c in caching if c["method"] == "timing"]
    assert evals[0] == 1 and evals[2] == evals[1] + 3 and evals[3] == 1, evals
