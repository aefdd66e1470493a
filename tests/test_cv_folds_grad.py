"""CPU tests (-m "not gpu") of the k-fold gradient feature:

1. tests/lgo_grad_ref.py (the NumPy restatement gpak_cv_folds_grad is compared with on the GPU) on groups above 128
   samples, against central differences of -log_pl of tests/cvg_ref.py and against its second float64 route;
2. the closed-form factor Q against C for groups of 129, 257 and 442 samples;
3. include/gpak_cv_folds_grad.h and include/gpak_dev_cv_mix.h against the binding and the library;
4. `--objective lgo train --folds / --kfold [--seed]` of the command line: what it accepts and refuses, before any device
   is opened.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvf_cases as cc  # noqa: E402
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import lgo_grad_ref as gref  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

PARAMS = {"defaults": (cc.E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2), "theta2": (cc.THETA2, 0.35, 0.05)}
BY_ID = {c[0]: c for c in cc.CASES}
SHAPES = ("N200-129+71", "N513-2-random-folds", "N700-256+257+187", "N1000-1+128+129+300+442")
CASES = [(shape, name) for shape in SHAPES for name in ("defaults", "theta2")]


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def data(shape):
    _, N, cols, grouping, _ = BY_ID[shape]
    X, y = cc.data(N, cols)
    return X, y, grouping(N), cols


_GRAD = {}


def restatement(shape, name):
    """(gradient, W) of the Cholesky route, computed once per case."""
    if (shape, name) not in _GRAD:
        X, y, labels, _ = data(shape)
        e, bias, sn2 = PARAMS[name]
        _GRAD[shape, name] = gref.grad_lgo(X, y, [(xref.EXPANS, e)], bias, sn2, labels, want_w=True)
    return _GRAD[shape, name]


@pytest.mark.parametrize("shape,name", CASES)
def test_restatement_matches_central_differences_on_large_groups(shape, name):
    """The entries and steps of tests/test_cv_groups_grad.py: one inverse width (entry 1) and Sigma (entry 6) with h = 1e-5,
    the bias (entry 8) with h = 1e-5, sn2 (entry 9) with h = 1e-6.  Bound 1e-7 of |g|inf."""
    X, y, labels, cols = data(shape)
    e, bias, sn2 = PARAMS[name]
    g, _ = restatement(shape, name)
    x0 = np.array(list(e) + [bias, sn2])

    def F(x):
        return gref.objective(X, y, [(xref.EXPANS, x[:8])], float(x[8]), float(x[9]), labels)

    worst = 0.0
    for k, h in [(1, 1e-5), (6, 1e-5), (8, 1e-5), (9, 1e-6)]:
        d = np.zeros(10)
        d[k] = h
        fd = (F(x0 + d) - F(x0 - d)) / (2 * h)
        err = abs(g[k] - fd) / np.abs(g).max()
        worst = max(worst, err)
        print(f"\n{shape} {name} entry {k}: restatement {g[k]:.12g}, differences {fd:.12g}, |err| / |g|inf = {err:.3g}")
    assert worst <= 1e-7
    assert cols == 3 and g[7] == 0.0


@pytest.mark.parametrize("shape,name", CASES)
def test_restatement_matches_a_second_float64_route_on_large_groups(shape, name):
    """np.linalg.inv in place of every factor and C_I formed directly, without Q.  Kernel block <= 1e-10 of its largest
    entry, the sn2 entry <= 1e-10 of itself."""
    X, y, labels, _ = data(shape)
    e, bias, sn2 = PARAMS[name]
    g, W = restatement(shape, name)
    g2 = gref.grad_lgo(X, y, [(xref.EXPANS, e)], bias, sn2, labels, route="inv")
    ek = np.abs(g2[:8] - g[:8]).max() / np.abs(g[:8]).max()
    es = abs(g2[9] - g[9]) / abs(g[9])
    print(f"\n{shape} {name}: kernel block {ek:.3g}, sn2 {es:.3g} relative")
    assert ek <= 1e-10 and es <= 1e-10


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_closed_form_q_is_a_factor_of_c_for_large_groups(name):
    """Q_I Q_I' against C_I = sn2 S^-1 + e_I e_I' for groups of 129, 257 and 442 samples, within 1e-12 of max|C_I|."""
    N = 129 + 257 + 442
    X, y = synth.drillholes(N)
    e, bias, sn2 = PARAMS[name]
    labels = cc.contiguous(129, 257, 442)(N)
    Ky = xref.gram(X, [(xref.EXPANS, e)], bias) + sn2 * np.eye(N)
    Kinv = np.linalg.inv(Ky)
    alpha = Kinv @ y
    sizes, worst = [], 0.0
    for I in cvg_ref.members(labels):
        Q, C, eI = gref.closed_form_q(sn2 * Kinv[np.ix_(I, I)], alpha[I], sn2)
        sizes.append(len(I))
        worst = max(worst, np.abs(Q @ Q.T - C).max() / np.abs(C).max())
    print(f"\n{name}: worst |Q Q' - C|max / |C|max = {worst:.3g}")
    assert sizes == [129, 257, 442] and worst <= 1e-12


def test_headers_binding_and_library_list_the_same_symbols():
    grad, mix = header_functions("gpak_cv_folds_grad.h"), header_functions("gpak_dev_cv_mix.h")
    assert grad == sorted(_lib.CV_FOLDS_GRAD_SYMBOLS) == ["gpak_cv_folds_grad"]
    assert mix == sorted(_lib.DEV_CV_MIX_SYMBOLS) == ["gpak_dev_mix_cols"]
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert "gpak_cv_folds_grad.h" in headers and "gpak_dev_cv_mix.h" in headers
    for name, own in (("gpak_cv_folds_grad", "gpak_cv_folds_grad.h"), ("gpak_dev_mix_cols", "gpak_dev_cv_mix.h")):
        assert [h for h in headers if name in header_functions(h)] == [own]          # declared once
    text = open(os.path.join(ROOT, "include", "gpak.h")).read()
    assert "gpak_cv_folds_grad" not in text and "gpak_dev_cv_mix" not in text and "gpak_dev_mix_cols" not in text
    assert '#include "gpak_cv_folds.h"' in open(os.path.join(ROOT, "include", "gpak_cv_folds_grad.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in grad + mix:
        assert hasattr(lib, name), name
    # a NULL context is refused without a device; so are NULL buffers of the device-pointer call
    lib.gpak_cv_folds_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_int]
    g = (ctypes.c_double * 10)()
    assert lib.gpak_cv_folds_grad(None, None, 1, g, 10, None, 0) == gpak.EINVAL
    lib.gpak_dev_mix_cols.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long]
    assert lib.gpak_dev_mix_cols(None, None, 128, 128, None, 1, None, 1, None, 128) == gpak.EINVAL


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_cv_folds_grad.h"\n#include "gpak_dev_cv_mix.h"\n'
                   'int main(void){gpak_cv_groups_summary s; (void)s; '
                   'if (gpak_dev_mix_cols(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_cv_folds_grad(0, 0, 0, 0, 0, 0, GPAK_CV_FOLDS_NO_BATCH) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("args,msg", [
    (["train", "--folds", "f.txt", "x.txt"], "train --folds goes with --objective lgo"),
    (["train", "--kfold", "4", "x.txt"], "train --kfold goes with --objective lgo"),
    (["--objective", "loo", "train", "--kfold", "4", "x.txt"], "goes with --objective lgo"),
    (["--objective", "lgo", "train", "--folds", "f.txt", "--kfold", "4", "x.txt"], "exclude each other"),
    (["--objective", "lgo", "train", "--groups", "g.txt", "--kfold", "4", "x.txt"], "exclude each other"),
    (["--objective", "lgo", "train", "--groups", "g.txt", "--folds", "f.txt", "x.txt"], "exclude each other"),
    (["--objective", "lgo", "train", "--folds", "f.txt", "--seed", "3", "x.txt"], "--seed goes with --kfold"),
    (["--objective", "lgo", "train", "--groups", "g.txt", "--seed", "3", "x.txt"], "--seed goes with --kfold"),
    (["--objective", "lgo", "train", "--kfold", "x", "x.txt"], "--kfold takes the number of folds"),
    (["--objective", "lgo", "train", "--kfold", "4", "--seed", "-", "x.txt"], "--seed takes a non-negative integer"),
    (["--objective", "lgo", "train", "--folds"], "--folds takes a file of labels"),
    (["--objective", "lgo", "--gradient", "reference", "train", "--kfold", "4", "x.txt"], "drop --gradient reference"),
    (["--objective", "lgo", "--gpus", "2", "train", "--folds", "f.txt", "x.txt"], "one GPU only"),
    (["--objective", "lgo", "train", "x.txt"], "train --groups FILE"),
    (["--objective", "bogus", "train", "x.txt"], "--objective takes nlz or loo"),
])
def test_cli_refuses_bad_fold_objective_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


@pytest.mark.parametrize("args", [
    ["--objective", "lgo", "train", "--folds", "f.txt"],
    ["--objective", "lgo", "train", "--kfold", "10"],
    ["--objective", "lgo", "train", "--kfold", "10", "--seed", "7", "-np"],
    ["--objective", "lgo", "--gradient", "exact", "train", "--seed", "7", "--kfold", "10"],
])
def test_cli_accepts_the_fold_objective(args):
    """The options and their combinations pass the parser: `train` without a data file then stops at its own check, before
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


@pytest.mark.parametrize("verb_args,labels,msg", [
    (["--folds", "f.txt"], list(range(9)), "--folds: f.txt holds 9 labels for 10 training samples"),
    (["--folds", "f.txt"], [0] * 9 + ["x"], "is not an integer label"),
    (["--kfold", "1"], None, "--kfold: 1 folds for 10 training samples (2 <= K <= N is needed)"),
    (["--kfold", "11"], None, "--kfold: 11 folds for 10 training samples (2 <= K <= N is needed)"),
])
def test_cli_checks_the_folds_before_a_context_exists(tmp_path, verb_args, labels, msg):
    """The checks of `cv --folds` / `cv --kfold`, in their words, on the labels of `train`."""
    build()
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(10)])
    if labels is not None:
        write_rows(tmp_path / "f.txt", [(v,) for v in labels])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--objective", "lgo", "train", "-np", *verb_args, "train.txt", "model"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and msg in r.stderr.decode()


def test_cli_still_refuses_a_group_above_the_limit_through_groups(tmp_path):
    build()
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(130)])
    write_rows(tmp_path / "g.txt", [(7,) for _ in range(130)])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--objective", "lgo", "train", "-np", "--groups", "g.txt", "train.txt", "model"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and "group 7 has more than 128 samples" in r.stderr.decode()
