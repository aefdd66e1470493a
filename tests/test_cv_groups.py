"""CPU tests (-m "not gpu") of the leave-group-out feature:

1. tests/cvg_ref.py (the NumPy restatement gpak_cv_groups is compared with on the GPU) against brute-force refits with the
   group's rows and columns deleted;
2. groups of one sample against tests/loo_ref.py;
3. include/gpak_cv_groups.h against the binding and the library, as tests/test_loo_grad.py holds include/gpak_loo_grad.h;
4. what `gp_ss_ak cv --groups` refuses, before any device is opened;
5. the label mapping of Gpak.cv_groups.
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
import loo_ref  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
BOUND = 1e-8     # the project's bound
# (terms, bias, white, sn2): the defaults and the last three compositions of tests/test_loo_gpu.py
COMPOSITIONS = {
    "defaults": ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "expans+exp": ([(xref.EXPANS, E), (xref.EXP, [0.5, 0.9])], 0.0, 0.0, 0.016),
    "rbf": ([(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03),
    "expans+rbf+bias+white": ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016),
}
GROUPINGS = {"holes": cvg_ref.holes, "random37": cvg_ref.random_groups, "singletons": cvg_ref.singletons,
             "sizes-1-2-127-128": cvg_ref.mixed_sizes}
CASES = [(N, cols, gname, cname) for N, cols in ((200, 3), (513, 3), (1000, 3), (300, 4)) for gname in GROUPINGS
         for cname in COMPOSITIONS]

_FACTORED = {}


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def problem(N, cols, cname):
    """(K with the White child on its diagonal, y, sn2), computed once per (data, composition)."""
    key = (N, cols, cname)
    if key not in _FACTORED:
        X, y = synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
        terms, bias, white, sn2 = COMPOSITIONS[cname]
        _FACTORED[key] = (loo_ref.add_white(xref.gram(X, terms, bias), white), y, sn2)
    return _FACTORED[key]


def sample_of_groups(labels):
    """The groups a refit is made for: all of them up to 12, otherwise the first, the last, the largest, the smallest and
    eight seeded ones.  A refit costs a whole factorisation (a thousand of them for the singletons of N = 1000), and a
    group's numbers depend on no other group's: what a sample cannot show is a fault tied to one particular group, which
    the first / last / largest / smallest are the candidates for."""
    G = int(labels.max()) + 1
    if G <= 12:
        return np.arange(G)
    sizes = np.bincount(labels)
    pick = {0, G - 1, int(sizes.argmax()), int(sizes.argmin())}
    pick |= set(np.random.default_rng(G).choice(G, 8, replace=False).tolist())
    return np.array(sorted(pick))


@pytest.mark.parametrize("N,cols,gname,cname", CASES)
def test_restatement_matches_the_refit(N, cols, gname, cname):
    K, y, sn2 = problem(N, cols, cname)
    labels = GROUPINGS[gname](N)
    mean, var, logp, md = cvg_ref.cv_groups(K, y, sn2, labels)
    pick = sample_of_groups(labels)
    members = np.isin(labels, pick)
    rm, rv, rl, rd = cvg_ref.refit(K, y, sn2, labels, only=pick)
    em = np.abs(mean[members] - rm[members]).max() / np.abs(y).max()
    ev = (np.abs(var[members] - rv[members]) / rv[members]).max()
    el = (np.abs(logp[pick] - rl) / np.abs(rl)).max()
    ed = (np.abs(md[pick] - rd) / np.abs(rd)).max()
    print(f"\nN={N} d={cols} {gname} {cname}: {len(pick)} of {int(labels.max()) + 1} groups refitted; mean {em:.3g} of max|y|, "
          f"variance {ev:.3g}, logp {el:.3g}, Mahalanobis {ed:.3g} relative")
    assert em <= BOUND and ev <= BOUND and el <= BOUND and ed <= BOUND


@pytest.mark.parametrize("N,cols", [(200, 3), (513, 3), (300, 4)])
def test_singletons_are_leave_one_out(N, cols):
    K, y, sn2 = problem(N, cols, "defaults")
    mean, var, logp, md = cvg_ref.cv_groups(K, y, sn2, np.arange(N))
    lm, lv = loo_ref.loo(K, y, sn2)
    want, got = loo_ref.summary(y, lm, lv), cvg_ref.summary(y, mean, var, logp, md)
    em, ev = np.abs(mean - lm).max() / np.abs(y).max(), (np.abs(var - lv) / lv).max()
    es = max(abs(got[k] - want[k]) / abs(want[k]) for k in ("mse", "mssr", "log_pl"))
    print(f"\nN={N} d={cols}: mean {em:.3g}, variance {ev:.3g}, summary {es:.3g}")
    assert em <= 1e-12 and ev <= 1e-12 and es <= 1e-12
    assert abs(got["msmd"] - got["mssr"]) <= 1e-12 * got["mssr"]


# ---- the header -----------------------------------------------------------------------------------------------------
def test_header_binding_and_library_list_the_same_symbols():
    declared = header_functions("gpak_cv_groups.h")
    assert declared == sorted(_lib.CV_GROUPS_SYMBOLS) == ["gpak_cv_groups"]
    assert not set(declared) & set(header_functions())               # declared once
    assert not set(declared) & set(header_functions("gpak_loo_grad.h"))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    txt = open(os.path.join(ROOT, "include", "gpak.h")).read()
    assert txt.rstrip().endswith('#include "gpak_loo_grad.h"\n#include "gpak_cv_groups.h"\n#endif /* GPAK_H */')


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_cv_groups.h"\n'
                   'int main(void){gpak_cv_groups_summary s; (void)s; '
                   'return gpak_cv_groups(0, 0, GPAK_CV_GROUP_MAX, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_summary_structure_matches_the_header():
    """The ctypes structure against the C compiler's layout of gpak_cv_groups_summary."""
    fields = [n for n, _ in _lib.CvGroupsSummary._fields_]
    assert fields == ["mse", "mssr", "msmd", "log_pl", "ms", "groups", "max_size"]
    assert ctypes.sizeof(_lib.CvGroupsSummary) == 5 * 8 + 2 * 4
    assert _lib.CvGroupsSummary.groups.offset == 40 and _lib.CvGroupsSummary.max_size.offset == 44


# ---- the command line -----------------------------------------------------------------------------------------------
def write_train(path, n):
    X, y = synth.drillholes(n)
    with open(path, "w") as f:
        f.write("# x, y, z, grade\n")
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")


@pytest.mark.parametrize("labels,extra,msg", [
    ("\n".join(str(i // 8) for i in range(39)), [], "holds 39 labels for 40 training samples"),
    ("\n".join(str(i // 8) for i in range(41)), [], "holds 41 labels for 40 training samples"),
    ("\n".join(["0"] * 20 + ["1.5"] + ["2"] * 19), [], "'1.5' in"),
    ("\n".join(["0"] * 20 + ["hole7"] + ["2"] * 19), [], "'hole7' in"),
    ("\n".join(str(i // 8) for i in range(40)), ["--gpus", "2"], "one GPU only"),
])
def test_cli_refuses_bad_group_files(tmp_path, labels, extra, msg):
    build()
    write_train(tmp_path / "train.txt", 40)
    (tmp_path / "groups.txt").write_text("# hole of each sample\n" + labels + "\n")
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *extra, "cv", "--groups", str(tmp_path / "groups.txt"),
                        str(tmp_path / "train.txt"), str(tmp_path / "model"), str(tmp_path / "out.txt")],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()
    assert not (tmp_path / "out.txt").exists() and not (tmp_path / "model_lgo.txt").exists()


def test_cli_refuses_a_group_above_128(tmp_path):
    build()
    write_train(tmp_path / "train.txt", 200)
    (tmp_path / "groups.txt").write_text("\n".join(["-3"] * 129 + ["4"] * 71) + "\n")
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "cv", "--groups", str(tmp_path / "groups.txt"), str(tmp_path / "train.txt"),
                        str(tmp_path / "model")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert "group -3 has more than 128 samples" in r.stderr.decode()
    assert not (tmp_path / "model_lgo.txt").exists()


def test_cli_groups_needs_a_file():
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "cv", "--groups"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and "--groups takes a file of labels" in r.stderr.decode()


# ---- the label mapping of the binding -----------------------------------------------------------------------------------
def test_labels_are_numbered_by_sorted_unique_value():
    group, values = gpak.group_labels([7, -2, 7, 100, -2, 0])
    assert group.dtype == np.int32 and group.tolist() == [2, 0, 2, 3, 0, 1] and values.tolist() == [-2, 0, 7, 100]
    group, values = gpak.group_labels(np.array([5, 5, 5], dtype=np.int64), n=3)
    assert group.tolist() == [0, 0, 0] and values.tolist() == [5]
    big = np.array([2 ** 40, -2 ** 40, 0])
    group, values = gpak.group_labels(big)
    assert group.tolist() == [2, 0, 1] and values.tolist() == [-2 ** 40, 0, 2 ** 40]
    labels = cvg_ref.random_groups(513)
    group, values = gpak.group_labels(3 * labels - 11)
    assert np.array_equal(group, labels) and np.array_equal(values, 3 * np.arange(labels.max() + 1) - 11)


@pytest.mark.parametrize("bad", [[0.0, 1.0], [[0, 1], [1, 0]], [], ["a", "b"], [True, False]])
def test_labels_must_be_a_vector_of_integers(bad):
    with pytest.raises(ValueError):
        gpak.group_labels(bad)


def test_labels_must_match_the_sample_count():
    with pytest.raises(ValueError):
        gpak.group_labels([0, 1, 2], n=4)
