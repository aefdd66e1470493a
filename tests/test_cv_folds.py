"""CPU tests (-m "not gpu") of the k-fold feature:

1. tests/cvg_ref.py (the NumPy restatement gpak_cv_folds is compared with on the GPU; it has no limit on a group) against
   brute-force refits on the groupings of tests/cvf_cases.py;
2. include/gpak_cv_folds.h and include/gpak_dev_cv.h against the binding, the library and a C99 compiler;
3. what `gp_ss_ak cv --folds / --kfold` refuses, before any device is opened, and that `cv --groups` still refuses a group
   of 129;
4. the fold assignment of --kfold (gp_ss_ak_amd/host/kfold_assign.hpp, compiled alone) is a function of its seed.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvf_cases as cc  # noqa: E402
import cvg_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402
from test_abi import header_functions  # noqa: E402
from test_cv_groups import write_train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
EXE = os.path.join(HOST, "gp_ss_ak")


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_restatement_matches_the_refit(case):
    name, N, cols, grouping, (terms, bias, white, sn2) = case
    X, y = cc.data(N, cols)
    K = loo_ref.add_white(xref.gram(X, terms, bias), white)
    labels = grouping(N)
    mean, var, logp, md = cvg_ref.cv_groups(K, y, sn2, labels)
    rm, rv, rl, rd = cvg_ref.refit(K, y, sn2, labels)
    em = np.abs(mean - rm).max() / np.abs(y).max()
    ev = (np.abs(var - rv) / rv).max()
    el = (np.abs(logp - rl) / np.abs(rl)).max()
    ed = (np.abs(md - rd) / np.abs(rd)).max()
    print(f"\n{name}: sizes {np.bincount(labels).tolist()}; mean {em:.3g} of max|y|, variance {ev:.3g}, logp {el:.3g} "
          f"(smallest |logp| {np.abs(rl).min():.3g}), Mahalanobis {ed:.3g} relative")
    assert em <= cc.BOUND and ev <= cc.BOUND and el <= cc.BOUND and ed <= cc.BOUND


# ---- the headers ----------------------------------------------------------------------------------------------------
def test_header_binding_and_library_list_the_same_symbols():
    declared = header_functions("gpak_cv_folds.h")
    assert declared == sorted(_lib.CV_FOLDS_SYMBOLS) == ["gpak_cv_folds"]
    others = set(header_functions()) | set(header_functions("gpak_loo_grad.h")) | set(header_functions("gpak_cv_groups.h")) \
        | set(header_functions("gpak_dev.h")) | set(header_functions("gpak_dev_f32.h")) | set(header_functions("gpak_dist.h"))
    assert not set(declared) & others                                # declared once
    assert header_functions("gpak_dev_cv.h") == ["gpak_dev_pack_rows"] and "gpak_dev_pack_rows" not in others
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared + ["gpak_dev_pack_rows", "gpak_cv_folds_last_split"]:
        assert hasattr(lib, name), name
    assert "gpak_cv_folds" not in open(os.path.join(ROOT, "include", "gpak.h")).read()   # gpak.h does not include it
    assert gpak.NO_BATCH == 1 and hasattr(gpak.Gpak, "cv_folds")


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_cv_folds.h"\n#include "gpak_dev_cv.h"\n'
                   'int main(void){gpak_cv_groups_summary s; (void)s; (void)gpak_dev_pack_rows;\n'
                   'return gpak_cv_folds(0, 0, 1, 0, 0, 0, 0, GPAK_CV_FOLDS_NO_BATCH) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_a_null_context_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.gpak_cv_folds(None, None, 1, None, None, None, None, 0) == gpak.EINVAL
    assert lib.gpak_cv_folds(None, None, 1, None, None, None, None, 2) == gpak.EINVAL


# ---- the command line -----------------------------------------------------------------------------------------------
HOLES40 = "\n".join(str(i // 8) for i in range(40))


@pytest.mark.parametrize("labels,args,msg", [
    ("\n".join(str(i // 8) for i in range(39)), ["cv", "--folds", "folds.txt"], "--folds: folds.txt holds 39 labels for 40 training samples"),
    ("\n".join(str(i // 8) for i in range(41)), ["cv", "--folds", "folds.txt"], "holds 41 labels for 40 training samples"),
    ("\n".join(["0"] * 20 + ["1.5"] + ["2"] * 19), ["cv", "--folds", "folds.txt"], "--folds: '1.5' in"),
    ("\n".join(["0"] * 20 + ["fold7"] + ["2"] * 19), ["cv", "--folds", "folds.txt"], "--folds: 'fold7' in"),
    (HOLES40, ["cv", "--kfold", "1"], "--kfold: 1 folds for 40 training samples"),
    (HOLES40, ["cv", "--kfold", "41"], "--kfold: 41 folds for 40 training samples"),
    (HOLES40, ["cv", "--kfold", "four"], "--kfold takes the number of folds"),
    (HOLES40, ["cv", "--folds", "folds.txt", "--kfold", "4"], "exclude each other"),
    (HOLES40, ["cv", "--groups", "folds.txt", "--folds", "folds.txt"], "exclude each other"),
    (HOLES40, ["cv", "--kfold", "4", "--groups", "folds.txt"], "exclude each other"),
    (HOLES40, ["cv", "--seed", "3"], "--seed goes with --kfold"),
    (HOLES40, ["--gpus", "2", "cv", "--folds", "folds.txt"], "one GPU only"),
    (HOLES40, ["--gpus", "2", "cv", "--kfold", "4"], "one GPU only"),
])
def test_cli_refuses_before_a_context_exists(tmp_path, labels, args, msg):
    build()
    write_train(tmp_path / "train.txt", 40)
    (tmp_path / "folds.txt").write_text("# fold of each sample\n" + labels + "\n")
    r = subprocess.run([EXE, *args, "train.txt", "model", "out.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode(), r.stderr.decode()
    assert not any((tmp_path / f).exists() for f in ("out.txt", "model_folds.txt", "model_lgo.txt", "model_loo.txt"))


def test_cli_folds_needs_a_file():
    build()
    r = subprocess.run([EXE, "cv", "--folds"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and "--folds takes a file of labels" in r.stderr.decode()


def test_cli_groups_still_refuses_a_group_above_128(tmp_path):
    """The new dispatch does not leak into --groups."""
    build()
    write_train(tmp_path / "train.txt", 200)
    (tmp_path / "groups.txt").write_text("\n".join(["-3"] * 129 + ["4"] * 71) + "\n")
    r = subprocess.run([EXE, "cv", "--groups", "groups.txt", "train.txt", "model"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert "--groups: group -3 has more than 128 samples" in r.stderr.decode()
    assert not (tmp_path / "model_lgo.txt").exists() and not (tmp_path / "model_folds.txt").exists()


# ---- the fold assignment of --kfold -----------------------------------------------------------------------------------
def test_kfold_assignment_is_a_function_of_its_seed(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "kfold_assign.hpp"\n'
                   'int main(int, char **v){std::vector<int> f; gpak_kfold_assign(strtoull(v[1], 0, 10), (size_t)atoi(v[2]), atoi(v[3]), f);\n'
                   'for (int x : f) printf("%d\\n", x);\nreturn 0;}\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, str(src), "-o", exe])

    def folds(seed, n, k):
        return np.array(subprocess.check_output([exe, str(seed), str(n), str(k)]).split(), dtype=int)

    for n, k in ((40, 4), (513, 10), (7, 7), (9, 2)):
        a = folds(1, n, k)
        sizes = np.bincount(a, minlength=k)
        assert a.size == n and set(a.tolist()) == set(range(k)) and sizes.max() - sizes.min() <= 1
        assert np.array_equal(folds(1, n, k), a)
    assert not np.array_equal(folds(1, 513, 10), folds(2, 513, 10))
    assert not np.array_equal(folds(1, 513, 10), np.arange(513) % 10)          # shuffled at all
    # the generator and the loop are fixed by the standard and by the header: the first entries of seed 1, n = 10, K = 3
    # from this restatement of the header in Python's integers
    assert folds(1, 10, 3).tolist() == _kfold_restated(1, 10, 3)


def _mt19937_64(seed):
    """std::mt19937_64 (Matsumoto & Nishimura 2000, the constants of the C++ standard) as a generator of draws."""
    n, m, mask = 312, 156, (1 << 64) - 1
    mt = [seed & mask]
    for i in range(1, n):
        mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & mask)
    while True:
        for i in range(n):
            x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % n] & 0x7FFFFFFF)
            mt[i] = mt[(i + m) % n] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        for i in range(n):
            y = mt[i]
            y ^= (y >> 29) & 0x5555555555555555
            y ^= (y << 17) & 0x71D67FFFEDA60000
            y ^= (y << 37) & 0xFFF7EEE000000000
            y ^= y >> 43
            yield y & mask


def _kfold_restated(seed, n, k):
    gen = _mt19937_64(seed)
    perm = list(range(n))
    for i in range(n - 1, 0, -1):
        j = next(gen) % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    fold = [0] * n
    for pos, i in enumerate(perm):
        fold[i] = pos % k
    return fold
