"""CPU tests (-m "not gpu") of the kernel-alone entries of the cross-validation code (include/gpak_dev_cv_kernels.h):

1. the header against the binding, the library and a C99 compiler, and every entry's GPAK_EINVAL on NULL buffers (no device
   is touched: the refusal comes before any launch);
2. tests/cv_kernels_ref.py pinned: its restatements chained together (Gram -> solve, sum of squares -> finish) reproduce
   tests/cvg_ref.py and tests/loo_ref.py on cases of those modules' own tests to 1e-12 relative, so the reference of a
   kernel is the operation the call performs; the closed-form Q is a factor of C; the fold stages chained reproduce the
   solve;
3. the cases of tests/test_cv_kernels_gpu.py: the layouts the issue of the Gram case asks for, kappa_2(S) <= 16 for every
   group, the constant c of the solve's bound, the failing pivots;
4. the bounds bite: against a reference with one deliberate error every comparison misses its bound by at least 1000 times.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_kernels_ref as kr  # noqa: E402
import cvg_ref  # noqa: E402
import dev_ops_cases as dc  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import loo_ref  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = kr.LD
BITE = 1000.0
SOLVE_C = 8.0       # DESIGN.md section 8 states it; SolveCase computes it

pytestmark = pytest.mark.skipif(not dc.long_double_ok(), reason="numpy's long double is no wider than double here")


# ---- 1. the header ------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_list_the_same_symbols():
    declared = header_functions("gpak_dev_cv_kernels.h")
    assert declared == sorted(_lib.DEV_CV_KERNELS_SYMBOLS) and len(declared) == 17
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for name in declared:
        assert [h for h in headers if name in header_functions(h)] == ["gpak_dev_cv_kernels.h"], name     # declared once
    assert len(header_functions("gpak_dev.h")) == 31
    assert header_functions("gpak_dev_cv.h") == ["gpak_dev_pack_rows"]
    assert header_functions("gpak_dev_cv_mix.h") == ["gpak_dev_mix_cols"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_every_entry_is_launched_by_the_gpu_worker():
    import cv_kernels_worker as worker
    launched = sorted("gpak_dev_" + e for fam in worker.FAMILIES for e in worker.ENTRIES[fam])
    assert launched == sorted(_lib.DEV_CV_KERNELS_SYMBOLS)
    text = open(os.path.join(ROOT, "tests", "cv_kernels_worker.py")).read()
    for e in (e for fam in worker.FAMILIES for e in worker.ENTRIES[fam]):
        assert f'r.call("{e}"' in text, e


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_dev_cv_kernels.h"\n'
                   'int main(void){ if (gpak_dev_cvf_pad(0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_dev_lgo_colscale(0, 0, 0, 0.0, 0) == GPAK_EINVAL ? GPAK_OK : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_null_buffers_are_refused_before_any_launch():
    lib = _lib.load()
    n, z = None, 0
    calls = {
        "gpak_dev_cvg_gram": (n, n, 128, 128, n, n, 1, n, n),
        "gpak_dev_cvg_solve": (n, n, n, n, n, 1, 1, n, n, 1.0, n, n, n, n, n, n, n, n),
        "gpak_dev_cvg_mix": (n, n, 128, 128, n, n, 1, n),
        "gpak_dev_cvf_pad": (n, n, 128, 1),
        "gpak_dev_cvf_w": (n, n, 128, 1, n, n, n),
        "gpak_dev_cvf_ev": (n, n, 128, 1, n, n, n, 1.0, n, n, n, n, n),
        "gpak_dev_cvf_sums": (n, n, 128, 1, n, n, n, n, 1.0, n, n, n),
        "gpak_dev_cvf_beta": (n, n, 1, 1.0, n),
        "gpak_dev_cvf_q": (n, z, n, 128, 1, n, n, n, n, n, 128, n),
        "gpak_dev_cvf_gather": (n, n, 128, 128, n, 1, n, 128),
        "gpak_dev_cvf_unmix": (n, n, 128, 128, n, 1, n, 128),
        "gpak_dev_loo_rowsumsq": (n, n, 128, 128, 1, 0, n, n),
        "gpak_dev_loo_finish": (n, 1, n, n, n, 1.0, n, n, n, n),
        "gpak_dev_loo_vectors": (n, 1, 128, n, n, 1.0, n, n),
        "gpak_dev_loo_mirror_scale": (n, 1, 128, n, 128, n, n, 128),
        "gpak_dev_loo_rank2": (n, 128, n, 128, n, n),
        "gpak_dev_lgo_colscale": (n, 1, 128, 1.0, n),
    }
    assert sorted(calls) == sorted(_lib.DEV_CV_KERNELS_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == gpak.EINVAL, name


# ---- 2. the references are the operations of the calls ------------------------------------------------------------------
def _factor(K, y, sn2):
    """G = L^-T and alpha as tests/cvg_ref.py and tests/loo_ref.py form them"""
    N = K.shape[0]
    L = np.linalg.cholesky(np.eye(N) + K / sn2)
    G = np.triu(np.linalg.solve(L, np.eye(N)).T)
    return G, np.linalg.solve(L.T, np.linalg.solve(L, y / sn2))


def _problem(N):
    X, y = synth.drillholes(N)
    sn2 = synth.DEFAULT_SN2
    return xref.gram(X, [(xref.EXPANS, list(synth.DEFAULT_EXPANS))], synth.DEFAULT_BIAS), y, sn2


def test_gram_then_solve_is_cv_groups():
    """N = 200, the defaults, groups of sizes 1, 2, 127, 128 (a case of tests/test_cv_groups.py): gram_ref -> solve_ref against
    cvg_ref.cv_groups, 1e-12 relative (the mean of max|y|)."""
    K, y, sn2 = _problem(200)
    labels = cvg_ref.mixed_sizes(200)
    mean, var, logp, md = cvg_ref.cv_groups(K, y, sn2, labels)
    G, alpha = _factor(K, y, sn2)
    worst = 0.0
    for g, I in enumerate(cvg_ref.members(labels)):
        S = np.asarray(kr.gram_ref(G, I)[0], dtype=np.float64)
        r = kr.solve_ref(S, alpha[I], y[I], sn2)
        errs = [np.abs(r["mean"] - mean[I]).max() / np.abs(y).max(), (np.abs(r["var"] - var[I]) / var[I]).max(),
                abs(r["logp"] - logp[g]) / abs(logp[g]), abs(r["gsum"][2] - md[g]) / abs(md[g])]
        worst = max(worst, float(max(errs)))
    print(f"\nworst relative difference {worst:.3g}")
    assert worst <= 1e-12


def test_rowsumsq_then_finish_is_loo():
    """N = 200, the defaults (a case of tests/test_loo.py): rowsumsq_ref -> finish_ref against loo_ref.loo and its summary."""
    K, y, sn2 = _problem(200)
    mean, var = loo_ref.loo(K, y, sn2)
    G, alpha = _factor(K, y, sn2)
    d = np.asarray(kr.rowsumsq_ref(G)[0], dtype=np.float64)
    f = kr.finish_ref(d, y, alpha, sn2)
    em = float(np.abs(f["mean"][0] - mean).max() / np.abs(y).max())
    ev = float((np.abs(f["var"][0] - var) / var).max())
    want = loo_ref.summary(y, mean, var)
    s = f["sums"][0]
    es = max(abs(float(s[0]) / 200 - want["mse"]) / want["mse"], abs(float(s[1]) / 200 - want["mssr"]) / want["mssr"],
             abs(float(-0.5 * (s[1] + s[2] + 200 * kr.LOG2PI_LD)) - want["log_pl"]) / abs(want["log_pl"]))
    print(f"\nmean {em:.3g}, var {ev:.3g}, summary {es:.3g}")
    assert max(em, ev, es) <= 1e-12


def test_fold_stages_chained_are_the_solve():
    """The references of w, e / var, the sums, beta and Q of a one-at-a-time group, chained on T = R^-T of a group's S,
    reproduce solve_ref on the same S (long double against long double: 1e-15 relative)."""
    sc = kr.solve_case()
    g = 12                                                             # 113 members
    I, S, r = sc.groups[g], sc.S[g], sc.ref[g]
    m = len(I)
    fc = kr.FoldCase.__new__(kr.FoldCase)
    fc.m, fc.mp, fc.sn2 = m, kr.pad128(m), sc.sn2
    fc.rows = np.arange(m, dtype=np.int32)
    fc.alpha, fc.y = np.resize(sc.alpha[I], kr.FOLD_NP), np.resize(sc.y[I], kr.FOLD_NP)
    T = r["X"].T                                                       # long double
    fc.Tz = T
    w = fc.expect_w()["wv"][0]
    fc.wv = w
    ev = fc.expect_ev()
    fc.ev, fc.vv, fc.rdiag = ev["ev"][0], ev["vv"][0], np.diag(r["R"])
    sums = fc.expect_sums()
    fc.sc = np.array([fc.expect_beta()["sc0"][0], fc.expect_beta()["sc1"][0]], dtype=LD)
    Q = fc.expect_q(False)["Q"][0][:m, :m]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())     # noqa: E731
    errs = [rel(w, r["w"]), rel(ev["ev"][0], r["e"]), rel(ev["var"][0], r["var"]), rel(ev["mean"][0], r["mean"]),
            rel(sums["gsum"][0], r["gsum"]), rel(np.array([sums["logp"][0]]), np.array([r["logp"]])), rel(Q, r["Q"])]
    print("\n" + " ".join(f"{e:.2g}" for e in errs))
    assert max(errs) <= 1e-15


def test_q_of_the_solve_reference_is_a_factor_of_c():
    sc = kr.solve_case()
    for g in range(len(sc.groups)):
        C, _ = sc.c_ref(g)
        Q = sc.ref[g]["Q"]
        assert float(np.abs(Q @ Q.T - C).max() / np.abs(C).max()) <= 1e-17, g


# ---- 3. the cases --------------------------------------------------------------------------------------------------------
def test_gram_layouts_are_what_the_case_promises():
    gc = kr.gram_case()
    sizes = [len(I) for I in gc.groups]
    assert tuple(sizes) == kr.GRAM_SIZES and sorted({kr.pad16(s) // 16 for s in sizes}) == list(range(1, 9))
    every = np.concatenate(gc.groups)
    assert len(np.unique(every)) == len(every) == 947 and every.min() == 0 and every.max() < gc.Np     # disjoint; 77 left out
    assert all(np.all(np.diff(I) > 0) for I in gc.groups)                                              # members ascending
    assert gc.groups[kr.GRAM_SIZES.index(128)][0] == 0                                                 # one starts at row 0
    last = gc.groups[kr.GRAM_SIZES.index(64)]
    assert last.min() >= gc.Np - 128 and np.all(np.diff(last) == 1)                                    # wholly in the last tile
    scattered = [I for I in gc.groups if len(I) > 1 and np.all(np.diff(I) == 7)]
    assert len(scattered) == 13
    assert sorted({r[2] for r in gc.ref}) == [0, 384, 512, 640, 768, 896]              # loops from 1024 down to 128 columns
    assert np.all(np.tril(gc.G, -1) == 0.0)


def test_solve_case_conditioning_and_constant():
    sc = kr.solve_case()
    print(f"\nkappa_2 in [{min(sc.kappa):.3g}, {max(sc.kappa):.3g}]; float64 restatement {sc.f64_ratio:.3g} of the c = 1 bound; "
          f"c = {sc.c:g}")
    assert max(sc.kappa) <= 16.0
    assert sc.c == SOLVE_C and sc.f64_ratio * 8 < sc.c <= sc.f64_ratio * 16
    for g, col in kr.SOLVE_FAIL.items():                               # the pivot fails at the chosen column, not before
        R, fail = kr.chol_lower(sc.S_fail[g], LD)
        assert fail == col and col < len(sc.groups[g])
        assert np.array_equal(np.delete(sc.S_fail[g].ravel(), col * (len(sc.groups[g]) + 1)),
                              np.delete(sc.S[g].ravel(), col * (len(sc.groups[g]) + 1)))


# ---- 4. the bounds bite --------------------------------------------------------------------------------------------------
def test_gram_bound_bites():
    gc = kr.gram_case()
    for g, (S, bound, _) in enumerate(gc.ref):
        assert kr.worst(gc.wrong(g) - S, bound) >= BITE, g


def test_solve_bound_bites():
    """two members swapped; a group of one has no two members: its neighbouring row's alpha is used"""
    sc = kr.solve_case()
    for g, I in enumerate(sc.groups):
        if len(I) == 1:
            w = kr.solve_ref(sc.S[g], sc.alpha[I + 1], sc.y[I], sc.sn2)
        else:
            w = sc.wrong(g)
        r = sc.ref[g]
        for k in ("e", "logp", "Q"):
            assert kr.worst(w[k] - r[k], sc.bound(g, k)) >= BITE, (g, k)
        assert kr.worst(w["gsum"] - r["gsum"], sc.bound(g, "gsum")) >= BITE, g
        assert kr.worst(w["mean"] - r["mean"], sc.mean_bound(g)) >= BITE, g
        # var does not depend on alpha: a neighbouring member's variance instead
        if len(I) > 1:
            assert kr.worst(np.roll(r["var"], 1) - r["var"], sc.bound(g, "var")) >= BITE, g
        C, cb = sc.c_ref(g)
        assert kr.worst(w["Q"] @ w["Q"].T - C, cb) >= BITE, g


def test_mix_bound_bites():
    mc = kr.mix_case()
    for b in range(len(kr.MIX_WIDTHS)):
        ref, bound = mc.expect(b)
        assert kr.worst(mc.wrong(b) - ref, bound) >= BITE, b


@pytest.mark.parametrize("m", kr.FOLD_M)
def test_fold_bounds_bite(m):
    fc = kr.fold_case(m)
    pairs = [(fc.expect_w(), fc.expect_w(shift=1)), (fc.expect_ev(), fc.expect_ev(shift=1)),
             (fc.expect_sums(), fc.expect_sums(swap=True)), (fc.expect_beta(), fc.expect_beta(drop=True)),
             (fc.expect_q(False), fc.expect_q(False, shift=1)), (fc.expect_q(True), fc.expect_q(True, shift=1))]
    hit = set()
    for good, bad in pairs:
        for k, (ref, bound) in good.items():
            if kr.worst(np.asarray(bad[k][0] - ref), bound) >= BITE:
                hit.add(k)
    # what the errors above cannot move: sc0 and vv / var do not depend on the shifted input; gsum's first two entries
    # not on alpha -- the entry that does is checked by itself
    assert hit >= {"wv", "ev", "mean", "logp", "sc1", "Q"}, hit
    good, bad = fc.expect_sums(), fc.expect_sums(swap=True)
    assert kr.worst(bad["gsum"][0][2] - good["gsum"][0][2], good["gsum"][1][2]) >= BITE
    ev = fc.expect_ev()
    assert kr.worst(np.roll(ev["vv"][0], 1) - ev["vv"][0], ev["vv"][1]) >= BITE           # a neighbouring row's variance


def test_loo_bounds_bite():
    lc = kr.loo_case()
    assert kr.worst(lc.d_wrong() - lc.d_ld, lc.d_bound) >= BITE
    good, bad = lc.expect_finish(), lc.expect_finish(shift=1)
    assert kr.worst(bad["mean"][0] - good["mean"][0], good["mean"][1]) >= BITE
    assert kr.worst(np.roll(good["var"][0], 1) - good["var"][0], good["var"][1]) >= BITE  # var: a neighbouring row's d
    assert kr.worst((bad["sums"][0] - good["sums"][0])[:2], good["sums"][1][:2]) >= BITE
    d2 = lc.d.copy()
    d2[:lc.N] = np.roll(d2[:lc.N], 1)
    d2[0] *= 1.5                                                       # a permutation alone leaves the sum of logs alone
    logs = kr.finish_ref(d2[:lc.N], lc.y[:lc.N], lc.alpha[:lc.N], lc.sn2)["sums"][0][2]
    assert kr.worst(logs - good["sums"][0][2], good["sums"][1][2]) >= BITE
    good, bad = lc.expect_vectors(), lc.expect_vectors(shift=1)
    for k in ("s", "r"):
        assert kr.worst(bad[k][0] - good[k][0], good[k][1]) >= BITE, k
    ref, bound = lc.expect_rank2()
    low = kr.lower_tiles(lc.Np, 64)
    assert kr.worst((lc.expect_rank2(shift=1)[0] - ref)[low], bound[low]) >= BITE
