"""CPU tests (-m "not gpu") of moving-neighbourhood kriging:

1. tests/local_ref.py (the NumPy restatement gpak_predict_local is compared with on the GPU) against a refit: with all s
   samples in every list it equals block_ref.block_predict on a model of exactly those samples -- mean, variance and latent
   variance -- for every composition of the GPU tests;
2. its float64 route against its long-double route on every case of the GPU tests, within the GPU tests' bound (so that
   bound is known to be reachable), and no node of any case fails to factor;
3. gpak_local_neighbours against a NumPy full sort, bit for bit;
4. the search source alone, with its own main, under AddressSanitizer + UBSan and under ThreadSanitizer;
5. include/gpak_local.h and include/gpak_dev_local.h against the binding and the library;
6. the `local` verb of the command line: what it refuses, before a context exists.

Bound of 1: the project's CPU bound, 1e-10 (tests/test_design.py), means relative to max|y|, variances to the prior variance.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref  # noqa: E402
import local_cases as lc  # noqa: E402
import local_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
CSRC = os.path.join(ROOT, "gp_ss_ak_amd", "csrc")
CPU_BOUND = 1e-10
BOUND = 1e-8       # the GPU tests' bound (tests/test_block_gpu.py)


# ---- 1. the restatement against a refit ------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 8])
@pytest.mark.parametrize("comp", lc.COMPS)
def test_restatement_matches_a_refit_on_the_listed_samples(comp, nd):
    s, M = 100, 12
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y = tb.data(300, cols)
    pick = np.arange(0, 300, 3)[:s]                           # the model holds these samples only
    Xd = tb.blocks(300, cols, M, nd)
    nbr = np.tile(np.arange(s, dtype=np.int32), (M, 1))
    want = block_ref.block_predict(X[pick], y[pick], Xd, nd, terms, bias, white, sn2)
    assert np.all(want["latent"] > 0.0)                       # block_ref clamps at 0: nothing is clamped here
    for dt in (float, local_ref.LD):
        got = local_ref.local_predict(X[pick], y[pick], Xd, nd, nbr, terms, bias, white, sn2, dt)
        em = float(np.abs(got["mean"] - want["mean"]).max() / np.abs(y).max())
        ev = float(np.abs(got["var"] - want["var"]).max() / tb.prior_variance(comp))
        el = float(np.abs(got["latent"] - want["latent"]).max() / tb.prior_variance(comp))
        print(f"\n{comp} nd={nd} {np.dtype(dt).name}: mean {em:.3g} of max|y|, variance {ev:.3g}, latent {el:.3g} of the prior "
              f"variance (bound {CPU_BOUND:g})")
        assert max(em, ev, el) <= CPU_BOUND and not got["notpd"].any()


def test_an_empty_list_is_the_prior():
    cols, terms, bias, white, sn2 = tb.COMPS["expans+rbf+bias+white"]
    X, y = tb.data(300, cols)
    Xd = tb.blocks(300, cols, 3, 8)
    got = local_ref.local_predict(X, y, Xd, 8, np.full((3, 4), -1), terms, bias, white, sn2, float)
    prior = block_ref._parts(X[:1], Xd, 8, terms, bias)[2] + white / 8
    assert np.all(got["mean"] == 0.0) and np.allclose(got["latent"], prior, rtol=1e-14) and np.all(got["used"] == 0)
    assert np.allclose(got["var"], prior + sn2 / 8, rtol=1e-14)


# ---- 2. float64 against long double on the GPU tests' cases ----------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_float64_route_meets_the_gpu_bound(name):
    Ns, M, nd, comp = lc.CASES[name]
    Xs, ys, Xd, nbr = lc.inputs(name)
    a, b = lc.reference(name, float), lc.reference(name)
    assert not b["notpd"].any() and not a["notpd"].any()     # the reference flags no node: a GPU test may leave out none
    assert sorted(set(b["used"])) == sorted(set(lc.S[:min(M, len(lc.S))])) and np.all(b["latent"].astype(float) > 0.0)
    em, ev = lc.errors(comp, ys, a["mean"], a["var"], b)
    _, el = lc.errors(comp, ys, a["mean"], a["latent"], b, "latent")
    print(f"\n{name}: float64 against long double: mean {em:.3g} of max|y|, variance {ev:.3g}, latent {el:.3g} of the prior "
          f"variance (bound {BOUND:g})")
    assert max(em, ev, el) <= BOUND


# ---- 3. the search against a full sort -------------------------------------------------------------------------------
def lattice(n, d=3):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=float)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.column_stack([g, (np.arange(len(g)) % 2).astype(float)]) if d == 4 else g


def search_inputs(case):
    rng = np.random.default_rng(7)
    if case == "random":
        return rng.random((700, 3)), rng.random((60, 3)) * 1.4 - 0.2, None
    if case == "lattice":       # centres on the lattice points and halfway between them: ties everywhere
        Xs = lattice(7)
        return Xs, np.vstack([Xs[::5], Xs[::7] + 0.5, [[-3.0, 2.0, 11.0]]]), None
    if case == "duplicates":    # every sample three times
        base = rng.random((90, 3))
        return np.vstack([base, base, base]), np.vstack([base[:20], rng.random((20, 3))]), None
    if case == "anisotropic":
        G = np.array([[2.0, 0.3, 0.0], [-0.4, 0.5, 0.1], [0.0, 0.2, 7.0]])
        return rng.random((600, 3)) * [10.0, 3.0, 0.5], rng.random((50, 3)) * [10.0, 3.0, 0.5], G
    if case == "d4":
        Xs = np.column_stack([rng.random((500, 3)), rng.integers(0, 3, 500).astype(float)])
        Xc = np.column_stack([rng.random((40, 3)), rng.integers(0, 3, 40).astype(float)])
        return Xs, Xc, np.diag([1.0, 2.0, 0.5, 0.7])
    if case == "d4-lattice":
        Xs = lattice(5, 4)
        return Xs, Xs[::3] + [0.5, 0.0, 0.5, 0.0], None
    if case == "flat":          # no extent in z, one sample far away
        Xs = np.column_stack([rng.random((300, 2)), np.zeros(300)])
        Xs[17] = [40.0, -3.0, 0.0]
        return Xs, np.column_stack([rng.random((30, 2)) * 2, rng.random(30) - 0.5]), None
    if case == "elongated":     # one dimension 1e5 times the others: far more cells along it than the grid allows itself
        Xs = rng.random((20000, 3)) * [1e5, 1.0, 1.0]
        return Xs, np.vstack([Xs[::400] + 0.25, [[1.2e5, 0.5, 0.5], [-3e4, 0.5, 0.5]]]), None
    if case == "outlier":       # one sample far from a dense set, and centres next to it
        Xs = rng.random((20000, 3))
        Xs[123] = [5e4, 0.5, 0.5]
        return Xs, np.vstack([rng.random((20, 3)), [[5e4 + 1.0, 0.5, 0.5], [4.9e4, 0.0, 1.0], [1e9, 0.0, 0.0]]]), None
    raise KeyError(case)


SEARCH = [(c, k, r) for c in ("random", "lattice", "duplicates", "anisotropic", "d4", "d4-lattice", "flat") for k in (1, 17, 128)
          for r in (0.0,)] + [("random", 17, 0.12), ("lattice", 128, 1.5), ("anisotropic", 17, 1.0), ("d4", 128, 0.3),
                           ("elongated", 8, 0.0), ("elongated", 8, 20.0), ("elongated", 128, 500.0), ("outlier", 8, 0.0), ("outlier", 8, 2.0),
                           ("outlier", 17, 1500.0)]


@pytest.mark.parametrize("case,k,radius", SEARCH, ids=[f"{c}-k{k}-r{r:g}" for c, k, r in SEARCH])
def test_search_equals_a_full_sort(case, k, radius):
    Xs, Xc, G = search_inputs(case)
    want, want_used = local_ref.brute_neighbours(Xs, Xc, k, G, radius)
    got, used = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=1)
    got4, used4 = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=4)
    got0, used0 = gpak.local_neighbours(Xs, Xc, k, G, radius)
    assert got.dtype == np.int32 and got.shape == (len(Xc), k)
    assert np.array_equal(got, want) and np.array_equal(used, want_used)
    assert got4.tobytes() == got.tobytes() == got0.tobytes() and used4.tobytes() == used.tobytes() == used0.tobytes()
    if radius > 0.0:           # some centres empty, some partly filled, or the radius decides nothing
        assert used.min() < k and (case != "random" or (used.min() == 0 and 0 < np.median(used) < k))
        assert case not in ("elongated", "outlier") or used.max() > 0


def test_search_with_more_neighbours_than_samples():
    rng = np.random.default_rng(3)
    Xs, Xc = rng.random((40, 3)), rng.random((9, 3))
    got, used = gpak.local_neighbours(Xs, Xc, 128)
    want, want_used = local_ref.brute_neighbours(Xs, Xc, 128)
    assert np.array_equal(got, want) and np.all(used == 40) and np.all(got[:, 40:] == -1) and np.array_equal(used, want_used)


def test_search_refuses_bad_arguments():
    rng = np.random.default_rng(4)
    Xs, Xc = rng.random((50, 3)), rng.random((5, 3))
    lib = _lib.load()
    ip = ctypes.POINTER(ctypes.c_int)
    nbr = np.full((5, 8), -9, dtype=np.int32)
    used = np.full(5, -9, dtype=np.int32)
    p = gpak._p

    def call(xs=Xs, xc=Xc, ns=50, d=3, m=5, G=None, k=8, out=nbr):
        xs, xc = (None if a is None else np.asfortranarray(a) for a in (xs, xc))
        return lib.gpak_local_neighbours(p(xs), ns, d, p(xc), m, p(G), k, 0.0, 1, None if out is None else out.ctypes.data_as(ip),
                                         used.ctypes.data_as(ip))

    bad = Xs.copy()
    bad[7, 1] = np.nan
    far = Xc.copy()
    far[2, 0] = np.inf
    for rc in (call(xs=None), call(xc=None), call(out=None), call(d=2), call(d=5), call(k=0), call(k=129), call(ns=0), call(m=0),
               call(xs=bad), call(xc=far), call(G=np.full((3, 3), np.nan, order="F"))):
        assert rc == gpak.EINVAL
    assert np.all(nbr == -9) and np.all(used == -9)          # nothing written
    assert call() == gpak.OK and np.all(used == 8)
    with pytest.raises(gpak.GpakError):
        gpak.local_neighbours(Xs, Xc, 129)


# ---- 4. the search source alone under the sanitizers -----------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                                   ["-fsanitize=thread", "-static-libtsan"]], ids=["asan+ubsan", "tsan"])
def test_search_is_clean_under_the_sanitizers(tmp_path, flags):
    exe = tmp_path / "local_search_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "local_search_main.cpp"),
                           os.path.join(CSRC, "local_search.cpp"), "-o", str(exe), "-lpthread"])
    # the runtimes are linked statically: the program runs in the environment as it is, whatever that preloads
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok" and not r.stderr, (r.stdout.decode(), r.stderr.decode())


# ---- 5. headers, binding, library ------------------------------------------------------------------------------------
def test_headers_binding_and_library_list_the_same_symbols():
    call, dev = header_functions("gpak_local.h"), header_functions("gpak_dev_local.h")
    assert call == sorted(_lib.LOCAL_SYMBOLS) == ["gpak_local_metric", "gpak_local_neighbours", "gpak_predict_local"]
    assert dev == sorted(_lib.DEV_LOCAL_SYMBOLS) == ["gpak_dev_local_krige"]
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for name in call:
        assert [h for h in headers if name in header_functions(h)] == ["gpak_local.h"]          # declared once
    assert [h for h in headers if "gpak_dev_local_krige" in header_functions(h)] == ["gpak_dev_local.h"]
    text = open(os.path.join(ROOT, "include", "gpak.h")).read()
    assert "gpak_local" not in text and "gpak_predict_local" not in text and "gpak_dev_local" not in text
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in call + dev:
        assert hasattr(lib, name), name
    s = _lib.LocalSummary()
    assert [n for n, _ in s._fields_] == ["upload_ms", "krige_ms", "nodes", "empty", "notpd", "batches", "max_used"]
    assert gpak.LOCAL_MAX == 128 and gpak.LOCAL_LATENT == 1
    # a NULL context is refused without a device; so are NULL buffers of the device-pointer call
    vp = ctypes.c_void_p
    lib.gpak_predict_local.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_int,
                                       vp, vp, ctypes.c_int, vp]
    assert lib.gpak_predict_local(None, None, None, 1, 3, None, 1, 1, None, 1, None, None, 0, None) == gpak.EINVAL
    lib.gpak_local_metric.argtypes = [vp, ctypes.c_int, vp]
    assert lib.gpak_local_metric(None, 0, None) == gpak.EINVAL
    lib.gpak_dev_local_krige.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                         ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, vp, ctypes.c_int,
                                         ctypes.c_int, vp, vp, vp]
    assert lib.gpak_dev_local_krige(None, None, 1, 1, 1, None, 1, 1, None, None, 0.0, 0, 0.0, 0.1, None, 1, 0, None, None,
                                    None) == gpak.EINVAL


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_local.h"\n#include "gpak_dev_local.h"\n'
                   'int main(void){gpak_local_summary s; s.max_used = GPAK_LOCAL_MAX; s.batches = GPAK_LOCAL_LATENT; (void)s; '
                   'if (gpak_dev_local_krige(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0.0, 0.0, 0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'if (gpak_local_metric(0, 0, 0) != GPAK_EINVAL) return 1; '
                   'if (gpak_local_neighbours(0, 0, 3, 0, 0, 0, 1, 0.0, 1, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_predict_local(0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_search_source_compiles_alone(tmp_path):
    """host code only: no HIP header, no other file of the library"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", os.path.join(CSRC, "local_search.cpp"), "-o",
                           str(tmp_path / "s.o")])
    text = open(os.path.join(CSRC, "local_search.cpp")).read() + open(os.path.join(CSRC, "local_search.h")).read()
    assert "#include <hip" not in text and "gpak_internal.h" not in text


# ---- 6. the command line: everything is refused before a context exists (no model file is ever read) ------------------
def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


FILES = ["n.txt", "model", "train.txt"]
NEED_K = "local needs --neighbours k, the samples per node, between 1 and 128"


@pytest.mark.parametrize("args,msg", [
    (["local", *FILES], NEED_K),
    (["--neighbours", "0", "local", *FILES], NEED_K),
    (["--neighbours", "129", "local", *FILES], NEED_K),
    (["--neighbours", "x", "local", *FILES], NEED_K),
    (["--neighbours", "64", "--radius", "0", "local", *FILES], "--radius takes a positive distance"),
    (["--neighbours", "64", "--radius", "-1.5", "local", *FILES], "--radius takes a positive distance"),
    (["--neighbours", "64", "--radius", "x", "local", *FILES], "--radius takes a positive distance"),
    (["--neighbours", "64", "--block-size", "1,1,1", "local", *FILES], "local takes --block-size and --block-disc together"),
    (["--neighbours", "64", "--block-disc", "2,2,2", "local", *FILES], "local takes --block-size and --block-disc together"),
    (["--gpus", "2", "--neighbours", "64", "local", *FILES], "single-GPU context (gpak_create) only: drop --gpus"),
    (["--neighbours", "64", "local", "n.txt", "model"], "There are not enough input parameters"),
    (["--neighbours", "64", "local", "--bogus", *FILES], "Unknown flag"),
])
def test_cli_refuses_bad_local_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


def write_rows(path, rows):
    with open(path, "w") as f:
        f.write("# comment\n")
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")


@pytest.mark.parametrize("node_cols,train_cols,msg", [
    (3, 4, "Nodes need 3 or 4 input columns."),              # two input columns and y
    (6, 4, "Nodes need 3 or 4 input columns."),
    (4, 5, "The samples need the nodes' input columns."),
    (5, 4, "The samples need the nodes' input columns."),
])
def test_cli_checks_the_columns_before_a_context_exists(tmp_path, node_cols, train_cols, msg):
    """No model file exists here, so passing a check would fail on reading it -- after all of these."""
    build()
    write_rows(tmp_path / "n.txt", [tuple(0.1 * i + c for c in range(node_cols)) for i in range(5)])
    write_rows(tmp_path / "train.txt", [tuple(0.3 * i + c for c in range(train_cols)) for i in range(10)])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--neighbours", "8", "local", "-np", *FILES], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and msg in r.stderr.decode(), r.stderr.decode()


def test_cli_local_passes_its_checks_up_to_the_model(tmp_path):
    """The same files with nothing wrong: the verb gets as far as the model's files, which are not there."""
    build()
    write_rows(tmp_path / "n.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(5)])
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(10)])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--neighbours", "128", "--radius", "2.5", "--block-size", "1,1,1",
                        "--block-disc", "2,2,2", "--latent", "local", "-np", *FILES], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode != 0 and "--" not in err and "model" in err, err


def test_help_names_the_verb():
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "local", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and "local :" in r.stdout.decode() and "--neighbours k" in r.stdout.decode()
