"""CPU tests (-m "not gpu") of ordinary kriging in a moving neighbourhood and of the octant search:

1. tests/local_ok_ref.py's block-elimination restatement (what gpak_predict_local_ok is compared with on the GPU) against
   its second route, the augmented (s + 1) x (s + 1) system built without the bias and solved with pivoting, in long
   double; the weights sum to one;
2. its float64 route against its long-double route on every case of local_cases.CASES, within the GPU tests' bound;
3. the invariances of ordinary kriging, in the reference;
4. gpak_local_neighbours_octant against a NumPy full sort, bit for bit;
5. the search source with a driver of its own under AddressSanitizer + UBSan and under ThreadSanitizer;
6. include/gpak_local_ok.h and include/gpak_dev_local_ok.h against the binding and the library;
7. the new options of the `local` verb: what is refused, before a context exists.

Bound of 1 and 3: the project's CPU bound, 1e-10 (tests/test_design.py), means relative to max|y|, variances to the prior
variance.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_cases as lc  # noqa: E402
import local_ok_ref as okr  # noqa: E402
import local_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
CSRC = os.path.join(ROOT, "gp_ss_ak_amd", "csrc")
CPU_BOUND = 1e-10
BOUND = 1e-8       # the GPU tests' bound (tests/test_block_gpu.py)
GPU_CASES = ["N300-M37-nd1-defaults", "N513-M130-nd8-defaults", "N300-M37-nd8-d4-defaults", "N513-M130-nd1-expans+rbf+bias+white"]


# ---- 1. the restatement against the augmented system -----------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_restatement_equals_the_augmented_system(name):
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    a = okr.reference(name)
    b = okr.local_predict_ok_augmented(Xs, ys, Xd, nd, nbr, terms, white, sn2)
    assert not a["notpd"].any() and np.array_equal(a["used"], b["used"])
    err = {key: okr.errors(comp, ys, b[key], a, key) for key in ("mean", "mu", "var", "latent")}
    ws = max(float(np.abs(a["wsum"] - 1).max()), float(np.abs(b["wsum"] - 1).max()))
    print(f"\n{name}: block elimination against the augmented system, long double: {err}, |sum of weights - 1| {ws:.3g} "
          f"(bound {CPU_BOUND:g})")
    assert max(err.values()) <= CPU_BOUND and ws <= CPU_BOUND


# ---- 2. float64 against long double ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_float64_route_meets_the_gpu_bound(name):
    Ns, M, nd, comp = lc.CASES[name]
    Xs, ys, Xd, nbr = lc.inputs(name)
    a, b = okr.reference(name, float), okr.reference(name)
    assert not a["notpd"].any() and not b["notpd"].any()
    assert np.all(np.isfinite(a["mean"])) and np.all(b["latent"].astype(float) > 0.0)
    err = {key: okr.errors(comp, ys, a[key], b, key) for key in ("mean", "mu", "var", "latent")}
    print(f"\n{name}: float64 against long double: {err} (bound {BOUND:g})")
    assert max(err.values()) <= BOUND


# ---- 3. invariances, in the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["N300-M37-nd1-defaults", "N300-M37-nd8-expans+rbf+bias+white"])
def test_invariances_of_the_reference(name):
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    base = okr.reference(name)
    ymax, prior = np.abs(ys).max(), tb.prior_variance(comp)
    # a constant added to the bias changes nothing
    more = okr.local_predict_ok(Xs, ys, Xd, nd, nbr, terms, bias + 3.0, white, sn2)
    for key in ("mean", "mu", "var", "latent"):
        assert okr.errors(comp, ys, more[key], base, key) <= CPU_BOUND, key
    # a constant added to ys is added to mean and mu; var does not move
    lifted = okr.local_predict_ok(Xs, ys + 7.25, Xd, nd, nbr, terms, bias, white, sn2)
    assert float(np.abs(lifted["mean"] - 7.25 - base["mean"]).max()) / ymax <= CPU_BOUND
    assert float(np.abs(lifted["mu"] - 7.25 - base["mu"]).max()) / ymax <= CPU_BOUND
    assert float(np.abs(lifted["var"] - base["var"]).max()) / prior <= CPU_BOUND
    # one sample: the estimate is that sample's value, and so is the local mean
    one = base["used"] == 1
    assert one.any()
    assert float(np.abs(base["mean"][one] - ys[nbr[one, 0]]).max()) / ymax <= CPU_BOUND
    assert float(np.abs(base["mu"][one] - ys[nbr[one, 0]]).max()) / ymax <= CPU_BOUND
    # not knowing the mean never lowers the variance: against simple kriging by local_ref, another code path
    sk = lc.reference(name)
    gap = (base["latent"] - sk["latent"]) / prior
    print(f"\n{name}: (OK latent - SK latent) / prior variance between {float(gap.min()):.3g} and {float(gap.max()):.3g}")
    assert float(gap.min()) >= -CPU_BOUND and float(gap.max()) > 0.1
    assert okr.errors(comp, ys, base["sk_latent"], sk, "latent") <= CPU_BOUND


def test_an_empty_list_has_no_estimate():
    cols, terms, bias, white, sn2 = tb.COMPS["defaults"]
    X, y = tb.data(300, cols)
    Xd = tb.blocks(300, cols, 3, 8)
    nbr = np.full((3, 4), -1)
    nbr[1, :2] = [5, 9]
    got = okr.local_predict_ok(X, y, Xd, 8, nbr, terms, bias, white, sn2, float)
    for key in ("mean", "var", "latent", "mu"):
        assert np.isnan(got[key][[0, 2]]).all() and np.isfinite(got[key][1])
    assert got["used"].tolist() == [0, 2, 0] and not got["notpd"].any()


# ---- 4. the octant search against a full sort ------------------------------------------------------------------------
def lattice(n, d=3):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=float)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.column_stack([g, (np.arange(len(g)) % 2).astype(float)]) if d == 4 else g


def octant_inputs(case):
    rng = np.random.default_rng(11)
    if case == "uniform":        # centres inside, on and outside the hull
        Xs = rng.random((2000, 3))
        Xc = np.vstack([rng.random((40, 3)), Xs[:10], rng.random((10, 3)) * [1.0, 1.0, 0.0], rng.random((10, 3)) + [1.05, 0.0, 0.0],
                        [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [-0.5, -0.5, 2.0]]])
        return Xs, Xc, None
    if case == "drillholes":     # clustered down the holes: a plain list fills from one direction
        Xs, _ = synth.drillholes(2000)
        Xs = np.asarray(Xs)
        return Xs, np.vstack([rng.random((50, 3)) * 2 - 1, Xs[::200], [[1.0, 1.0, 1.0], [-1.3, 0.0, 0.0]]]), None
    if case == "lattice":        # centres on lattice points: zero differences and equal distances everywhere
        Xs = lattice(7)
        return Xs, np.vstack([Xs[::5], Xs[::7] + 0.5, [[0.0, 3.0, 6.0], [-3.0, 2.0, 11.0]]]), None
    if case == "anisotropic":
        G = np.array([[2.0, 0.3, 0.0], [-0.4, 0.5, 0.1], [0.0, 0.2, 7.0]])
        return rng.random((2000, 3)) * [10.0, 3.0, 0.5], rng.random((50, 3)) * [11.0, 3.0, 0.5], G
    if case == "d4":
        Xs = np.column_stack([rng.random((1500, 3)), rng.integers(0, 3, 1500).astype(float)])
        Xc = np.column_stack([rng.random((40, 3)) * 1.2, rng.integers(0, 3, 40).astype(float)])
        return Xs, Xc, np.array([[1.0, 0.2, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.1, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 0.3]])
    if case == "d4-lattice":
        Xs = lattice(5, 4)
        return Xs, np.vstack([Xs[::3], Xs[::4] + [0.5, 0.0, 0.5, 0.0]]), None
    raise KeyError(case)


# (case, k, per_octant, radius)
OCTANT = [("uniform", 16, 2, 0.15), ("uniform", 24, 3, 0.02), ("uniform", 128, 16, 0.4), ("uniform", 8, 8, 0.2),
          ("drillholes", 16, 2, 0.3), ("drillholes", 24, 4, 0.6), ("drillholes", 128, 128, 0.5), ("drillholes", 5, 1, 0.05),
          ("lattice", 17, 3, 2.5), ("lattice", 8, 1, 1.0), ("lattice", 128, 16, 3.5),
          ("anisotropic", 16, 2, 1.5), ("anisotropic", 40, 7, 3.0),
          ("d4", 16, 2, 0.3), ("d4", 128, 20, 0.6), ("d4-lattice", 12, 2, 1.5)]


@pytest.mark.parametrize("case,k,per,radius", OCTANT, ids=[f"{c}-k{k}-n{n}-r{r:g}" for c, k, n, r in OCTANT])
def test_octant_search_equals_a_full_sort(case, k, per, radius):
    Xs, Xc, G = octant_inputs(case)
    want, want_used = okr.brute_octant_neighbours(Xs, Xc, k, per, G, radius)
    got, used = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=1, octant=per)
    assert got.dtype == np.int32 and got.shape == (len(Xc), k)
    assert np.array_equal(got, want) and np.array_equal(used, want_used)
    for threads in (3, 16):
        g2, u2 = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=threads, octant=per)
        assert g2.tobytes() == got.tobytes() and u2.tobytes() == used.tobytes()
    plain, plain_used = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=1)
    if per == k:                 # the limiting case: the plain search at the same radius
        assert plain.tobytes() == got.tobytes() and plain_used.tobytes() == used.tobytes()
    if (case, radius) in (("uniform", 0.02), ("drillholes", 0.05)):
        assert used.min() == 0 and used.max() > 0                            # a radius so small that some lists are empty
    if (case, k) in (("drillholes", 16), ("uniform", 16), ("lattice", 17)):
        # an octant with no sample inside the radius while another one overflows its cap: the centres on and off the hull
        inside = local_ref.brute_neighbours(Xs, Xc, 128, G, radius)[0]
        some = False
        for b in range(len(Xc)):
            I = inside[b][inside[b] >= 0]
            e = Xs[I, :3] - Xc[b, :3]
            octs = (e[:, 0] < 0) + 2 * (e[:, 1] < 0) + 4 * (e[:, 2] < 0)
            counts = np.bincount(octs, minlength=8)
            some |= bool(counts.min() == 0 and counts.max() > per and len(I) < 128)
        assert some
        assert not np.array_equal(got, plain)                                # and the cap changes lists


def test_octant_search_refuses_bad_arguments():
    rng = np.random.default_rng(4)
    Xs, Xc = rng.random((50, 3)), rng.random((5, 3))
    lib = _lib.load()
    ip = ctypes.POINTER(ctypes.c_int)
    nbr = np.full((5, 8), -9, dtype=np.int32)
    used = np.full(5, -9, dtype=np.int32)
    p = gpak._p

    def call(xs=Xs, xc=Xc, ns=50, d=3, m=5, G=None, k=8, per=2, radius=0.5, out=nbr):
        xs, xc = (None if a is None else np.asfortranarray(a) for a in (xs, xc))
        return lib.gpak_local_neighbours_octant(p(xs), ns, d, p(xc), m, p(G), k, per, radius, 1,
                                                None if out is None else out.ctypes.data_as(ip), used.ctypes.data_as(ip))

    bad = Xs.copy()
    bad[7, 1] = np.nan
    far = Xc.copy()
    far[2, 0] = np.inf
    for rc in (call(xs=None), call(xc=None), call(out=None), call(d=2), call(d=5), call(k=0), call(k=129), call(ns=0), call(m=0),
               call(xs=bad), call(xc=far), call(G=np.full((3, 3), np.nan, order="F")), call(radius=0.0), call(radius=-1.0),
               call(radius=np.nan), call(radius=np.inf), call(per=0), call(per=9), call(per=-1)):
        assert rc == gpak.EINVAL
    assert np.all(nbr == -9) and np.all(used == -9)          # nothing written
    assert call() == gpak.OK and np.all(used >= 0) and np.all(used <= 8)
    for kw in ({"radius": 0.0}, {}, {"radius": 0.5, "octant": 9}, {"radius": 0.5, "octant": -1}):
        with pytest.raises(gpak.GpakError):
            gpak.local_neighbours(Xs, Xc, 8, **{"octant": 2, **kw})
    # the default leaves the function as it is
    a, ua = gpak.local_neighbours(Xs, Xc, 8, None, 0.3, 1)
    b, ub = gpak.local_neighbours(Xs, Xc, 8, None, 0.3, 1, octant=0)
    assert a.tobytes() == b.tobytes() and ua.tobytes() == ub.tobytes()


# ---- 5. the search source with the octant driver under the sanitizers ------------------------------------------------
@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                                   ["-fsanitize=thread", "-static-libtsan"]], ids=["asan+ubsan", "tsan"])
def test_octant_search_is_clean_under_the_sanitizers(tmp_path, flags):
    exe = tmp_path / "local_octant_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "local_octant_main.cpp"),
                           os.path.join(CSRC, "local_search.cpp"), "-o", str(exe), "-lpthread"])
    # the runtimes are linked statically: the program runs in the environment as it is, whatever that preloads
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok" and not r.stderr, (r.stdout.decode(), r.stderr.decode())


# ---- 6. headers, binding, library ------------------------------------------------------------------------------------
def test_headers_binding_and_library_list_the_same_symbols():
    call, dev = header_functions("gpak_local_ok.h"), header_functions("gpak_dev_local_ok.h")
    assert call == sorted(_lib.LOCAL_OK_SYMBOLS) == ["gpak_local_neighbours_octant", "gpak_predict_local_ok"]
    assert dev == sorted(_lib.DEV_LOCAL_OK_SYMBOLS) == ["gpak_dev_local_krige_ok"]
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for name in call:
        assert [h for h in headers if name in header_functions(h)] == ["gpak_local_ok.h"]       # declared once
    assert [h for h in headers if "gpak_dev_local_krige_ok" in header_functions(h)] == ["gpak_dev_local_ok.h"]
    for h in ("gpak.h", "gpak_dev.h", "gpak_local.h", "gpak_dev_local.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "_ok" not in text and "octant" not in text, h
    assert len(header_functions("gpak_dev.h")) == 31
    assert not set(call + dev) & set(_lib.SYMBOLS + _lib.LOCAL_SYMBOLS + _lib.DEV_LOCAL_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in call + dev:
        assert hasattr(lib, name), name
    # a NULL context is refused without a device; so are NULL buffers of the device-pointer call
    vp = ctypes.c_void_p
    lib.gpak_predict_local_ok.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_int,
                                          vp, vp, vp, ctypes.c_int, vp]
    assert lib.gpak_predict_local_ok(None, None, None, 1, 3, None, 1, 1, None, 1, None, None, None, 0, None) == gpak.EINVAL
    lib.gpak_dev_local_krige_ok.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                            ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, vp, ctypes.c_int,
                                            ctypes.c_int, vp, vp, vp, vp]
    assert lib.gpak_dev_local_krige_ok(None, None, 1, 1, 1, None, 1, 1, None, None, 0.0, 0, 0.0, 0.1, None, 1, 0, None, None, None,
                                       None) == gpak.EINVAL


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_local_ok.h"\n#include "gpak_dev_local_ok.h"\n'
                   'int main(void){gpak_local_summary s; s.max_used = GPAK_LOCAL_MAX; s.batches = GPAK_LOCAL_LATENT; (void)s; '
                   'if (gpak_dev_local_krige_ok(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'if (gpak_local_neighbours_octant(0, 0, 3, 0, 0, 0, 1, 1, 1.0, 1, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_predict_local_ok(0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_search_source_still_compiles_alone(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", os.path.join(CSRC, "local_search.cpp"), "-o",
                           str(tmp_path / "s.o")])
    text = open(os.path.join(CSRC, "local_search.cpp")).read() + open(os.path.join(CSRC, "local_search.h")).read()
    assert "#include <hip" not in text and "gpak_internal.h" not in text and "gpak_local_neighbours_octant" in text


# ---- 7. the command line: the new refusals, before a context exists (no model file is ever read) ---------------------
def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


FILES = ["n.txt", "model", "train.txt"]
ONLY_LOCAL = "--kriging and --octant are options of the local verb"


@pytest.mark.parametrize("args,msg", [
    (["--neighbours", "64", "--kriging", "universal", "local", *FILES], "--kriging takes simple or ordinary"),
    (["--neighbours", "64", "--kriging", "", "local", *FILES], "--kriging takes simple or ordinary"),
    (["--neighbours", "64", "--octant", "4", "local", *FILES], "--octant needs --radius"),
    (["--neighbours", "64", "--radius", "1.5", "--octant", "0", "local", *FILES], "--octant takes the samples per octant, between 1 and --neighbours"),
    (["--neighbours", "64", "--radius", "1.5", "--octant", "65", "local", *FILES], "--octant takes the samples per octant, between 1 and --neighbours"),
    (["--neighbours", "64", "--radius", "1.5", "--octant", "x", "local", *FILES], "--octant takes the samples per octant, between 1 and --neighbours"),
    (["--kriging", "ordinary", "local", *FILES], "local needs --neighbours k, the samples per node, between 1 and 128"),
    (["--kriging", "ordinary", "test", *FILES], ONLY_LOCAL),
    (["--octant", "4", "--radius", "1", "cv", "train.txt", "model"], ONLY_LOCAL),
    (["--kriging", "simple", "block", *FILES], ONLY_LOCAL),
])
def test_cli_refuses_bad_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


def test_cli_passes_its_checks_up_to_the_model(tmp_path):
    """Both options with nothing wrong: the verb gets as far as the model's files, which are not there."""
    build()
    for name in ("n.txt", "train.txt"):
        with open(tmp_path / name, "w") as f:
            for i in range(10):
                f.write(f"{i}\t{2 * i}\t{3 * i}\t{0.5 * i}\n")
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--neighbours", "8", "--radius", "2.5", "--octant", "8", "--kriging", "ordinary",
                        "local", "-np", *FILES], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode != 0 and "--" not in err and "model" in err, err


def test_help_names_the_options():
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "local", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and "--kriging simple|ordinary" in r.stdout.decode() and "--octant n" in r.stdout.decode()
