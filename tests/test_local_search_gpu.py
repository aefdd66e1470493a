"""GPU tests (-m gpu) of the device neighbour search: gpak_local_neighbours_dev, gpak_dev_local_search and
`gp_ss_ak local --search device`.

The answer has one right value: the lists are ordered by (dist2, index), a total order, and dist2 has a stated rounding.  So
every comparison here is of BYTES -- against the host search, against a NumPy full sort (local_ref.brute_neighbours) and,
for dist2, against the stated unfused arithmetic (tests/local_search_ref.py).  No centre is left out of a comparison.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import local_ref  # noqa: E402
import local_search_ref as sr  # noqa: E402
import local_search_worker  # noqa: E402
import test_block_gpu as tb  # noqa: E402
from test_local import SEARCH, lattice, search_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    """a context with neither parameters nor a training set: the search needs the device and the stream only"""
    g = gpak.Gpak(0)
    yield g
    g.close()


def same(a, b):
    return a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def brute(case, k, radius):
    Xs, Xc, G = search_inputs(case)
    return local_ref.brute_neighbours(Xs, Xc, k, G, radius)


def check_against_brute(sg, Xs, Xc, k, G=None, radius=0.0):
    """the device lists, used and dist2 against the full sort and the stated arithmetic, as bytes; returns them"""
    want, want_used = local_ref.brute_neighbours(Xs, Xc, k, G, radius)
    nbr, used, d2, s = sg.local_neighbours_dev(Xs, Xc, k, G, radius, want_dist2=True)
    assert nbr.dtype == np.int32 and nbr.shape == (len(Xc), k) and used.dtype == np.int32 and d2.shape == nbr.shape
    assert same(nbr, want), np.flatnonzero((nbr != want).any(axis=1))[:8]
    assert same(used, want_used)
    assert same(d2, sr.dist2_lists(sr.transform(Xs, G), sr.transform(Xc, G), want))
    assert s["centres"] == len(Xc) and s["max_used"] == want_used.max() and s["batches"] == 1
    return nbr, used, d2, s


# ---- 1. bytes, through the context-level call ------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,radius", SEARCH, ids=[f"{c}-k{k}-r{r:g}" for c, k, r in SEARCH])
def test_device_search_equals_the_host_search_and_a_full_sort(sg, case, k, radius):
    Xs, Xc, G = search_inputs(case)
    want, want_used = brute(case, k, radius)
    host, host_used = gpak.local_neighbours(Xs, Xc, k, G, radius, threads=1)
    nbr, used, d2, s = sg.local_neighbours_dev(Xs, Xc, k, G, radius, want_dist2=True)
    none = sg.local_neighbours_dev(Xs, Xc, k, G, radius)
    print(f"\n{case} k={k} r={radius:g}: {s}")
    assert nbr.dtype == np.int32 and nbr.shape == (len(Xc), k) and used.shape == (len(Xc),)
    wrong = np.flatnonzero((nbr != host).any(axis=1))
    assert same(nbr, host) and same(used, host_used), wrong[:8]                      # every centre
    assert same(nbr, want) and same(used, want_used)
    want_d2 = sr.dist2_lists(sr.transform(Xs, G), sr.transform(Xc, G), want)
    assert same(d2, want_d2) and np.all(d2[nbr < 0] == 0.0)
    assert none[2] is None and same(none[0], nbr) and same(none[1], used)
    assert s["centres"] == len(Xc) and s["batches"] == 1 and s["max_used"] == used.max() and s["cells"] >= 1
    assert used.astype(np.int64).sum() <= s["visited"] <= len(Xs) * len(Xc)
    assert s["search_ms"] > 0 and s["grid_ms"] >= 0 and s["upload_ms"] >= 0


# ---- 2. boundaries -----------------------------------------------------------------------------------------------------
def crowd():
    """200 random samples and one sample 130 times; 12 centres, that sample itself and a point 1e6 away among them"""
    rng = np.random.default_rng(11)
    base = rng.random((200, 3))
    Xs = np.vstack([base[:120], np.tile(base[7], (130, 1)), base[120:]])
    Xc = np.vstack([rng.random((10, 3)) * 1.2 - 0.1, base[7], [[1e6, 0.5, 0.5]]])
    return Xs, Xc


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 127, 128])
def test_boundaries_of_the_list(sg, k):
    Xs, Xc = crowd()
    nbr, used, d2, _ = check_against_brute(sg, Xs, Xc, k)
    assert np.all(used == k) and np.all(d2[10, :min(k, 130)] == 0.0)               # the crowd, in index order
    assert np.array_equal(nbr[10, :min(k, 130)], np.flatnonzero((Xs == Xs[7]).all(axis=1))[:k])


def test_one_sample_and_more_neighbours_than_samples(sg):
    Xs, Xc = crowd()
    nbr, used, _, _ = check_against_brute(sg, Xs[:1], Xc, 128)
    assert np.all(used == 1) and np.all(nbr[:, 0] == 0) and np.all(nbr[:, 1:] == -1)
    nbr, used, _, s = check_against_brute(sg, Xs[:40], Xc, 128)
    assert np.all(used == 40) and np.all(nbr[:, 40:] == -1) and s["visited"] == 40 * len(Xc)


def test_radius_boundary_is_inside(sg):
    """a 7^3 lattice with radius exactly 2: the samples at dist2 == 4 are in, and used differs between the centres"""
    Xs = lattice(7)
    Xc = np.vstack([Xs[::19], [[3.0, 3.0, 3.0], [0.0, 0.0, 0.0], [-1.0, 3.0, 3.0]]])
    nbr, used, d2, _ = check_against_brute(sg, Xs, Xc, 128, radius=2.0)
    assert len(set(used.tolist())) > 2 and d2.max() == 4.0 and np.all(d2 <= 4.0)
    centre = len(Xc) - 3                                                             # (3, 3, 3): 33 lattice points within 2
    assert used[centre] == 33 and np.sum(d2[centre, :33] == 4.0) == 6


def test_radius_that_leaves_centres_empty(sg):
    Xs, Xc = crowd()
    nbr, used, d2, s = check_against_brute(sg, Xs, Xc, 17, radius=0.05)
    assert used.min() == 0 and used.max() == 17 and np.all(nbr[used == 0] == -1) and np.all(d2[used == 0] == 0.0)
    assert used[11] == 0                                                             # the point 1e6 away


# ---- 3. independence -------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_the_call_the_batch_or_the_other_centres(sg):
    Xs, Xc, G = search_inputs("anisotropic")
    M = len(Xc)
    a = sg.local_neighbours_dev(Xs, Xc, 128, G, want_dist2=True)
    b = sg.local_neighbours_dev(Xs, Xc, 128, G, want_dist2=True)
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2])
    sg.set_option(gpak.OPT_PRED_BATCH, 16)
    try:
        c = sg.local_neighbours_dev(Xs, Xc, 128, G, want_dist2=True)
    finally:
        sg.set_option(gpak.OPT_PRED_BATCH, 0)
    assert same(a[0], c[0]) and same(a[1], c[1]) and same(a[2], c[2])
    assert c[3]["batches"] == -(-M // 16) and a[3]["batches"] == 1 and c[3]["visited"] == a[3]["visited"]
    pick = np.array([41, 3, 17, 3, 0, 29])
    e = sg.local_neighbours_dev(Xs, Xc[pick], 128, G, want_dist2=True)
    assert same(e[0], a[0][pick]) and same(e[1], a[1][pick]) and same(e[2], a[2][pick])
    f = sg.local_neighbours_dev(Xs, Xc, 17, G, want_dist2=True)
    assert same(f[0], np.ascontiguousarray(a[0][:, :17])) and same(f[2], np.ascontiguousarray(a[2][:, :17])) and np.all(f[1] == 17)


# ---- 4. the kernel alone -----------------------------------------------------------------------------------------------
_KERNEL = {}


def kernel_records():
    if not _KERNEL:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_search_worker.py")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        _KERNEL["rc"], _KERNEL["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _KERNEL[rec["name"]] = rec
    return _KERNEL


@pytest.mark.parametrize("case", local_search_worker.CASES, ids=[local_search_worker.name_of(c) for c in local_search_worker.CASES])
def test_kernel_alone(case):
    """gpak_dev_local_search on caller-owned buffers and on grids the library did not build (tests/local_search_worker.py):
    lists, used and dist2 are the full sort's bytes on every grid; visited lies between what no exact search can skip and n
    per centre; guard words and operands untouched; every refusal writes nothing."""
    recs = kernel_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[local_search_worker.name_of(case)]
    print(f"\n{rec}")
    for key in ("rc", "lists", "used", "dist2", "guards", "operands_untouched", "refusals", "refusals_write_nothing", "optional_outputs"):
        assert rec[key] is True, (key, rec)
    assert rec["visited_floor"] <= rec["visited"] <= rec["visited_ceiling"]
    assert case[3] == 0.0 or rec["some_list_short"] is True                          # the radius decides something


# ---- 5. the context is left alone --------------------------------------------------------------------------------------
def test_a_trained_context_answers_as_before():
    X, y = tb.data(256, 3)
    Xte = tb.data(40, 3)[0] * 0.9 + 0.05
    Xs, Xc, G = search_inputs("random")
    g = gpak.Gpak(0)
    try:
        g.set_train(X, y)
        tb.set_defaults(g)
        nlz = g.logLikelihood()
        mean, var = g.posteriorMeanVar(Xte)
        nbr, used, _, _ = g.local_neighbours_dev(Xs, Xc, 17, G)
        mean2, var2 = g.posteriorMeanVar(Xte)
        nlz2 = g.logLikelihood()
        assert same(nbr, brute("random", 17, 0.0)[0])
        assert np.float64(nlz).tobytes() == np.float64(nlz2).tobytes() and same(mean, mean2) and same(var, var2)
    finally:
        g.close()


def test_statuses_leave_the_outputs_untouched(sg):
    Xs, Xc, G = search_inputs("random")
    Xs, Xc = np.asfortranarray(Xs), np.asfortranarray(Xc)
    lib, p = sg._lib, gpak._p
    nbr = np.full((len(Xc), 8), -9, dtype=np.int32)
    used = np.full(len(Xc), -9, dtype=np.int32)
    d2 = np.full((len(Xc), 8), 7.5)
    summ = _lib.LocalSearchSummary()
    ip = ctypes.POINTER(ctypes.c_int)

    def call(h=None, xs=Xs, xc=Xc, ns=len(Xs), d=3, m=len(Xc), G=None, k=8, radius=0.0, out=nbr):
        return lib.gpak_local_neighbours_dev(sg._h if h is None else h, p(xs), ns, d, p(xc), m, p(G), k, radius,
                                             None if out is None else out.ctypes.data_as(ip), used.ctypes.data_as(ip), p(d2),
                                             ctypes.byref(summ))

    bad, far = Xs.copy(order="F"), Xc.copy(order="F")
    bad[7, 1] = np.nan
    far[2, 0] = np.inf
    huge = np.asfortranarray(np.full((3, 3), 1e308))                                 # the transformed coordinates overflow
    einval = [call(xs=None), call(xc=None), call(out=None), call(d=2), call(d=5), call(k=0), call(k=129), call(ns=0), call(m=0),
              call(ns=2 ** 31 - 128), call(radius=float("nan")), call(xs=bad), call(xc=far),
              call(G=np.full((3, 3), np.nan, order="F")), call(G=huge)]
    assert einval == [gpak.EINVAL] * len(einval)
    multi = gpak.Gpak(devices=[0, 0])
    try:
        assert call(h=multi._h) == gpak.ENOTIMPL
        with pytest.raises(gpak.GpakError) as ei:
            multi.local_neighbours_dev(Xs, Xc, 8)
        assert ei.value.status == gpak.ENOTIMPL
    finally:
        multi.close()
    assert np.all(nbr == -9) and np.all(used == -9) and np.all(d2 == 7.5)           # nothing written
    assert call() == gpak.OK and np.all(used == 8) and summ.centres == len(Xc)
    assert same(nbr, brute("random", 8, 0.0)[0])


# ---- 6. the command line -----------------------------------------------------------------------------------------------
def test_cli_search_device_writes_the_same_file(tmp_path):
    """train on N = 400 (two iterations), then local on 50 nodes with the host and the device search, simple and ordinary
    kriging: the files are the same bytes, and the console names the device search and its three times."""
    import make_golden_lbfgs
    tb.build()
    N, M = 400, 50
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(51)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (M, 3))
    tb.write_csv(tmp_path / "nodes.txt", centres, np.linspace(-0.5, 0.5, M))
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)

    def local(out, *options):
        r = subprocess.run([exe, "-v", "1", "--neighbours", "24", "--radius", "0.6", *options, "local", str(tmp_path / "nodes.txt"), model,
                            str(tmp_path / "train.txt"), str(tmp_path / out)], cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
        return r.stdout.decode(), open(tmp_path / out, "rb").read()

    for kriging in ("simple", "ordinary"):
        bare_out, bare = local("bare.txt", "--kriging", kriging)
        host_out, host = local("host.txt", "--kriging", kriging, "--search", "host")
        dev_out, dev = local("dev.txt", "--kriging", kriging, "--search", "device")
        assert len(bare.splitlines()) == M + 1 and bare == host == dev
        assert "on the device (grid " in dev_out and "upload " in dev_out and "on the device" not in bare_out + host_out
        used = np.loadtxt(tmp_path / "dev.txt", comments="#")[:, 4]
        assert used.min() < 24 and used.max() > 0                                   # the radius decides something
