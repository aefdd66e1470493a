"""Every gpak_dev_* operation ALONE against a long-double reference (tests/dev_ops_cases.py): dispatch branches the
workload reaches only at its own sizes (the in-place rs<4,2,false> panel product above 160 tile rows, the scalar-base
GEMM at K >= 2048, the row splits of the packed back substitution), WHICH elements a kernel writes (tiles above the
diagonal, tiles with art < gct of the cyclic map, skew columns, rows past nrows, read-only operands, guard bands),
the edges of the super-tile walk, and the GPAK_EINVAL / no-op returns.

CPU (-m "not gpu"): the cases on the float64 restatement (tests/np_engine.py, tests/np_dist_engine.py) -- references,
masks and bounds agree with what the project itself says the operations do.  GPU (-m gpu): the same cases on
libgpak_hip.so, one fresh process per group.

Not covered here: gpak_dev_stream_create / gpak_dev_stream_destroy.  The two linear-algebra operations of the
distributed gradient, gpak_dev_grad_g_rows and gpak_dev_grad_binv_rows, are the group `grad`; the group `panel` holds
gpak_dev_factor_panel_co ALONE -- per element against a long-double Cholesky factor at W = 128 .. 1024, what it writes,
either build of the block kernel, and `info`: the minimum failing global column for matrices that fail at a chosen
column (tests/failcol_ref.py); the group `pairs` holds
either pair pass of csrc/grad.hip alone (gpak_dev_grad_pair_sums, gpak_dev_grad_pairs_rows) to a long-double sum over
the pairs, slot by slot, and the host ends of that chain (gpak_dev_grad_consts through the oracle, gpak_dev_grad_finish /
_finish_d).

The group `f32` holds the fp32 prediction kernels of a GPAK_F32 context alone (include/gpak_dev_f32.h): the three builds
of the fp32 product and its wide accumulation, the cross-kernel fill under every composition, the conversions, the row
sums and the ladder of the forward substitution.

Worst error / bound per group on an MI355X, and the float64-vs-long-double ratios that set the substitution
tolerances: DESIGN.md, "Device-level operations alone".
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dev_ops_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOT_COVERED = {"gpak_dev_stream_create", "gpak_dev_stream_destroy"}


def _worker(engine, groups, timeout):
    return subprocess.run([sys.executable, os.path.join(HERE, "dev_ops_worker.py"), "--engine", engine, "--group"] + list(groups),
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout)


def _records(r):
    recs = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
    if r.returncode == 3:
        pytest.skip(recs[-1]["skip"])
    return recs


def _assert_group(recs, group, r):
    mine = [x for x in recs if x.get("group") == group]
    expected = [n for g, n, _e, _f in dc.CASES if g == group]
    print(f"{group}: worst error / bound = {max([0.0] + [float(x['ratio']) for x in mine]):.3g}")
    for x in mine:
        print(f"  {x['case']}: ratio {x['ratio']}" + "".join(f", {k} {v:.3g}" for k, v in x["info"].items()))
        if len(x.get("ratios", {})) > 1:
            print("      " + ", ".join(f"{k} {float(v):.3g}" for k, v in x["ratios"].items() if float(v) > 0))
    for x in mine:
        name = x["case"]
        assert all(g == w for _l, g, w in x["rc"]), f"{name}: return codes (label, got, wanted) {x['rc']}"
        assert not x["violations"], f"{name}: elements written that the operation must leave alone: {x['violations']}"
        assert x["guards_ok"], f"{name}: a guard band was written"
        assert float(x["ratio"]) <= 1.0, f"{name}: error / bound = {x['ratio']}"
        assert x["deterministic"], f"{name}: two runs differ bit for bit"
        assert x["ok"], name
    assert [x["case"] for x in mine] == expected, (r.returncode, r.stderr.decode()[-3000:])


# ---- CPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def numpy_run():
    r = _worker("numpy", dc.GROUPS, 600)        # one process: the cases share the start-up cost
    return _records(r), r


@pytest.mark.parametrize("group", dc.GROUPS)
def test_cases_hold_on_the_float64_restatement(numpy_run, group):
    recs, r = numpy_run
    _assert_group(recs, group, r)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def test_every_declared_entry_point_has_a_case():
    declared = dc.declared_entry_points()
    covered = set(dc.covered_entry_points())
    missing = [n for n in declared if n not in covered and n not in NOT_COVERED]
    assert not missing, missing
    assert covered <= set(declared), sorted(covered - set(declared))
    assert {"gpak_dev_" + k for k in dc.SIG} >= covered


def test_sliced_long_double_product_matches_numpy():
    if not dc.long_double_ok():
        pytest.skip("np.longdouble is no wider than float64 on this host")
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((70, 200)) * 10.0 ** rng.integers(-3, 4, (70, 1)), rng.standard_normal((45, 200))
    plain = A.astype(np.longdouble) @ B.astype(np.longdouble).T
    scale = (np.abs(A) @ np.abs(B).T).astype(np.longdouble)
    assert (np.abs(dc.mm_ld(A, B) - plain) <= 200 * 2.0 ** -62 * scale).all()     # the plain product's own rounding
    Bl = B.astype(np.longdouble) / 3
    assert (np.abs(dc.mm_ld(A, Bl) - A.astype(np.longdouble) @ Bl.T) <= 200 * 2.0 ** -62 * scale).all()
    L = np.tril(rng.standard_normal((40, 40))) + 6 * np.eye(40)
    assert np.abs(dc.tri_inv_ld(L) @ L.astype(np.longdouble) - np.eye(40)).max() < 1e-17


def test_the_checks_bite():
    """An engine that is subtly wrong fails the case: a GEMM that forgets the skip rule writes the tiles above the
    diagonal, one that drops a k-column is far outside the bound, a stray store in a skew row or a guard band counts."""
    if not dc.long_double_ok():
        pytest.skip("np.longdouble is no wider than float64 on this host")
    cases = {n: f for _g, n, _e, f in dc.CASES}
    good = dc.numpy_ops()

    class Wrong:
        name = "wrong"

        def __init__(self, how):
            self.how = how

        def call(self, name, *a):
            a = list(a)
            if self.how == "no skip" and name == "update_rect":
                a[9] = 0
            if self.how == "short k" and name == "update_rect":
                a[4] -= 128
            rc = good.call(name, *a)
            if self.how == "skew" and name == "update_rect":
                a[5].data[a[7]] = 1.0                     # first skew row of column 0
            if self.how == "guard" and name == "update_rect":
                a[5].full[dc.GUARD - 1] = 1.0
            return rc

    name = "update_rect[1152,384,128,diag_first=1]"
    ok = dc.summarise(name, cases[name](good), cases[name](good))
    assert ok["ok"] and 0 < ok["ratio"] < 0.5
    for how, field in (("no skip", "violations"), ("skew", "violations"), ("guard", "guards_ok")):
        rec = dc.summarise(name, cases[name](Wrong(how)), cases[name](Wrong(how)))
        assert not rec["ok"] and (rec[field] if field == "violations" else not rec[field]), (how, rec)
    name = "update_rect[256,1152,512,diag_first=0]"
    rec = dc.summarise(name, cases[name](Wrong("short k")), cases[name](Wrong("short k")))
    assert not rec["ok"] and float(rec["ratio"]) > 1e10, rec
    _the_pair_checks_bite()
    _the_panel_checks_bite()
    _the_f32_checks_bite()


def _the_pair_checks_bite():
    """The same for the group `pairs`: wrong pair passes built on the float64 restatement (np_dist_engine.pair_sums) --
    one pair doubled, dropped, read from above the diagonal or from the wrong column group, one operand mis-indexed, two
    slots exchanged -- are at least 1000 bounds away, or show as NaN; the good engine is inside the bound."""
    cases = {n: f for _g, n, _e, f in dc.CASES}
    p0, p3, ex = ("pair_sums[as written,P=0,expans+bias,direct]", "pair_sums[as written,P=3,a=1,expans+bias,direct]",
                  "pair_sums[exact,P=0,expans+bias,direct]")
    good = dc.numpy_ops()
    for name in (p0, p3, ex):
        ok = dc.summarise(name, cases[name](good), cases[name](good))
        assert ok["ok"] and 0 < ok["ratio"] < 1, ok
    for how, name, want in (("diag2", p0, 1e3), ("last row", p0, 1e3), ("upper", p0, np.inf), ("unpermuted", p3, 1e3),
                            ("alpha row", p0, 1e3), ("dk", p0, np.inf), ("swap 9 10", ex, 1e3), ("store", p0, None)):
        wrong = dc.NumpyOps(mut=[how])
        rec = dc.summarise(name, cases[name](wrong), cases[name](wrong))
        print(how, rec["ratio"], rec["violations"])
        assert not rec["ok"], (how, rec)
        if want is None:
            assert rec["violations"] == {"binv": 1}, (how, rec)
        else:
            assert float(rec["ratio"]) >= want and not rec["violations"], (how, rec)


def _the_panel_checks_bite():
    """The same for the group `panel`: wrong panel factorisations built on the float64 restatement -- `col0` dropped (the
    column within the panel), the tile-local column, the last writer of `info` winning over the minimum, the second image
    of `inv` not transposed, one element above the diagonal written -- each fail at least one case; the good engine
    passes them all."""
    good = dc.numpy_ops()

    class WrongPanel:
        name = "wrong"

        def __init__(self, how):
            self.how = how

        def call(self, name, *a):
            if name not in ("factor_panel", "factor_panel_co"):
                return good.call(name, *a)
            blk, ld, Np, J, W, inv, info = a[:7]
            mine = np.full(4, dc.INT_MAX, dtype=np.int32)
            rc = good.call(name, *(a[:6] + (mine,) + a[7:]))
            col = int(mine[0])
            if col != dc.INT_MAX:
                if self.how == "col0 dropped":
                    col -= J
                elif self.how == "tile-local column":
                    col = (col - 1) % dc.TILE + 1
                elif self.how == "last writer wins":
                    info[0] = good.nde.last_reports[-1]          # a plain store: no minimum, the pre-set value lost
                    col = dc.INT_MAX
                info[0] = min(int(info[0]), col)
            iv = (inv.data if isinstance(inv, dc.Mat) else inv).reshape(W // dc.TILE, 2, dc.TILE, dc.TILE)
            if self.how == "inv not transposed":
                iv[:, 1] = iv[:, 0]
            if self.how == "above the diagonal":
                blk.get()[J + 3, 5] = 1e-300                     # inside the first diagonal 16-tile
            return rc

    panel = [(n, f) for g, n, _e, f in dc.CASES if g == "panel"]
    assert len(panel) == 28
    quick = [(n, f) for n, f in panel if "info" in n or "W=128," in n or n == "factor_panel[W=256,J=384,below=128]"]
    for n, f in quick:
        rec = dc.summarise(n, f(good), f(good))
        assert rec["ok"], rec
    fails = {}
    for how in ("col0 dropped", "tile-local column", "last writer wins", "inv not transposed", "above the diagonal"):
        fails[how] = [n for n, f in quick if not dc.summarise(n, f(WrongPanel(how)), f(WrongPanel(how)))["ok"]]
        print(how, "fails", fails[how])
        assert fails[how], how
    info_cases = {n for n, _f in quick if "info" in n}
    assert "factor_panel info[-1]" in fails["col0 dropped"] and "factor_panel info[-1]" in fails["tile-local column"]
    assert {"factor_panel info[two failures]", "factor_panel info[pre-set]"} <= set(fails["last writer wins"])
    assert set(fails["inv not transposed"]) == {n for n, _f in quick} - info_cases      # every accuracy case, no info case
    assert set(fails["above the diagonal"]) >= {n for n, _f in quick} - info_cases


def _the_f32_checks_bite():
    """The same for the group `f32`: wrong fp32 kernels built on the float32 restatements (dev_ops_cases.F32Restated) each
    fail the case named beside them; the good engine passes every one of those cases."""
    cases = {n: f for _g, n, _e, f in dc.CASES}
    wrong = (("f32 short k", "gemm_nt_f32[wide,rsd=4][1,1,256]"),                        # one 128-chunk of k dropped
             ("f32 plain", "gemm_nt_f32[wide,rsd=4][accumulates wide]"),                 # plain accumulation, positive operands
             ("f32 unpermuted", "gemm_nt_f32[plain][1,1,128]"),                          # rows 4 j + i left in MFMA order
             ("f32 beta0", "gemm_nt_f32[wide,rsd=4][3,2,128]"),                          # beta applied when it is 0: NaN leaks
             ("f32 rbf as exp", "fill_f32[rbf]"),                                        # the RBF child with the exponential profile
             ("f32 no col4", "fill_f32[expans d4]"),                                     # the 4th column ignored
             ("f32 pair kept", "fill_f32[expans]"),                                      # second element of the last valid row pair kept
             ("f32 white", "fill_f32[expans+rbf+bias,white=0.1]"),                       # White added on the coincident pair
             ("f32 clip skipped", "fwd_subst_f32[levels=128,512,mrows=128,wide,rsd=4]"), # the clipped last child skipped
             ("f32 inv transposed", "fwd_subst_f32[levels=128,mrows=128,plain]"),        # the transposed image of an inverse block
             ("f32 odd tail", "rowsumsq_f32[rows=255,cols=5,splits=5]"))                 # an odd split's last column dropped
    good = dc.numpy_ops()
    for _how, name in wrong:
        ok = dc.summarise(name, cases[name](good), cases[name](good))
        assert ok["ok"] and float(ok["ratio"]) < 1, ok
    for how, name in wrong:
        eng = dc.NumpyOps(mut=[how])
        rec = dc.summarise(name, cases[name](eng), cases[name](eng))
        print(how, "fails", name, "ratio", rec["ratio"], rec["violations"], [t for t in rec["rc"] if t[1] != t[2]])
        assert not rec["ok"], (how, rec)
        assert rec["guards_ok"] and rec["deterministic"], (how, rec)        # it fails for the value, not for a stray store


def test_f32_header_binding_and_library_agree():
    """include/gpak_dev_f32.h, the binding's list and the library's exports name the same functions, each has a signature
    in dev_ops_cases.SIG, and gpak_dev.h still includes nothing of it."""
    import ctypes
    from gp_ss_ak_amd import _lib
    with open(os.path.join(ROOT, "include", "gpak_dev_f32.h")) as f:
        txt = f.read()
    declared = sorted(set(re.findall(r"^int (gpak_dev_\w+)\(", txt, flags=re.M)))
    assert declared == sorted(_lib.DEV_F32_SYMBOLS) == sorted("gpak_dev_" + k for k in dc.F32_OPS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert set(declared) <= set(dc.declared_entry_points())
    import tempfile
    with tempfile.TemporaryDirectory() as d:                 # plain C, like the headers test_abi.py compiles
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "gpak_dev_f32.h"\nint main(void){return GPAK_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                               os.path.join(d, "t.o")])


# ---- GPU ---------------------------------------------------------------------------------------------------
_DEVICE_TROUBLE = []       # set by the first worker that faulted, aborted or hung: no further GPU process is started


def _gpu_group(group):
    if _DEVICE_TROUBLE:
        pytest.fail(f"not started: {_DEVICE_TROUBLE[0]}")
    try:
        r = _worker("hip", [group], 300)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"the worker of group {group} did not finish in 300 s")
        pytest.fail(_DEVICE_TROUBLE[0])
    err = r.stderr.decode()
    if r.returncode < 0 or r.returncode in (134, 139) or "HIP error" in err or "hipError" in err:
        _DEVICE_TROUBLE.append(f"the worker of group {group} ended with status {r.returncode}: {err[-1500:]}")
        pytest.fail(_DEVICE_TROUBLE[0])
    _assert_group(_records(r), group, r)
    assert r.returncode == 0, err[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("group", dc.GROUPS)
def test_device_ops_alone(group):
    _gpu_group(group)
