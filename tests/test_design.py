"""CPU tests (-m "not gpu") of infill drilling design:

1. tests/design_ref.py (the NumPy restatement gpak_design is compared with on the GPU) against refits: for every hole,
   reduction[:, h] = the latent block variances of block_ref.block_predict on the training set minus those on the training
   set with the hole appended, and var_after = the refit variances with all picked holes appended;
2. its float64 route against its long-double route;
3. the pick order of every case the GPU tests take picks from: at every step the two largest long-double gains differ by
   at least 1e-6 of the largest, and the case built to tie exactly goes to the smaller label;
4. include/gpak_design.h and include/gpak_dev_design.h against the binding and the library;
5. the `design` verb of the command line: what it accepts and refuses, before any device is opened.

Bound of 1 and 2: the project's CPU bound, 1e-10 of the prior variance (tests/test_block.py, tests/test_joint.py), times
sum(wt) for the weighted sums.
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
import design_cases as dc  # noqa: E402
import design_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
CPU_BOUND = 1e-10
GAP = 1e-6
NAMES = list(dc.CASES)


def latent(name, extra):
    """latent block variances of the case's targets by block_ref on the training set with the points `extra` appended"""
    N, comp, T, nd, layout, k = dc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = dc.inputs(name)
    Xa = np.vstack([X, extra]) if len(extra) else X
    ya = np.concatenate([y, np.zeros(len(extra))])
    return block_ref.block_predict(Xa, ya, Xt, nd, terms, bias, white, sn2)["latent"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_refits(name):
    N, comp, T, nd, layout, k = dc.CASES[name]
    X, y, Xt, Xc, hole = dc.inputs(name)
    pv = tb.prior_variance(comp)
    got = dc.reference(name, False, float)
    base = latent(name, Xc[:0])
    assert np.all(base > 0.0)                                   # block_ref clamps at 0: nothing is clamped here
    worst = np.abs(got["var"] - base).max() / pv
    for h in range(int(hole.max()) + 1):
        after = latent(name, Xc[hole == h])
        assert np.all(after > 0.0)
        worst = max(worst, np.abs(got["reduction"][:, h] - (base - after)).max() / pv)
    picked = np.isin(hole, got["picked"])
    after = latent(name, Xc[picked])
    assert np.all(after > 0.0) and len(got["picked"]) == k
    e_after = np.abs(got["var_after"] - after).max() / pv
    print(f"\n{name}: reduction and var against refits {worst:.3g}, var_after {e_after:.3g} of the prior variance "
          f"(bound {CPU_BOUND:g})")
    assert worst <= CPU_BOUND and e_after <= CPU_BOUND


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_float64_route_matches_long_double(name, weighted):
    N, comp, T, nd, layout, k = dc.CASES[name]
    pv = tb.prior_variance(comp)
    a, b = dc.reference(name, weighted, float), dc.reference(name, weighted)
    sw = float(dc.weights(T).sum()) if weighted else float(T)
    errs = {key: float(np.abs(np.asarray(a[key], dtype=float) - np.asarray(b[key]).astype(float)).max()) / (pv * scale)
            for key, scale in (("gain", sw), ("pick_gain", sw), ("reduction", 1.0), ("var", 1.0), ("var_after", 1.0))}
    print(f"\n{name} weighted={weighted}: " + ", ".join(f"{key} {v:.3g}" for key, v in errs.items()) + f" (bound {CPU_BOUND:g})")
    assert a["picked"] == b["picked"] and max(errs.values()) <= CPU_BOUND


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pick_order_is_decided_by_a_margin(name, weighted):
    """What lets the GPU tests ask for EQUAL picks: no step of any plan is decided by less than 1e-6 of the largest gain --
    except one step of "twins", which is an exact tie by construction and goes to the smaller label."""
    N, comp, T, nd, layout, k = dc.CASES[name]
    ref = dc.reference(name, weighted)
    gaps = design_ref.pick_gaps(ref["rounds"])
    print(f"\n{name} weighted={weighted}: picks {ref['picked']}, gaps {['%.3g' % g for g in gaps]}")
    assert len(gaps) == k
    if layout == "twins":
        tie = [p for p, g in enumerate(gaps) if g == 0.0]
        assert len(tie) == 1                                     # one step of the plan is the tie
        g = ref["rounds"][tie[0]]
        assert g[1] == g[3] and np.all(g[1] > np.delete(g, [1, 3])[~np.isnan(np.delete(g, [1, 3]).astype(float))])
        assert ref["picked"][tie[0]] == 1                        # the twins lead, exactly level: the smaller label
        gaps = [g for p, g in enumerate(gaps) if p != tie[0]]
    assert all(g >= GAP for g in gaps)


def test_twins_share_their_points():
    X, y, Xt, Xc, hole = dc.inputs("N200-defaults-T17-nd8-twins")
    assert np.array_equal(Xc[hole == 1], Xc[hole == 3]) and int(hole.max()) == 3


def test_layout_sizes_is_what_the_gpu_case_needs():
    N, comp, T, nd, layout, k = dc.CASES["N513-defaults-T130-nd8-sizes"]
    X, y, Xt, Xc, hole = dc.inputs("N513-defaults-T130-nd8-sizes")
    sizes = np.bincount(hole)
    assert sorted(sizes[:6]) == [1, 15, 16, 17, 127, 128] and list(sizes[6:]) == [20, 20]
    for h in (4, 5):      # its rows straddle a multiple of 128 (the targets are padded to a multiple of 256 in front)
        rows = np.flatnonzero(hole == h)
        assert rows[0] // 128 != rows[-1] // 128
    rows = np.flatnonzero(hole == 6)
    assert np.any(np.diff(rows) > 1)                            # not contiguous


def test_headers_binding_and_library_list_the_same_symbols():
    call, dev = header_functions("gpak_design.h"), header_functions("gpak_dev_design.h")
    assert call == sorted(_lib.DESIGN_SYMBOLS) == ["gpak_design"]
    assert dev == sorted(_lib.DEV_DESIGN_SYMBOLS) == ["gpak_dev_design_score"]
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for name, own in (("gpak_design", "gpak_design.h"), ("gpak_dev_design_score", "gpak_dev_design.h")):
        assert [h for h in headers if name in header_functions(h)] == [own]          # declared once
    text = open(os.path.join(ROOT, "include", "gpak.h")).read()
    assert "gpak_design" not in text and "gpak_dev_design" not in text
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in call + dev:
        assert hasattr(lib, name), name
    s = _lib.DesignSummary()
    assert [n for n, _ in s._fields_] == ["var_before", "var_after", "ms", "holes", "max_size", "picks"]
    # a NULL context is refused without a device; so are NULL buffers of the device-pointer call
    vp = ctypes.c_void_p
    lib.gpak_design.argtypes = [vp, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, vp, ctypes.c_int, vp,
                                ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
    assert lib.gpak_design(None, None, 1, 1, None, 1, 3, None, 1, None, 0, None, None, None, None, None, None, None) == gpak.EINVAL
    lib.gpak_dev_design_score.argtypes = [vp, vp, ctypes.c_long, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_double, vp, vp,
                                          vp, ctypes.c_long, vp]
    assert lib.gpak_dev_design_score(None, None, 256, 1, None, None, None, 1, 0.0, None, None, None, 0, None) == gpak.EINVAL


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_design.h"\n#include "gpak_dev_design.h"\n'
                   'int main(void){gpak_design_summary s; s.picks = GPAK_CV_GROUP_MAX; (void)s; '
                   'if (gpak_dev_design_score(0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_design(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


# ---- the command line: everything is refused before a context exists (no model file is ever read) ----------------------
def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


FILES = ["--candidates", "c.txt", "--holes", "h.txt", "t.txt", "model", "train.txt"]


@pytest.mark.parametrize("args,msg", [
    (["design", "t.txt", "model", "train.txt"], "design needs --candidates FILE"),
    (["design", "--candidates", "c.txt", "t.txt", "model", "train.txt"], "design needs --candidates FILE"),
    (["--gpus", "2", "design", *FILES], "single-GPU context (gpak_create) only: drop --gpus"),
    (["--block-size", "1,1,1", "design", *FILES], "--block-size and --block-disc together"),
    (["--block-disc", "2,2,2", "design", *FILES], "--block-size and --block-disc together"),
    (["--pick", "x", "design", *FILES], "--pick takes the number of holes"),
    (["--pick", "-1", "design", *FILES], "--pick takes the number of holes"),
    (["design", "--candidates"], "--candidates takes a file"),
    (["design", "--candidates", "c.txt", "--holes"], "--holes takes a file of labels"),
    (["design", "--candidates", "c.txt", "--holes", "h.txt", "t.txt", "model"], "There are not enough input parameters"),
    (["design", "--bogus", *FILES], "Unknown flag"),
])
def test_cli_refuses_bad_design_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


def write_rows(path, rows):
    with open(path, "w") as f:
        f.write("# comment\n")
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")


@pytest.mark.parametrize("opts,cand_rows,cand_cols,labels,weights,msg", [
    ([], 10, 4, list(range(9)), None, "--holes: h.txt holds 9 labels for 10 candidate points"),
    ([], 10, 4, [0] * 9 + ["x"], None, "is not an integer label"),
    ([], 130, 4, [7] * 130, None, "--holes: hole 7 has more than 128 points"),
    ([], 10, 5, [0] * 10, None, "the candidate points need the targets' input columns"),
    (["--pick", "3"], 10, 4, [5] * 4 + [-2] * 6, None, "--pick: 3 holes to plan out of 2"),
    (["--weights", "w.txt"], 10, 4, [0] * 10, [1, 2, 3, 4], "--weights: w.txt holds 4 weights for 5 targets"),
    (["--weights", "w.txt"], 10, 4, [0] * 10, [1, 2, -3, 4, 5], "'-3' in w.txt is not a non-negative number"),
    (["--weights", "w.txt"], 10, 4, [0] * 10, [1, 2, "nan", 4, 5], "'nan' in w.txt is not a non-negative number"),
    (["--weights", "nowhere.txt"], 10, 4, [0] * 10, None, "nowhere.txt not readable"),
])
def test_cli_checks_the_design_before_a_context_exists(tmp_path, opts, cand_rows, cand_cols, labels, weights, msg):
    """Targets, candidates, labels (with the label code of `cv --groups`), weights and --pick are checked in the verb's
    own words; no model file exists here, so passing a check would fail on reading it -- after all of these."""
    build()
    write_rows(tmp_path / "t.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(5)])
    write_rows(tmp_path / "c.txt", [tuple(0.1 * i + c for c in range(cand_cols)) for i in range(cand_rows)])
    write_rows(tmp_path / "h.txt", [(v,) for v in labels])
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(10)])
    if weights is not None:
        write_rows(tmp_path / "w.txt", [(v,) for v in weights])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *opts, "design", "-np", *FILES], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode != 0 and msg in r.stderr.decode(), r.stderr.decode()


def test_cli_design_passes_its_checks_up_to_the_model(tmp_path):
    """The same files with nothing wrong: the verb gets as far as the model file, which is not there."""
    build()
    write_rows(tmp_path / "t.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(5)])
    write_rows(tmp_path / "c.txt", [(0.1 * i, 0.2 * i, 0.3 * i, 0) for i in range(10)])
    write_rows(tmp_path / "h.txt", [(v,) for v in [5] * 4 + [-2] * 6])
    write_rows(tmp_path / "w.txt", [(v,) for v in (1, 0, 2.5, 1e-3, 4)])
    write_rows(tmp_path / "train.txt", [(i, 2 * i, 3 * i, 0.5 * i) for i in range(10)])
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--pick", "2", "--weights", "w.txt", "--block-size", "1,1,1",
                        "--block-disc", "2,2,2", "design", "-np", *FILES], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode != 0 and "--" not in err and "model" in err, err
