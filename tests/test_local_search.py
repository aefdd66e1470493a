"""CPU tests (-m "not gpu") of the device neighbour search:

1. include/gpak_local_search.h and include/gpak_dev_local_search.h against the binding and the library;
2. both headers as C99, and the refusals that need no device;
3. the grids the kernel is run on alone (tests/local_search_ref.py) obey the invariants the kernel may assume and have the
   properties they were chosen for;
4. csrc/local_grid.h is plain C++;
5. the `--search` option of the command line: what it refuses, before a context exists.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, gpak

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_search_ref as sr  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
CSRC = os.path.join(ROOT, "gp_ss_ak_amd", "csrc")


# ---- 1. headers, binding, library ------------------------------------------------------------------------------------
def test_headers_binding_and_library_list_the_same_symbols():
    call, dev = header_functions("gpak_local_search.h"), header_functions("gpak_dev_local_search.h")
    assert call == sorted(_lib.LOCAL_SEARCH_SYMBOLS) == ["gpak_local_neighbours_dev"]
    assert dev == sorted(_lib.DEV_LOCAL_SEARCH_SYMBOLS) == ["gpak_dev_local_search"]
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert [h for h in headers if "gpak_local_neighbours_dev" in header_functions(h)] == ["gpak_local_search.h"]      # declared once
    assert [h for h in headers if "gpak_dev_local_search" in header_functions(h)] == ["gpak_dev_local_search.h"]
    for h in ("gpak.h", "gpak_local.h", "gpak_local_ok.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "gpak_local_neighbours_dev" not in text and "gpak_dev_local_search" not in text and "gpak_local_search" not in text, h
    assert header_functions("gpak_local.h") == sorted(_lib.LOCAL_SYMBOLS)                    # as it was
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in call + dev:
        assert hasattr(lib, name), name
    s = _lib.LocalSearchSummary()
    assert [n for n, _ in s._fields_] == ["grid_ms", "upload_ms", "search_ms", "centres", "cells", "visited", "batches", "max_used"]


def test_refusals_that_need_no_device():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.gpak_local_neighbours_dev.argtypes = [vp, vp, ctypes.c_long, i, vp, ctypes.c_long, vp, i, d, vp, vp, vp, vp]
    assert lib.gpak_local_neighbours_dev(None, None, 1, 3, None, 1, None, 1, 0.0, None, None, None, None) == gpak.EINVAL
    lib.gpak_dev_local_search.argtypes = [vp, vp, vp, vp, i, i, d, d, d, d, i, i, i, d, vp, i, i, d, vp, vp, vp, vp]
    assert lib.gpak_dev_local_search(None, None, None, None, 1, 3, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, 1.0, None, 1, 1, 0.0, None, None, None,
                                     None) == gpak.EINVAL


def test_headers_are_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_local_search.h"\n#include "gpak_dev_local_search.h"\n'
                   'int main(void){gpak_local_search_summary s; s.max_used = 0; s.visited = 0; (void)s; '
                   'if (gpak_dev_local_search(0, 0, 0, 0, 0, 3, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, 0.0, 0, 0, 1, 0.0, 0, 0, 0, 0) != GPAK_EINVAL) return 1; '
                   'return gpak_local_neighbours_dev(0, 0, 0, 3, 0, 0, 0, 1, 0.0, 0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


# ---- 3. the fixtures of the kernel's own test ------------------------------------------------------------------------
def test_kernel_grids_have_the_properties_they_are_chosen_for():
    most, cells, empty, outside = 0, [], [], set()
    for inputs in sr.KERNEL_INPUTS:
        for which in sr.KERNEL_GRIDS:
            Ts, Tc, G, g = sr.kernel_case(inputs, which)
            sr.check_grid(g, Ts)
            counts = np.diff(g["start"].astype(np.int64))
            most = max(most, int(counts.max()))
            cells.append(counts.size)
            empty.append(float((counts == 0).mean()))
            hi = g["lo"] + g["h"] * np.array(g["n"])
            for j in range(3):
                if np.any(Tc[:, j] < g["lo"][j]):
                    outside.add((j, -1))
                if np.any(Tc[:, j] > hi[j]):
                    outside.add((j, 1))
            assert np.any(np.abs(Tc).max(axis=1) >= 1e6)                                     # and one far away
    print(f"\nlargest cell {most} samples; cells {cells}; empty share {[round(e, 3) for e in empty]}")
    assert most >= 129 and 1 in cells and max(empty) > 0.9
    assert outside == {(j, s) for j in range(3) for s in (-1, 1)}


def test_grid_helper_bins_by_the_stated_rule():
    rng = np.random.default_rng(5)
    T = rng.random((300, 4)) * [3.0, 1.0, 0.2, 1.0]
    for h in (0.05, 0.31, 10.0):
        sr.check_grid(sr.grid(T, h), T)
    g = sr.grid(T, 0.31)
    assert g["n"] == [int(np.floor((T[:, j].max() - T[:, j].min()) / 0.31)) + 1 for j in range(3)]
    d2 = sr.dist2_lists(T, T[:2], np.array([[0, 5, -1], [1, -1, -1]]))
    assert d2[0, 0] == 0.0 and d2[1, 0] == 0.0 and d2[0, 2] == 0.0 and d2[0, 1] == (((T[5, 0] - T[0, 0]) ** 2 + (T[5, 1] - T[0, 1]) ** 2)
                                                                                  + (T[5, 2] - T[0, 2]) ** 2) + (T[5, 3] - T[0, 3]) ** 2


# ---- 4. the shared grid header ---------------------------------------------------------------------------------------
def test_grid_header_is_plain_cpp(tmp_path):
    text = open(os.path.join(CSRC, "local_grid.h")).read()
    assert "#include <hip" not in text and "gpak_internal.h" not in text and "namespace" in text
    host = open(os.path.join(CSRC, "local_search.cpp")).read()
    for definition in ("void transform_point(", "struct Grid {", "bool build_grid("):                # one owner
        assert definition in text and definition not in host
    assert '#include "local_grid.h"' in host and '#include "local_grid.h"' in open(os.path.join(CSRC, "local_search_dev.hip")).read()
    src = tmp_path / "g.cpp"
    src.write_text('#include "local_grid.h"\nint main() { gpak_local_grid::Grid g; const double X[6] = {0, 1, 0, 2, 0, 3};\n'
                   '  return gpak_local_grid::build_grid(X, 2, 3, nullptr, g) && g.ids.size() == 2 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src), "-o",
                           str(tmp_path / "g")])
    subprocess.check_call([str(tmp_path / "g")])


# ---- 5. the command line: everything is refused before a context exists (no model file is ever read) ------------------
def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


FILES = ["n.txt", "model", "train.txt"]


@pytest.mark.parametrize("args,msg", [
    (["--neighbours", "64", "--search", "gpu", "local", *FILES], "--search takes host or device"),
    (["--neighbours", "64", "--search", "", "local", *FILES], "--search takes host or device"),
    (["--search", "device", "test", *FILES], "--search is an option of the local verb"),
    (["--search", "host", "cv", "train.txt", "model"], "--search is an option of the local verb"),
    (["--neighbours", "64", "--radius", "1.5", "--octant", "8", "--search", "device", "local", *FILES],
     "--search device does not take --octant: the octant search runs on the host"),
    (["--search", "device", "local", *FILES], "local needs --neighbours k, the samples per node, between 1 and 128"),
])
def test_cli_refuses_bad_search_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


def test_cli_passes_its_checks_up_to_the_model(tmp_path):
    """--search device with nothing wrong: the verb gets as far as the model's files, which are not there."""
    build()
    for name in ("n.txt", "train.txt"):
        with open(tmp_path / name, "w") as f:
            for i in range(10):
                f.write(f"{i}\t{2 * i}\t{3 * i}\t{0.5 * i}\n")
    for search in ("device", "host"):
        r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "--neighbours", "8", "--radius", "2.5", "--search", search, "local", "-np",
                            *FILES], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = r.stderr.decode()
        assert r.returncode != 0 and "--" not in err and "model" in err, err


def test_help_names_the_option():
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), "local", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and "--search host|device" in r.stdout.decode()
