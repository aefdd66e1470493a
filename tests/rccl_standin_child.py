"""One case of tests/test_rccl_binding.py in a process of its own (the library's RCCL binding is process-wide): a rank
over the NumPy engine and the BUILT-IN transport, gpak_*_init_rccl against the stand-in GPAK_RCCL_LIB names, one JSON
line with what the calls returned.  python rccl_standin_child.py grid|dist CALLS"""
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gp_ss_ak_amd import dist as gd  # noqa: E402
from np_dist_engine import NumpyDistEngine  # noqa: E402


def main(kind, calls):
    lib = gd._load()
    eng = NumpyDistEngine()
    h = C.c_void_p()
    if kind == "grid":      # rank 1 of a 2 x 2 grid: pr = 1, pc = 0
        rc = lib.gpak_grid_create(C.byref(h), 1, 4, 2, 2, 0, C.byref(eng.table), None)
        init, last_error, destroy = lib.gpak_grid_init_rccl, lib.gpak_grid_last_error, lib.gpak_grid_destroy
    else:
        rc = lib.gpak_dist_create(C.byref(h), 1, 2, 0, C.byref(eng.table), None)
        init, last_error, destroy = lib.gpak_dist_init_rccl, lib.gpak_dist_last_error, lib.gpak_dist_destroy
    assert rc == 0, rc
    out = []
    for _ in range(calls):
        t0 = time.monotonic()
        rc = init(h, b"\x07" * 128)
        out.append({"rc": rc, "seconds": time.monotonic() - t0, "error": last_error(h).decode()})
    destroy(h)
    print(json.dumps(out), flush=True)
    os._exit(0)     # a helper thread the library abandoned may still sit in the stand-in's sleep: it ends here


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
