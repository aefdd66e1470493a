"""TEST INFRASTRUCTURE: gpak_dev_pack_rows (include/gpak_dev_cv.h) alone on caller-owned device buffers, in a process of
its own (torch holds the buffers, and its HIP runtime must come up before the library's).  Buffers are allocated as
tests/dev_ops_cases.py's HipOps allocates them: guarded, skewed, sentinel-filled.  One JSON record per shape on stdout.

P is compared with NumPy indexing bit for bit (the operation is a copy); rows m .. m_p - 1 must be +0.0; the guard bands
and skew rows of P and every bit of G must come back as they went in.  Each shape runs twice: P 16-byte aligned with an
even leading dimension (the 16-byte stores), and an odd leading dimension (the 8-byte stores).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dev_ops_cases as dc  # noqa: E402

OK, EINVAL = 0, 2
# (id, Np, m, how the rows are chosen)
SHAPES = [("m=1", 640, 1, "scattered"), ("m=128", 640, 128, "contiguous"), ("m=129", 640, 129, "contiguous"),
          ("m=300-scattered", 640, 300, "scattered"), ("m=Np", 640, 640, "contiguous")]


def sentinel_mat(rows, cols, ld):
    P = dc.Mat(np.zeros((rows, cols)), ld=ld)
    P.full[...] = dc.sentinel(P.full.size)                    # the payload too: every element of P must be written
    P.before = P.data.copy()
    return P


def run(ops, name, Np, m, how):
    eng, lib = ops.eng, ops.lib
    rng = np.random.default_rng(m)
    rows = np.sort(rng.choice(Np, m, replace=False)) if how == "scattered" else (Np - m) // 2 + np.arange(m)
    rows = rows.astype(np.int32)
    k0 = int(rows[0]) // 128 * 128
    mp, ncols = (m + 127) // 128 * 128, Np - k0
    G = dc.Mat(rng.standard_normal((Np, Np)), ld=Np + 34)
    want = np.zeros((mp, ncols))
    want[:m] = G.was()[rows][:, k0:]
    dG, drows = eng.from_numpy(G.full), eng.from_numpy(rows)
    gp = dG.data_ptr() + 8 * dc.GUARD
    rec = {"name": name, "m": m, "mp": mp, "k0": k0, "ncols": ncols}
    for tag, ld in (("vec", mp + 32), ("scalar", mp + 33)):
        P = sentinel_mat(mp, ncols, ld)
        dP = eng.from_numpy(P.full)
        pp = dP.data_ptr() + 8 * dc.GUARD
        rcs = [lib.gpak_dev_pack_rows(eng._st(), gp, G.ld, Np, drows.data_ptr(), m, k0, pp, P.ld),
               lib.gpak_dev_pack_rows(eng._st(), gp, G.ld, Np, drows.data_ptr(), 0, k0, pp, P.ld),         # m < 1
               lib.gpak_dev_pack_rows(eng._st(), gp, G.ld, Np, drows.data_ptr(), m, Np, pp, P.ld),         # k0 outside
               lib.gpak_dev_pack_rows(eng._st(), gp, G.ld, Np, drows.data_ptr(), m, k0, pp, mp - 1)]       # ldp < m_p
        eng.sync()
        P.full[...] = dP.cpu().numpy()
        skew = ~P.lift(np.ones((mp, ncols), dtype=bool))
        rec[tag] = {"rc": rcs == [OK, EINVAL, EINVAL, EINVAL],
                    "copy": bool(np.array_equal(dc.bits(P.get()[:m]), dc.bits(want[:m]))),
                    "zero_rows": bool(np.all(dc.bits(P.get()[m:]) == 0)),
                    "guards": P.guards_ok(),
                    "skew_rows": bool(np.array_equal(dc.bits(P.data)[skew], dc.bits(P.before)[skew]))}
    G.full[...] = dG.cpu().numpy()
    rec["G_untouched"] = bool(G.guards_ok() and np.array_equal(dc.bits(G.data), dc.bits(G.before)))
    return rec


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_pack_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long]
    for shape in SHAPES:
        print(json.dumps(run(ops, *shape)), flush=True)


if __name__ == "__main__":
    main()
