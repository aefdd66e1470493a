"""TEST INFRASTRUCTURE: gpak_dev_mix_cols (include/gpak_dev_cv_mix.h) alone on caller-owned device buffers, in a process
of its own (torch holds the buffers, and its HIP runtime must come up before the library's).  Buffers are allocated as
tests/dev_ops_cases.py's HipOps allocates them: guarded, skewed, sentinel-filled.  One JSON record per shape on stdout.

The mixed columns H[:, cols] are held against the long-double product (dev_ops_cases.mm_ld) of the columns as they went in
and Q, within (m + 2) 2^-53 (|H[:, cols]| |Q|) element by element: the rule of dev_ops_cases.gemm_expect for a chain of m
terms.  Every other column of H, every bit of Q and of cols, and the guard bands and skew rows of H, Q and Z must come
back as they went in (of Z's payload nothing is promised).  A second call on fresh copies must return the same bytes.
Each shape runs with even ldq / ldz and with odd ones.  "bites": the same comparison against a reference in which two
entries of cols were swapped must miss the bound by orders of magnitude -- the bound is not slack enough to hide a wrong
column.
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
NP = 640
# (id, m, how the columns are chosen)
SHAPES = [("m=1", 1, "scattered"), ("m=128", 128, "contiguous"), ("m=129", 129, "contiguous"),
          ("m=256", 256, "contiguous"), ("m=257", 257, "contiguous"), ("m=300-scattered", 300, "scattered"),
          ("m=Np", NP, "contiguous")]


def columns(m, how, rng):
    if how == "contiguous":
        return ((NP - m) // 2 + np.arange(m)).astype(np.int32)
    # scattered over every 128-row tile of the column range: as many per tile as m allows, the rest at random
    tiles = np.arange(NP) // 128
    pick = [rng.choice(np.flatnonzero(tiles == t)) for t in range(NP // 128)][:m]
    rest = np.setdiff1d(np.arange(NP), pick)
    pick = np.concatenate([pick, rng.choice(rest, m - len(pick), replace=False)]).astype(np.int64)
    return np.sort(pick).astype(np.int32)


def run(ops, name, m, how):
    eng, lib = ops.eng, ops.lib
    rng = np.random.default_rng(1000 + m)
    cols = columns(m, how, rng)
    mp = (m + 127) // 128 * 128
    H0 = rng.standard_normal((NP, NP))
    Q0 = rng.standard_normal((m, m))
    Hc = H0[:, cols]
    ref = dc.mm_ld(Hc, np.ascontiguousarray(Q0.T))                      # Hc @ Q0 in long double
    bound = (m + 2) * dc.U * (np.abs(Hc) @ np.abs(Q0))
    rec = {"name": name, "m": m, "mp": mp, "tiles_hit": int(np.unique(cols // 128).size)}
    mixed = np.zeros((NP, NP), dtype=bool)
    mixed[:, cols] = True
    for tag, ldq, ldz in (("even", m + 32 + (m & 1), NP + 34), ("odd", m + 33 + (m & 1), NP + 33)):
        outs = []
        for rep in range(2):                                           # the second call on fresh copies: the same bytes
            H, Q = dc.Mat(H0, ld=NP + 34), dc.Mat(Q0, ld=ldq)
            Z = dc.Mat(np.zeros((NP, mp)), ld=ldz)
            Z.full[...] = dc.sentinel(Z.full.size)
            Z.before = Z.data.copy()
            dH, dQ, dZ, dcols = eng.from_numpy(H.full), eng.from_numpy(Q.full), eng.from_numpy(Z.full), eng.from_numpy(cols)
            hp, qp, zp = (t.data_ptr() + 8 * dc.GUARD for t in (dH, dQ, dZ))
            st = eng._st()
            rcs = [lib.gpak_dev_mix_cols(st, hp, H.ld, NP, dcols.data_ptr(), m, qp, Q.ld, zp, Z.ld)]
            if rep == 0:
                rcs += [lib.gpak_dev_mix_cols(st, hp, H.ld, NP, dcols.data_ptr(), 0, qp, Q.ld, zp, Z.ld),         # m < 1
                        lib.gpak_dev_mix_cols(st, hp, H.ld, NP, dcols.data_ptr(), NP + 1, qp, Q.ld, zp, Z.ld),    # m > Np
                        lib.gpak_dev_mix_cols(st, hp, NP - 1, NP, dcols.data_ptr(), m, qp, Q.ld, zp, Z.ld),       # ld < Np
                        lib.gpak_dev_mix_cols(st, hp, H.ld, NP, dcols.data_ptr(), m, qp, m - 1, zp, Z.ld),        # ldq < m
                        lib.gpak_dev_mix_cols(st, hp, H.ld, NP, dcols.data_ptr(), m, qp, Q.ld, zp, NP - 1)]       # ldz < Np
            eng.sync()
            H.full[...], Q.full[...], Z.full[...] = dH.cpu().numpy(), dQ.cpu().numpy(), dZ.cpu().numpy()
            outs.append(H.data.copy())
            if rep:
                continue
            full_ref, full_bound = np.zeros((NP, NP), dtype=dc.LD), np.ones((NP, NP))
            full_ref[:, cols], full_bound[:, cols] = ref, bound
            chk = dc.Check("H", H, ref=full_ref, bound=full_bound, cmp=mixed)
            zskew = ~Z.lift(np.ones((NP, mp), dtype=bool))
            r = {"rc": rcs == [OK] + [EINVAL] * 5,
                 "ratio": chk.ratio(),
                 "other_columns_and_skew_rows": chk.violations() == 0,
                 "H_guards": H.guards_ok(),
                 "Q_untouched": bool(Q.guards_ok() and np.array_equal(dc.bits(Q.data), dc.bits(Q.before))),
                 "Z_guards": Z.guards_ok(),
                 "Z_skew_rows": bool(np.array_equal(dc.bits(Z.data)[zskew], dc.bits(Z.before)[zskew])),
                 "cols_untouched": bool(np.array_equal(dcols.cpu().numpy(), cols))}
            if m >= 2 and "bites" not in rec:                           # two columns of the reference swapped
                wrong = full_ref.copy()
                a, b = int(cols[0]), int(cols[-1])
                wrong[:, [a, b]] = full_ref[:, [b, a]]
                rec["bites"] = dc.Check("H", H, ref=wrong, bound=full_bound, cmp=mixed).ratio()
            rec[tag] = r
        rec[tag]["repeatable"] = bool(np.array_equal(dc.bits(outs[0]), dc.bits(outs[1])))
        rec[tag]["ldq"], rec[tag]["ldz"] = ldq, ldz
    return rec


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_mix_cols
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    for shape in SHAPES:
        print(json.dumps(run(ops, *shape)), flush=True)


if __name__ == "__main__":
    main()
