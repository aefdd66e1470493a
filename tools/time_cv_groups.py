"""Leave-group-out cross-validation at N = 8192 and N = 32768, holes of 128 and groups of 8: one JSON line.

Per size and grouping: ms of gpak_cv_groups and its split into the substitution for G = L^-T, the Gram pass and the solve
pass (the library keeps the split of the context's last call; no header declares that entry), with ms of gpak_loo on the
same context beside it.  The Gram pass is held against two floors: the bytes it must read -- the upper triangle of G from
each group's first 128-column tile on, 8 N^2 / 2 bytes -- at 5.5 TB/s, the rate the fill and the leave-one-out passes
reach; and its MFMA work, s N^2 flops for groups of s (the lower tiles alone: 36 of 64 at s = 128), at the device's fp64
MFMA rate of 78.6 TFLOP/s.

Usage: python tools/time_cv_groups.py [N ...]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_ss_ak_amd import gpak, synth  # noqa: E402

SIZES = [int(v) for v in sys.argv[1:]] or [8192, 32768]
HBM_RATE = 5.5e12
MFMA_F64_RATE = 78.6e12


def best(g, labels, reps=3):
    """The fastest of `reps` calls: (ms, [substitution, Gram, solve])."""
    out = []
    split = (C.c_double * 3)()
    for _ in range(reps):
        s = g.cv_groups(labels)[3]
        assert s["status"] == gpak.OK
        assert g._lib.gpak_cv_groups_last_split(g._h, split) == gpak.OK
        out.append((s["ms"], list(split)))
    return min(out)


res = {"hbm_bytes_per_s": HBM_RATE, "mfma_f64_flops_per_s": MFMA_F64_RATE, "N": {}}
for N in SIZES:
    X, y = synth.drillholes(N)
    g = gpak.Gpak(0)
    g.set_train(X, y)
    g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    g.logLikelihood()
    g.loo()
    loo_ms = min(g.loo()[2]["ms"] for _ in range(3))
    r = {"loo_ms": round(loo_ms, 3), "subst_flops": N ** 3 / 3.0}
    read_floor_ms = 1e3 * 8.0 * N * N / 2 / HBM_RATE
    for name, size in (("holes128", 128), ("groups8", 8)):
        labels = np.arange(N) // size
        g.cv_groups(labels)   # buffers, the LDS opt-in
        ms, (subst, gram, solve) = best(g, labels)
        mfma_floor_ms = 1e3 * size * float(N) * N * (36.0 / 64.0 if size == 128 else 1.0) / MFMA_F64_RATE
        r[name] = {"ms": round(ms, 3), "subst_ms": round(subst, 3), "gram_ms": round(gram, 3), "solve_ms": round(solve, 3),
                   "two_passes_over_subst": round((gram + solve) / subst, 4),
                   "gram_read_floor_ms": round(read_floor_ms, 3), "gram_fraction_of_hbm_rate": round(read_floor_ms / gram, 4),
                   "gram_mfma_floor_ms": round(mfma_floor_ms, 3), "gram_fraction_of_mfma_rate": round(mfma_floor_ms / gram, 4)}
    g.close()
    res["N"][str(N)] = r
print(json.dumps(res))
