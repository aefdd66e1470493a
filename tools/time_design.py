"""Infill drilling design at N = 32768: T = 4096 target blocks of nd = 8 points, 256 candidate holes of 64 points, a
round of scores (k = 0) and a greedy plan of k = 10: one JSON line.

Per phase, from the split the library keeps of the context's last call (no header declares that entry): the fills with
the transposition, the substitution over the stacked rows, the SYRK, the first score pass and one pick's downdate (X*,
the gather, U and P -= U U^T).  The score pass is held against two floors: the bytes of P_{I,.} it must read -- Mc T
doubles -- at the HBM rate gpak_calibrate measures on this device (the calibration bench.py uses), and its MFMA work,
2 T sum_h m_h^2 flops over the lower tiles of X alone (36 of 64 at m = 64: 10 of 16), at the fp64 MFMA rate the same
calibration measures.  The whole call stands beside what it replaces: one factorisation of N + m and one block prediction
per candidate hole and round, taken as factor_ms + the block path's predict_ms of this context at N.

Usage: python tools/time_design.py [N [T [holes [points]]]]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_ss_ak_amd import gpak, synth  # noqa: E402

args = [int(v) for v in sys.argv[1:]]
N, T, H, M = (args + [32768, 4096, 256, 64][len(args):])[:4]
ND, DISC, SIZE = 8, (2, 2, 2), (0.05, 0.05, 0.02)
PICKS = 10

X, y = synth.drillholes(N)
rng = np.random.default_rng(11)
centres = rng.uniform(-0.9, 0.9, (T, 3))
Xt, nd = gpak.block_points(centres, SIZE, DISC)
assert nd == ND
Xc = np.repeat(rng.uniform(-0.9, 0.9, (H, 3)), M, axis=0)
Xc[:, 2] = np.tile(0.9 - 1.8 / M * np.arange(M), H)
holes = np.repeat(np.arange(H), M)

g = gpak.Gpak(0)
tflops, gbs = g.calibrate()
g.set_train(X, y)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
g.logLikelihood()
factor_ms = g.timing()["factor_ms"]
g.predict_block(Xt, nd, latent=True)
block_ms = min((g.predict_block(Xt, nd, latent=True), g.timing()["predict_ms"])[1] for _ in range(3))


def best(k, reps=3):
    """the fastest of `reps` calls: (ms, [fills, substitution, SYRK, score, one downdate])"""
    out = []
    split = (C.c_double * 5)()
    for _ in range(reps):
        gain, picked, pick_gain, ex = g.design(Xt, nd, Xc, holes, None, k)
        assert ex["summary"]["status"] == gpak.OK
        assert g._lib.gpak_design_last_split(g._h, split) == gpak.OK
        out.append((ex["summary"]["ms"], list(split), ex["summary"]["var_before"], ex["summary"]["var_after"]))
    return min(out)


g.design(Xt, nd, Xc, holes, None, 1)      # buffers, the LDS opt-in
res = {"N": N, "T": T, "nd": nd, "holes": H, "points_per_hole": M, "hbm_gb_per_s": round(gbs, 1), "mfma_f64_tflops": round(tflops, 2),
       "factor_ms": round(factor_ms, 3), "block_predict_ms": round(block_ms, 3)}
for k in (0, PICKS):
    ms, (fill, subst, syrk, score, down), vb, va = best(k)
    read_floor = 1e3 * 8.0 * H * M * T / (gbs * 1e9)
    tiles = (M + 15) // 16
    mfma_floor = 1e3 * 2.0 * T * H * (tiles * (tiles + 1) / 2) * 256 / (tflops * 1e12)
    refit_ms = (factor_ms + block_ms) * H * max(k, 1)
    res[f"k{k}"] = {"ms": round(ms, 3), "fills_ms": round(fill, 3), "subst_ms": round(subst, 3), "syrk_ms": round(syrk, 3),
                    "score_ms": round(score, 3), "downdate_ms": round(down, 3),
                    "score_read_floor_ms": round(read_floor, 4), "score_fraction_of_hbm_rate": round(read_floor / score, 4),
                    "score_mfma_floor_ms": round(mfma_floor, 4), "score_fraction_of_mfma_rate": round(mfma_floor / score, 4),
                    "refits_replaced_ms": round(refit_ms, 1), "speedup_over_refits": round(refit_ms / ms, 1),
                    "var_before": vb, "var_after": va}
g.close()
print(json.dumps(res))
