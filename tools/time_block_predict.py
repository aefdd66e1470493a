"""Block-support prediction at N = 32768, M = 16384 blocks, nd = 1, 8, 64 discretisation points: one JSON line.

Per nd: predict_ms of gpak_predict_block with the variance and with var = NULL (fill + mean only: the difference is the
substitution, the row sums and the blocks' own covariance), the fill's share, and the fill against its fp64-VALU floor --
nd * N * M kernel evaluations times the fp64 instruction slots per evaluation of the compiled kernel over the 39.3 T
lane-instructions/s of the device (1024 SIMDs x 16 fp64 lanes x 2.4 GHz, the rate DESIGN.md section 6 uses for the
Gram-matvec).  At nd = 8 also gpak_predict with the variance over the flattened M * nd points: the only route to a block
mean without this call (the same evaluations, eight times the substitution).

Usage: python tools/time_block_predict.py [N] [M]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_ss_ak_amd import gpak, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
M = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
# fp64 VALU instructions per kernel evaluation in the point loop of gpak_fillblk1_f64<GPAK_DIST_DIRECT, false>: 928 v_*_f64
# in a loop body of 32 evaluations (hipcc -save-temps, the loop that ends in the backward branch); the body's other 199
# vector instructions are 32-bit (table index, exponent, selects)
SLOTS_PER_EVAL = 29
VALU_F64_RATE = 39.3e12
DISC = {1: (1, 1, 1), 8: (2, 2, 2), 64: (4, 4, 4)}


def best(f, reps=3):
    out = []
    for _ in range(reps):
        f()
        out.append(g.timing()["predict_ms"])
    return min(out)


X, y = synth.drillholes(N)
g = gpak.Gpak(0)
g.set_train(X, y)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
g.logLikelihood()
centres = synth.test_points(M)
res = {"N": N, "M": M, "slots_per_eval": SLOTS_PER_EVAL, "valu_f64_lane_instr_per_s": VALU_F64_RATE, "nd": {}}
for nd, disc in DISC.items():
    Xd, n = gpak.block_points(centres, (0.02, 0.02, 0.01), disc)
    g.predict_block(Xd, nd)   # buffers
    with_var = best(lambda: g.predict_block(Xd, nd))
    mean_only = best(lambda: g.predict_block(Xd, nd, want_var=False))
    floor_ms = 1e3 * nd * float(N) * M * SLOTS_PER_EVAL / VALU_F64_RATE
    r = {"predict_ms": round(with_var, 3), "mean_only_ms": round(mean_only, 3), "fill_share": round(mean_only / with_var, 4),
         "fill_valu_floor_ms": round(floor_ms, 3), "fill_over_floor": round(mean_only / floor_ms, 3)}
    if nd == 8:
        g.posteriorMeanVar(Xd)
        r["flattened_predict_ms"] = round(best(lambda: g.posteriorMeanVar(Xd)), 3)
        r["flattened_over_block"] = round(r["flattened_predict_ms"] / with_var, 3)
    res["nd"][str(nd)] = r
g.close()
print(json.dumps(res))
