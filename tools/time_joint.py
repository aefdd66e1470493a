"""Joint posterior of M blocks and conditional simulation at N = 32768, M = 4096 and 16384, nd = 1, 8, 27: one JSON line.

Per (M, nd), in one process:
  * predict_ms of gpak_predict_joint with the covariance, beside gpak_predict_block with the variance on the same blocks
    (the difference is the pair fill, the product W W' and the M^2-sized copy and mirror);
  * the pair fill alone (GPAK_JOINT_PRIOR: no substitution, no product) less the mean-only call, against its fp64-VALU
    floor -- nd^2 x (stored elements of the lower 128 x 64 tiles) evaluations x the fp64 instructions per evaluation of
    the compiled kernel over the 39.3 T lane-instructions/s of the device;
  * the product W W' (joint less prior less the block path's substitution share is not separable from outside: the
    figure given is joint - prior - (block with variance - block mean only), against the fp64 MFMA peak);
  * gpak_sample_joint at S = 128.
The calls that return a covariance include its copy to the host and the mirror (predict_ms covers the device part).

Usage: python tools/time_joint.py [N] [M ...]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_ss_ak_amd import gpak, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
MS = [int(v) for v in sys.argv[2:]] or [4096, 16384]
# fp64 VALU instructions per kernel evaluation in the a' loop of gpak_fillblk_pair_f64<1> on the exp(-sqrt(D2)) path:
# per evaluation one block of 27 v_*_f64 (distance in both forms, the select, the square root) and 20 of the block that
# holds the 32 exponentials of a column sweep (640 / 32), hipcc -S --cuda-device-only
SLOTS_PER_EVAL = 47
VALU_F64_RATE = 39.3e12
MFMA_F64_PEAK = 78.6e12
DISC = {1: (1, 1, 1), 8: (2, 2, 2), 27: (3, 3, 3)}
S = 128


def best(f, reps=3):
    out = []
    for _ in range(reps):
        f()
        out.append(g.timing()["predict_ms"])
    return min(out)


def stored_elements(M):
    """Elements of the lower 128 x 64 tiles (those that straddle the diagonal whole) of the padded matrix."""
    Mp = (M + 255) // 256 * 256
    return sum(128 * 64 for i in range(Mp // 128) for j in range(Mp // 64) if 128 * i + 128 > 64 * j)


X, y = synth.drillholes(N)
g = gpak.Gpak(0)
g.set_train(X, y)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
g.logLikelihood()
Np = (N + 127) // 128 * 128
res = {"N": N, "slots_per_eval": SLOTS_PER_EVAL, "valu_f64_lane_instr_per_s": VALU_F64_RATE, "cases": []}
for M in MS:
    centres = synth.test_points(M)
    xi = np.random.default_rng(M).standard_normal((M, S))
    Mp = (M + 255) // 256 * 256
    for nd, disc in DISC.items():
        Xd, n = gpak.block_points(centres, (0.02, 0.02, 0.01), disc)
        g.predict_joint(Xd, nd)   # buffers
        joint = best(lambda: g.predict_joint(Xd, nd))
        prior = best(lambda: g.predict_joint(Xd, nd, prior=True))
        mean_only = best(lambda: g.predict_joint(Xd, nd, want_cov=False))
        block = best(lambda: g.predict_block(Xd, nd))
        block_mean = best(lambda: g.predict_block(Xd, nd, want_var=False))
        sample = best(lambda: g.sample_joint(Xd, nd, xi, nugget=1e-8))
        fill_ms = prior - mean_only
        floor_ms = 1e3 * nd * nd * stored_elements(M) * SLOTS_PER_EVAL / VALU_F64_RATE
        syrk_ms = joint - prior - (block - block_mean)
        syrk_flops = 2.0 * Np * 128 * 128 * (Mp // 128) * (Mp // 128 + 1) / 2
        res["cases"].append({
            "M": M, "nd": nd, "joint_ms": round(joint, 3), "block_ms": round(block, 3), "joint_less_block_ms": round(joint - block, 3),
            "pair_fill_ms": round(fill_ms, 3), "pair_fill_valu_floor_ms": round(floor_ms, 3),
            "pair_fill_over_floor": round(fill_ms / floor_ms, 3), "syrk_ms": round(syrk_ms, 3),
            "syrk_of_mfma_peak": round(syrk_flops / (syrk_ms * 1e-3) / MFMA_F64_PEAK, 3) if syrk_ms > 0 else None,
            "sample_S128_ms": round(sample, 3)})
g.close()
print(json.dumps(res))
