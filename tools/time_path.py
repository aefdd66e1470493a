"""Simulation at any node count at N = 32768, S = 100 realisations: writes profiles/path.txt (one JSON record per line).

Two node sets: M = 65536 points, and M = 16384 blocks of 2 x 2 x 2 points.  For each, gpak_condition with the fused kernel
and with the comparison path (GPAK_COND_UNFUSED: averaged fill + GEMM), the fastest of three calls: the call's device
time and its split into the S solves and the product.  The fused product is held against two floors:
  VALU: M N nd evaluations at the general fill's 47 fp64 instructions each over 39.3 T lane-instructions/s;
  MFMA: 2 M N (S + 1) flops at the fp64 MFMA rate gpak_calibrate measures on this device (the calibration bench.py uses).
Then gpak_sample_path with 4096 frequencies on the same sets (the shares of the solves, of the prior and of the product),
and gpak_sample_joint at M = 16384 points, the one size both samplers can do.

Usage: python tools/time_path.py [N [S [features]]]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import gpak, synth  # noqa: E402

args = [int(v) for v in sys.argv[1:]]
N, S, F = (args + [32768, 100, 4096][len(args):])[:3]
VALU_RATE, FP64_PER_EVAL = 39.3e12, 47
SETS = [("points", 65536, 1, (1, 1, 1)), ("blocks 2x2x2", 16384, 8, (2, 2, 2))]
REPS = 3

X, y = synth.drillholes(N)
rng = np.random.default_rng(21)
g = gpak.Gpak(0)
tflops, gbs = g.calibrate()
g.set_train(X, y)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
g.logLikelihood()
out = open(os.path.join(ROOT, "profiles", "path.txt"), "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


emit({"N": N, "S": S, "features_per_term": F, "mfma_f64_tflops": round(tflops, 2), "hbm_gb_per_s": round(gbs, 1),
      "factor_ms": round(g.timing()["factor_ms"], 3), "valu_lane_instr_per_s": VALU_RATE, "fp64_instr_per_evaluation": FP64_PER_EVAL})


def best(fn):
    """the fastest of REPS calls by the call's device time: (predict_ms, summary)"""
    runs = []
    for _ in range(REPS):
        _Z, _mean, s = fn()
        assert s["status"] == gpak.OK
        runs.append((g.timing()["predict_ms"], s))
    return min(runs, key=lambda r: r[0])


Ysim = rng.standard_normal((N, S))
for name, M, nd, disc in SETS:
    centres = rng.uniform(-0.9, 0.9, (M, 3))
    Xd, n = gpak.block_points(centres, (0.05, 0.05, 0.02), disc)
    assert n == nd
    Fsim = rng.standard_normal((M, S))
    valu_ms = 1e3 * M * N * nd * FP64_PER_EVAL / VALU_RATE
    mfma_ms = 1e3 * 2.0 * M * N * (S + 1) / (tflops * 1e12)
    rec = {"nodes": name, "M": M, "nd": nd, "valu_floor_ms": round(valu_ms, 3), "mfma_floor_ms": round(mfma_ms, 3)}
    for label, unfused in (("fused", False), ("unfused", True)):
        g.condition(Xd, nd, Ysim, Fsim, unfused=unfused)                 # buffers
        ms, s = best(lambda: g.condition(Xd, nd, Ysim, Fsim, unfused=unfused))
        rec[label] = {"call_ms": round(ms, 3), "solve_ms": round(s["solve_ms"], 3), "product_ms": round(s["product_ms"], 3),
                      "batches": s["batches"], "solve_share": round(s["solve_ms"] / ms, 3)}
    p = rec["fused"]["product_ms"]
    rec["fused_over_unfused_product"] = round(p / rec["unfused"]["product_ms"], 3)
    rec["fused_product_over_valu_floor"] = round(p / valu_ms, 2)
    rec["fused_product_over_mfma_floor"] = round(p / mfma_ms, 2)
    rec["fused_product_over_sum_of_floors"] = round(p / (valu_ms + mfma_ms), 2)
    emit(rec)
    ft = np.zeros(F, dtype=np.int32)
    om = np.zeros((F, 4))
    om[:, :3] = rng.standard_normal((F, 3)) / np.abs(rng.standard_normal((F, 1)))
    ab, b0, E = rng.standard_normal((2 * F, S)), rng.standard_normal(S), rng.standard_normal((N, S))
    g.sample_path(Xd, nd, ft, om, ab, b0, E)
    ms, s = best(lambda: g.sample_path(Xd, nd, ft, om, ab, b0, E))
    emit({"nodes": name, "M": M, "nd": nd, "sample_path": {"call_ms": round(ms, 3), "solve_ms": round(s["solve_ms"], 3),
                                                             "prior_ms": round(s["prior_ms"], 3), "product_ms": round(s["product_ms"], 3),
                                                             "solve_share": round(s["solve_ms"] / ms, 3),
                                                             "prior_share": round(s["prior_ms"] / ms, 3),
                                                             "product_share": round(s["product_ms"] / ms, 3)}})

# the one size both samplers can do: M = 16384 points
M = 16384
Xd = rng.uniform(-0.9, 0.9, (M, 3))
xi = rng.standard_normal((M, S))
g.sample_joint(Xd, 1, xi, nugget=1e-8, latent=True)
joint_ms = min((g.sample_joint(Xd, 1, xi, nugget=1e-8, latent=True), g.timing()["predict_ms"])[1] for _ in range(2))
ft = np.zeros(F, dtype=np.int32)
om = np.zeros((F, 4))
om[:, :3] = rng.standard_normal((F, 3)) / np.abs(rng.standard_normal((F, 1)))
ab, b0, E = rng.standard_normal((2 * F, S)), rng.standard_normal(S), rng.standard_normal((N, S))
g.sample_path(Xd, 1, ft, om, ab, b0, E)
path_ms, s = best(lambda: g.sample_path(Xd, 1, ft, om, ab, b0, E))
emit({"nodes": "points", "M": M, "nd": 1, "sample_joint_ms": round(joint_ms, 3), "sample_path_ms": round(path_ms, 3),
      "joint_over_path": round(joint_ms / path_ms, 2)})
out.close()
g.close()
