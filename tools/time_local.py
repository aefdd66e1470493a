"""Moving-neighbourhood kriging on synthetic drill holes: writes profiles/local.txt (one JSON record per line).

Ns samples (synth.drillholes) and M nodes (synth.test_points: a regular block model for a cube number), the default
composition, the neighbours searched in the metric of its term.  Per k = 16, 32, 64, 128 (one tier each) and nd = 1, 8:
  * nodes per second of gpak_predict_local from krige_ms -- the node batches: uploads, transform, kernel and copies back
    (the kernel alone is not separable from outside the library) -- best of two calls;
  * that time over its fp64-VALU floor: per node s (s + 1) / 2 + s nd + nd^2 kernel evaluations, counted as
    tools/time_joint.py counts them (47 fp64 instructions each), plus the factorisation's s^3 / 3 and the substitutions'
    s^2 fused multiply-adds, over the 39.3 T lane-instructions/s of the device;
  * the search: gpak_local_neighbours at k = 64 and at k = 128 on 16 threads (the lists for smaller k are prefixes);
  * beside them gpak_predict_block of a context trained on a 32768-sample subsample, on the first M_cmp of the same nodes.

Usage: python tools/time_local.py [Ns [M [M_cmp]]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import gpak, synth  # noqa: E402

NS = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
M_CMP = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
N_GLOBAL = 32768
SLOTS_PER_EVAL = 47
VALU_F64_RATE = 39.3e12
THREADS = 16
SIZE, DISC = (0.02, 0.02, 0.01), {1: (1, 1, 1), 8: (2, 2, 2)}
out = open(os.path.join(ROOT, "profiles", "local.txt"), "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


Xs, ys = synth.drillholes(NS)
centres = synth.test_points(M)
g = gpak.Gpak(0)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
G = g.local_metric(0)
emit({"Ns": NS, "M": M, "threads": THREADS, "cpus": os.cpu_count(), "fp64_instr_per_evaluation": SLOTS_PER_EVAL,
      "valu_lane_instr_per_s": VALU_F64_RATE})
search = {}
for k in (64, 128):
    t0 = time.time()
    nbr, used = gpak.local_neighbours(Xs, centres, k, G, 0.0, THREADS)
    search[k] = time.time() - t0
    emit({"search_k": k, "seconds": round(search[k], 3), "centres_per_s": round(M / search[k])})
full = nbr                                                     # k = 128: ascending distance, so a prefix is the list of a smaller k
for nd in (1, 8):
    Xd, n = gpak.block_points(centres, SIZE, DISC[nd])
    for k in (16, 32, 64, 128):
        lists = np.ascontiguousarray(full[:, :k])
        best, summ = None, None
        for _ in range(2):
            mean, var, s = g.predict_local(Xs, ys, Xd, nd, lists)
            if best is None or s["krige_ms"] < best:
                best, summ = s["krige_ms"], s
        evals = k * (k + 1) / 2 + k * nd + nd * nd
        lane_instr = M * (evals * SLOTS_PER_EVAL + k ** 3 / 3.0 + k * k)
        floor_ms = lane_instr / VALU_F64_RATE * 1e3
        emit({"k": k, "nd": nd, "krige_ms": round(best, 2), "upload_ms": round(summ["upload_ms"], 2), "batches": summ["batches"],
              "nodes_per_s": round(M / (best * 1e-3)), "valu_floor_ms": round(floor_ms, 2), "krige_over_valu_floor": round(best / floor_ms, 1),
              "notpd": summ["notpd"], "empty": summ["empty"], "mean_abs_max": float(np.abs(mean).max()), "var_min": float(var.min())})
g.close()

# the global path beside it: a 32768-sample model on the first M_CMP of the same nodes
pick = np.random.default_rng(5).choice(NS, N_GLOBAL, replace=False) if NS > N_GLOBAL else np.arange(NS)
g = gpak.Gpak(0)
g.set_train(Xs[np.sort(pick)], ys[np.sort(pick)])
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
g.logLikelihood()
mc = min(M, M_CMP)
for nd in (1, 8):
    Xd, n = gpak.block_points(centres[:mc], SIZE, DISC[nd])
    times = []
    for _ in range(2):
        g.predict_block(Xd, nd)
        times.append(g.timing()["predict_ms"])
    emit({"predict_block_N": len(pick), "M": mc, "nd": nd, "predict_ms": round(min(times), 2), "nodes_per_s": round(mc / (min(times) * 1e-3))})
g.close()
out.close()
