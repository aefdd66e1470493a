"""Ordinary beside simple kriging in a moving neighbourhood, on the same node batch: writes profiles/local_ok.txt (one JSON
record per line).  A report, not a gate.

Ns samples (synth.drillholes) and M nodes (synth.test_points: a regular block model for a cube number), the default
composition, the neighbours searched once at k = 128 in the metric of its term (a prefix is the list of a smaller k).  Per
k = 16, 32, 64, 128 (one tier each) and nd = 1, 8, gpak_predict_local and gpak_predict_local_ok alternate REPS times after
one warm-up call each; the time is krige_ms, device events around the node batches (uploads, transform, kernel, copies
back: the kernel alone is not separable from outside the library).  Per estimator the median and the spread (min, max) are
written, and the ratio of the medians beside two models of it:
  * rows: the factorisation's fused multiply-adds alone, sum_j sum_{c > j} (s + x - c) = s^3 / 6 + x s^2 / 2 to leading
    order with x = 3 rows under the triangle instead of 2: (s + 9) / (s + 6);
  * lanes: the same with the fill in front of it, which ordinary kriging leaves unchanged -- s (s + 1) / 2 + s nd + nd^2
    kernel evaluations of 47 fp64 instructions (tools/time_local.py) -- so the ratio the whole kernel should show if it ran
    at the VALU rate.

Usage: python tools/time_local_ok.py [Ns [M [reps]]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import gpak, synth  # noqa: E402

NS = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SLOTS_PER_EVAL = 47
THREADS = 16
SIZE, DISC = (0.02, 0.02, 0.01), {1: (1, 1, 1), 8: (2, 2, 2)}
out = open(os.path.join(ROOT, "profiles", "local_ok.txt"), "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def fma_count(s, x):
    """fused multiply-adds of the right-looking factorisation over s + x rows (scalings left out)"""
    return sum((s - 1 - j) * (s + x) - (s * (s - 1) // 2 - j * (j + 1) // 2) for j in range(s))


Xs, ys = synth.drillholes(NS)
centres = synth.test_points(M)
g = gpak.Gpak(0)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
G = g.local_metric(0)
t0 = time.time()
full, used = gpak.local_neighbours(Xs, centres, 128, G, 0.0, THREADS)
emit({"Ns": NS, "M": M, "reps": REPS, "threads": THREADS, "search_k128_s": round(time.time() - t0, 3),
      "time": "krige_ms: device events around the node batches; median [min, max] of alternating calls"})
for nd in (1, 8):
    Xd, n = gpak.block_points(centres, SIZE, DISC[nd])
    for k in (16, 32, 64, 128):
        lists = np.ascontiguousarray(full[:, :k])
        g.predict_local(Xs, ys, Xd, nd, lists)                 # warm-up: both code objects and the LDS opt-in
        g.predict_local_ok(Xs, ys, Xd, nd, lists, want_mu=True)
        sk, ok = [], []
        for _ in range(REPS):
            sk.append(g.predict_local(Xs, ys, Xd, nd, lists)[2]["krige_ms"])
            mean, var, mu, s = g.predict_local_ok(Xs, ys, Xd, nd, lists, want_mu=True)
            ok.append(s["krige_ms"])
        evals = (k * (k + 1) / 2 + k * nd + nd * nd) * SLOTS_PER_EVAL
        f2, f3 = fma_count(k, 2), fma_count(k, 3)
        emit({"k": k, "nd": nd, "sk_ms": round(float(np.median(sk)), 3), "sk_spread": [round(min(sk), 3), round(max(sk), 3)],
              "ok_ms": round(float(np.median(ok)), 3), "ok_spread": [round(min(ok), 3), round(max(ok), 3)],
              "ok_over_sk": round(float(np.median(ok) / np.median(sk)), 4), "model_rows": round(f3 / f2, 4),
              "model_lanes": round((evals + f3) / (evals + f2), 4), "ok_nodes_per_s": round(M / (float(np.median(ok)) * 1e-3)),
              "batches": s["batches"], "notpd": s["notpd"], "empty": s["empty"], "mu_abs_max": float(np.abs(mu).max())})
g.close()
out.close()
