"""The neighbour search on the device beside the host search, on the same inputs in the same process: writes
profiles/local_search.txt (one JSON record per line).  A report, not a gate.

Ns samples (synth.drillholes) and M centres (synth.test_points: a regular block model for a cube number).  Per
configuration (k, radius, G) the device call (gpak_local_neighbours_dev) and the host call (gpak_local_neighbours on 16
threads) alternate REPS times after one warm-up of each; per quantity the median and the spread (min, max):
  * grid_ms, upload_ms, search_ms of the device call's summary and its whole wall time (grid, uploads, copies included);
  * the host call's wall time, and the ratio of the two medians;
  * visited per centre, and visited / search_ms in samples per second beside the floor of 12 fp64 lane-instructions per
    candidate (3 differences, 3 products, 2 sums, the compares of the filter) over the device's 39.3 T
    lane-instructions/s;
  * that the two calls returned the same bytes.
For the configurations with the identity and radius 0, krige_ms of gpak_predict_local on the same lists follows, so that
the search's share of `local` can be read off.

Usage: python tools/time_local_search.py [Ns [M [reps [configuration indices, comma-separated]]]]
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
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
THREADS = 16
LANE_RATE = 39.3e12
SLOTS_PER_CANDIDATE = 12
ANISO = np.diag([1.0, 1.0, 4.0])         # the anisotropic diagonal: the vertical counts four times
RADIUS = 0.05
CONFIGS = [(k, r, name) for name in ("identity", "anisotropic") for r in (0.0, RADIUS) for k in (16, 64, 128)]
PICK = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else list(range(len(CONFIGS)))
out = open(os.path.join(ROOT, "profiles", "local_search.txt"), "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def med(v):
    return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]


Xs, ys = synth.drillholes(NS)
centres = synth.test_points(M)
g = gpak.Gpak(0)
g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
emit({"Ns": NS, "M": M, "reps": REPS, "threads": THREADS, "configurations": [CONFIGS[i] for i in PICK],
      "time": "median [min, max] of alternating calls after one warm-up each; wall times in ms"})
for i in PICK:
    k, radius, name = CONFIGS[i]
    G = None if name == "identity" else ANISO
    g.local_neighbours_dev(Xs, centres, k, G, radius)
    gpak.local_neighbours(Xs, centres, k, G, radius, THREADS)
    dev_wall, host_wall, parts = [], [], {"grid_ms": [], "upload_ms": [], "search_ms": []}
    for _ in range(REPS):
        t0 = time.perf_counter()
        nbr, used, _, s = g.local_neighbours_dev(Xs, centres, k, G, radius)
        dev_wall.append(1e3 * (time.perf_counter() - t0))
        for key in parts:
            parts[key].append(s[key])
        t0 = time.perf_counter()
        host, host_used = gpak.local_neighbours(Xs, centres, k, G, radius, THREADS)
        host_wall.append(1e3 * (time.perf_counter() - t0))
        print(f"k={k} radius={radius:g} {name}: device {dev_wall[-1]:.0f} ms, host {host_wall[-1]:.0f} ms", file=sys.stderr, flush=True)
    rate = s["visited"] / (float(np.median(parts["search_ms"])) * 1e-3)
    rec = {"k": k, "radius": radius, "G": name, "dev_wall_ms": med(dev_wall), "host_wall_ms": med(host_wall),
           "host_over_dev": round(float(np.median(host_wall) / np.median(dev_wall)), 2),
           "grid_ms": med(parts["grid_ms"]), "upload_ms": med(parts["upload_ms"]), "search_ms": med(parts["search_ms"]),
           "cells": s["cells"], "batches": s["batches"], "max_used": s["max_used"], "visited_per_centre": round(s["visited"] / M, 1),
           "samples_per_s": round(rate), "floor_samples_per_s": round(LANE_RATE / SLOTS_PER_CANDIDATE),
           "floor_over_measured": round(LANE_RATE / SLOTS_PER_CANDIDATE / rate, 1),
           "same_bytes": bool(nbr.tobytes() == host.tobytes() and used.tobytes() == host_used.tobytes())}
    if G is None and radius == 0.0:
        g.predict_local(Xs, ys, centres, 1, nbr)
        rec["krige_ms"] = med([g.predict_local(Xs, ys, centres, 1, nbr)[2]["krige_ms"] for _ in range(3)])
    emit(rec)
g.close()
out.close()
