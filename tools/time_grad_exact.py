"""grad_ms of gpak_grad (as written) and gpak_grad_exact at N = 8192 and 32768, alternating in ONE process, and the
exact-mode `train` at N = 32768 (4 iterations) through the command line.
Usage: python tools/time_grad_exact.py [reps] > profiles/r08_grad_exact.txt
Both gradients share the N^3 inverse (G = L^-T, B^-1 = G G^T); they differ in the pair pass and its host assembly only.
The A/A spread of gpak_grad itself (max - min of its own repetitions, as a share of their median) is the yardstick the
difference is read against."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import gpak, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
E = np.array(synth.DEFAULT_EXPANS)
g = gpak.Gpak(0)
for N in (8192, 32768):
    X, y = synth.drillholes(N)
    g.set_train(X, y)
    g.set_params(E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    nlz = g.logLikelihood()
    g.GradLL(), g.GradLL_exact()                 # workspaces, first-launch costs
    ref, exact = [], []
    for _ in range(REPS):
        g.GradLL()
        ref.append(g.timing()["grad_ms"])
        g.GradLL_exact()
        exact.append(g.timing()["grad_ms"])
    mr, me = statistics.median(ref), statistics.median(exact)
    spread = (max(ref) - min(ref)) / mr
    print(f"N={N} nlZ={nlz:.9g}  ({REPS} alternating repetitions, grad_ms)")
    print(f"  gpak_grad        median {mr:9.3f}  min {min(ref):9.3f}  max {max(ref):9.3f}   A/A spread {100 * spread:.2f} %")
    print(f"  gpak_grad_exact  median {me:9.3f}  min {min(exact):9.3f}  max {max(exact):9.3f}")
    print(f"  exact - as written: {me - mr:+.3f} ms = {100 * (me - mr) / mr:+.2f} % of the median (spread + 1 % = {100 * spread + 1:.2f} %)")
    print(f"  all  as written {[round(v, 3) for v in ref]}\n       exact      {[round(v, 3) for v in exact]}", flush=True)
g.close()

# the train verb in exact mode at N = 32768, 4 iterations
N, maxit = 32768, 4
X, y = synth.drillholes(N)
with tempfile.TemporaryDirectory() as d:
    with open(os.path.join(d, "train.txt"), "w") as f:
        for r, v in zip(X, y):
            f.write("\t".join(f"{t:.17g}" for t in list(r) + [v]) + "\n")
    env = dict(os.environ, GPAK_MAX_ITERS=str(maxit), GPAK_OPT_TRACE=os.path.join(d, "trace.txt"))
    for mode in ("exact", "reference"):
        if os.path.exists(env["GPAK_OPT_TRACE"]):
            os.remove(env["GPAK_OPT_TRACE"])
        subprocess.run([os.path.join(ROOT, "gp_ss_ak_amd", "host", "gp_ss_ak"), "-v", "1", "-np", "--gradient", mode, "--timing",
                        os.path.join(d, "timing.json"), "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS",
                        os.path.join(d, "train.txt"), os.path.join(d, "model")], env=env, cwd=d, check=True,
                       stdout=subprocess.DEVNULL, timeout=900)
        rows = [[float(v) for v in line.split()] for line in open(env["GPAK_OPT_TRACE"])]
        tim = json.load(open(os.path.join(d, "timing.json")))
        acc = tim["accumulated"]
        print(f"train N={N} --gradient {mode}, {maxit} iterations: optimiser evaluations {[int(r[2]) for r in rows]}, hot-path "
              f"evaluations {tim['evaluations']} (+ the model's own after the optimiser)")
        print(f"  kept objectives {[r[1] for r in rows]}")
        print(f"  accumulated ms: gram {acc['gram_ms']:.1f} factor {acc['factor_ms']:.1f} solve {acc['solve_ms']:.1f} nlz {acc['nlz_ms']:.1f}"
              f"; last grad_ms {tim['last']['grad_ms']:.1f}, last factor_ms {tim['last']['factor_ms']:.1f}", flush=True)
