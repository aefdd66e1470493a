"""grad_ms of gpak_loo_grad beside gpak_grad_exact and gpak_loo (its summary's ms) at N = 8192 and 32768, alternating in
ONE process, and the bandwidth of gpak_loo_mirror_scale_f64 against the fill's 5.4 TB/s.
Usage: python tools/time_loo_grad.py [reps] > profiles/r10_loo_grad.txt

The matrix work of gpak_loo_grad is N^3/3 (G = L^-T) + N^3/3 (B^-1 = G G^T) + N^3 (2 M = 2 H H^T) against the exact
gradient's 2 N^3 / 3; both run one pair pass.  gpak_loo alone is the first N^3/3.

The mirror kernel has no timer of its own in the C-ABI: a fresh child (`python tools/time_loo_grad.py run N`) is started
under `rocprofv3 --kernel-trace` and the kernel's dispatches are read from the trace.  Its traffic is the lower 64 x 64
tiles of B^-1 read once and all of H written once: 8 (Np (Np + 64) / 2 + Np^2) bytes."""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import gpak, synth  # noqa: E402

FILL_TBS = 5.4
SIZES = (8192, 32768)
E = np.array(synth.DEFAULT_EXPANS)


def context(N):
    X, y = synth.drillholes(N)
    g = gpak.Gpak(0)
    g.set_train(X, y)
    g.set_params(E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    return g, g.logLikelihood()


def run_child(N):
    """What the profiled child does: one warm call, three measured ones."""
    g, _ = context(N)
    for _ in range(4):
        g.loo_grad()
    g.close()


def table(reps):
    for N in SIZES:
        g, nlz = context(N)
        g.GradLL_exact(), g.loo_grad(), g.loo()      # workspaces, first-launch costs
        exact, lgrad, loo = [], [], []
        for _ in range(reps):
            g.GradLL_exact()
            exact.append(g.timing()["grad_ms"])
            _, s = g.loo_grad()
            lgrad.append(g.timing()["grad_ms"])
            loo.append(g.loo()[2]["ms"])
        me, ml, mo = statistics.median(exact), statistics.median(lgrad), statistics.median(loo)
        print(f"N={N} nlZ={nlz:.9g} -log_pl={-s['log_pl']:.9g}  ({reps} alternating repetitions, ms)")
        print(f"  gpak_grad_exact  median {me:9.3f}  min {min(exact):9.3f}  max {max(exact):9.3f}")
        print(f"  gpak_loo_grad    median {ml:9.3f}  min {min(lgrad):9.3f}  max {max(lgrad):9.3f}")
        print(f"  gpak_loo         median {mo:9.3f}  min {min(loo):9.3f}  max {max(loo):9.3f}")
        print(f"  loo_grad / grad_exact = {ml / me:.3f} (matrix flops: 5/3 N^3 against 2/3 N^3 = 2.5, one pair pass each)", flush=True)
        g.close()


def mirror():
    for N in SIZES:
        Np = (N + 127) // 128 * 128
        nbytes = 8.0 * (Np * (Np + 64) / 2 + float(Np) * Np)
        with tempfile.TemporaryDirectory() as d:
            child = subprocess.run(["rocprofv3", "--output-format", "csv", "--kernel-trace", "-d", d, "-o", "kt", "--", sys.executable,
                                    os.path.abspath(__file__), "run", str(N)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                   timeout=600)
            us = []
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(path)):
                    if "gpak_loo_mirror_scale_f64" in r["Kernel_Name"]:
                        us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        us = us[1:]                                  # the first dispatch is the warm call
        if child.returncode != 0 or not us:
            sys.exit(f"N={N}: no dispatch of gpak_loo_mirror_scale_f64 in the kernel trace (child status {child.returncode}); "
                     f"its stderr:\n{child.stderr.decode(errors='replace')[-2000:]}")
        best = min(us)
        print(f"N={N} gpak_loo_mirror_scale_f64: {len(us)} dispatches, min {best:.1f} us median {statistics.median(us):.1f} us; "
              f"{nbytes / 1e9:.3f} GB moved -> {nbytes / best / 1e6:.2f} TB/s = {100 * nbytes / best / 1e6 / FILL_TBS:.0f} % of the "
              f"fill's {FILL_TBS} TB/s", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "run":
        run_child(int(sys.argv[2]))
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
        mirror()
