"""grad_ms of gpak_cv_groups_grad beside gpak_loo_grad and gpak_grad_exact at N = 8192 and 32768, alternating in ONE
process, for holes of 128 samples and for groups of one sample; and the time of its two own kernels, the column mix
(gpak_cvg_mix_f64) and the weight-emitting solve pass (gpak_cvg_solve_f64<true>).
Usage: python tools/time_cv_groups_grad.py [reps] > profiles/cv_groups_grad.txt

Written down beforehand: the matrix work is gpak_loo_grad's 5 N^3 / 3 (N^3/3 for G = L^-T, N^3/3 for B^-1 = G G^T, N^3 for
H H^T) and one pair pass, so the call should land within a few percent of gpak_loo_grad on the same box (826 ms at
N = 32768, profiles/r10_loo_grad.txt), plus the two passes of gpak_cv_groups (5.7 ms at N = 32768 with holes of 128,
DESIGN.md section 4.4) and a mix of at most 512 N^2 flop that reads and writes N^2 doubles once each.

The two kernels have no timer of their own in the C-ABI: a fresh child (`python tools/time_cv_groups_grad.py run N LABELS`)
is started under `rocprofv3 --kernel-trace` and their dispatches are read from the trace.  The mix moves 16 Np N bytes
(every column of Kinv read once and written once) and issues 2 * 128^2 * Np * bins flop, zeros of the bins included."""
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
LABELS = {"holes128": lambda n: np.arange(n) // 128, "singletons": lambda n: np.arange(n)}
KERNELS = {"mix": ("gpak_cvg_mix_f64",), "solve+weights": ("gpak_cvg_solve_f64<true>", "gpak_cvg_solve_f64ILb1E")}


def context(N):
    X, y = synth.drillholes(N)
    g = gpak.Gpak(0)
    g.set_train(X, y)
    g.set_params(E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    return g, g.logLikelihood()


def run_child(N, name):
    """What the profiled child does: one warm call, three measured ones."""
    g, _ = context(N)
    labels = LABELS[name](N)
    for _ in range(4):
        g.cv_groups_grad(labels)
    g.close()


def table(reps):
    for N in SIZES:
        g, nlz = context(N)
        g.GradLL_exact(), g.loo_grad()               # workspaces, first-launch costs
        for name, make in LABELS.items():
            labels = make(N)
            g.cv_groups_grad(labels)
            exact, lgrad, ggrad = [], [], []
            for _ in range(reps):
                g.GradLL_exact()
                exact.append(g.timing()["grad_ms"])
                g.loo_grad()
                lgrad.append(g.timing()["grad_ms"])
                _, s = g.cv_groups_grad(labels)
                ggrad.append(g.timing()["grad_ms"])
            me, ml, mg = statistics.median(exact), statistics.median(lgrad), statistics.median(ggrad)
            print(f"N={N} {name} nlZ={nlz:.9g} -log_pl={-s['log_pl']:.9g} groups={s['groups']}  ({reps} alternating repetitions, ms)")
            print(f"  gpak_grad_exact      median {me:9.3f}  min {min(exact):9.3f}  max {max(exact):9.3f}")
            print(f"  gpak_loo_grad        median {ml:9.3f}  min {min(lgrad):9.3f}  max {max(lgrad):9.3f}")
            print(f"  gpak_cv_groups_grad  median {mg:9.3f}  min {min(ggrad):9.3f}  max {max(ggrad):9.3f}")
            print(f"  cv_groups_grad / loo_grad = {mg / ml:.3f}, cv_groups_grad - loo_grad = {mg - ml:.3f} ms", flush=True)
        g.close()


def kernels():
    for N in SIZES:
        Np = (N + 127) // 128 * 128
        for name, make in LABELS.items():
            sizes = np.bincount(make(N))
            bins, fill = 0, 0
            for s in sizes:                          # the greedy packing of gpak_cvg_pack_bins
                if bins == 0 or fill + s > 128:
                    bins, fill = bins + 1, 0
                fill += s
            with tempfile.TemporaryDirectory() as d:
                child = subprocess.run(["rocprofv3", "--output-format", "csv", "--kernel-trace", "-d", d, "-o", "kt", "--", sys.executable,
                                        os.path.abspath(__file__), "run", str(N), name], stdout=subprocess.DEVNULL,
                                       stderr=subprocess.PIPE, timeout=900)
                us = {k: [] for k in KERNELS}
                for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    for r in csv.DictReader(open(path)):
                        for k, needles in KERNELS.items():
                            if any(n in r["Kernel_Name"] for n in needles):
                                us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            us = {k: v[1:] for k, v in us.items()}   # the first dispatch is the warm call
            if child.returncode != 0 or not all(us.values()):
                sys.exit(f"N={N} {name}: the kernel trace lacks a dispatch of {[k for k, v in us.items() if not v]} (child status "
                         f"{child.returncode}); its stderr:\n{child.stderr.decode(errors='replace')[-2000:]}")
            mix, solve = min(us["mix"]), min(us["solve+weights"])
            nbytes, flop = 16.0 * Np * N, 2.0 * 128 * 128 * Np * bins
            print(f"N={N} {name}: {bins} bins; gpak_cvg_mix_f64 {len(us['mix'])} dispatches, min {mix:.1f} us median "
                  f"{statistics.median(us['mix']):.1f} us: {nbytes / 1e9:.3f} GB moved -> {nbytes / mix / 1e6:.2f} TB/s = "
                  f"{100 * nbytes / mix / 1e6 / FILL_TBS:.0f} % of the fill's {FILL_TBS} TB/s, {flop / 1e9:.1f} GFLOP issued -> "
                  f"{flop / mix / 1e6:.1f} TFLOP/s; gpak_cvg_solve_f64<true> min {solve:.1f} us median "
                  f"{statistics.median(us['solve+weights']):.1f} us", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "run":
        run_child(int(sys.argv[2]), sys.argv[3])
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
        kernels()
