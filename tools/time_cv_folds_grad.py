"""grad_ms of gpak_cv_folds_grad beside gpak_cv_groups_grad and gpak_loo_grad at N = 8192 and 32768, alternating in ONE
process; the k refit exact-gradient evaluations the call replaces; and its own kernel, the wide column mix
(gpak_cvf_mix_f64 through gpak_dev_mix_cols), beside a composition of existing parts on the same operands.
Usage: python tools/time_cv_folds_grad.py [reps] table > profiles/cv_folds_grad.txt
       python tools/time_cv_folds_grad.py [reps] mix >> profiles/cv_folds_grad.txt      (a process of its own: torch first)

Written down beforehand (a model, nothing of it measured):
  * the matrix work is gpak_loo_grad's 5 N^3 / 3 (837 ms at N = 32768, profiles/r10_loo_grad.txt) plus gpak_cv_folds' pack /
    product / factor per group above 128 samples (146 ms for ten folds, profiles/cv_folds_times.json) plus the mix,
    2 Np m^2 flop per group: 7.3 TFLOP for ten random folds of 32768, 100 ms at the bulk GEMM's rate (~70 TFLOP/s).
    gpak_cvf_mix_f64 holds a 128 x 128 tile per workgroup as the bulk GEMM does, but reads its H operand straight from
    global memory into the MFMA layout, one 8-byte word per lane and k, with two waves per SIMD: expected at 50 - 70 % of
    the GEMM's rate, so 150 - 200 ms, and the whole call at 1.15 - 1.2 s for ten folds, ~1.35 s for five (the mix doubles),
    ~0.9 s for 164 holes of 200 (0.43 TFLOP of mix) and within 2 % of gpak_cv_groups_grad for 256 holes of which 8 hold 250.
  * N = 8192: loo_grad ~20 ms; ten folds add 0.11 TFLOP of mix (~3 ms) and the ten group sequences (~15 ms, launch bound).
  * ten refit exact-gradient evaluations on 0.9 N samples: ~2.5 s at N = 32768 by the flop model (N^3/3 factor + 5 N^3/3
    gradient each at 0.73 of the work), so the call should be about twice as fast as what it replaces.
  * the composition (a column gather into a dense Np x m_p operand, the bulk GEMM, a column scatter) moves 32 Np m bytes
    beside the product (3.4 GB, under 2 ms for a fold of 3277): it wins unless the fused kernel reaches the GEMM's rate.
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_ss_ak_amd import _lib, gpak, synth  # noqa: E402

SIZES = (8192, 32768)
E = np.array(synth.DEFAULT_EXPANS)


def random_folds(k):
    return lambda n: np.random.default_rng(1).permutation(n) % k


def holes_8_of_250(n):
    """n / 128 holes of consecutive samples, the first 8 of them 250 long (the others share the rest evenly: <= 128 each)."""
    k = n // 128
    sizes = np.full(k, (n - 8 * 250) // (k - 8))
    sizes[:8] = 250
    sizes[8:8 + n - sizes.sum()] += 1
    assert sizes.sum() == n and sizes[8:].max() <= 128
    return np.repeat(np.arange(k), sizes)


GROUPINGS = {"10-random-folds": random_folds(10), "5-random-folds": random_folds(5), "holes-of-200": lambda n: np.arange(n) // 200,
             "holes-8-of-250": holes_8_of_250}
REFIT_K = {"10-random-folds": 10, "5-random-folds": 5}


def context(N):
    X, y = synth.drillholes(N)
    g = gpak.Gpak(0)
    g.set_train(X, y)
    g.set_params(E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)
    return g, g.logLikelihood()


def med(v):
    return f"median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}"


def table(reps):
    for N in SIZES:
        g, nlz = context(N)
        small = np.arange(N) // 128
        g.loo_grad(), g.cv_groups_grad(small)               # workspaces, first-launch costs
        for name, make in GROUPINGS.items():
            labels = make(N)
            sizes = np.bincount(labels)
            g.cv_folds_grad(labels), g.cv_folds(labels)
            lgrad, ggrad, fgrad, folds = [], [], [], []
            for _ in range(reps):
                g.loo_grad()
                lgrad.append(g.timing()["grad_ms"])
                g.cv_groups_grad(small)
                ggrad.append(g.timing()["grad_ms"])
                _, s = g.cv_folds_grad(labels)
                fgrad.append(g.timing()["grad_ms"])
                folds.append(g.cv_folds(labels)[3]["ms"])
            mix_flop = 2.0 * ((N + 127) // 128 * 128) * float((sizes[sizes > 128].astype(float) ** 2).sum())
            print(f"N={N} {name}: nlZ={nlz:.9g} -log_pl={-s['log_pl']:.9g} groups={s['groups']} largest={s['max_size']} "
                  f"above128={int((sizes > 128).sum())} wide-mix={mix_flop / 1e12:.3f} TFLOP  ({reps} alternating repetitions, ms)")
            print(f"  gpak_loo_grad                   {med(lgrad)}")
            print(f"  gpak_cv_groups_grad (holes 128) {med(ggrad)}")
            print(f"  gpak_cv_folds (evaluate)        {med(folds)}")
            print(f"  gpak_cv_folds_grad              {med(fgrad)}")
            print(f"  cv_folds_grad - cv_groups_grad = {statistics.median(fgrad) - statistics.median(ggrad):.3f} ms, "
                  f"cv_folds_grad / loo_grad = {statistics.median(fgrad) / statistics.median(lgrad):.3f}", flush=True)
        g.close()
        # what the call replaces: k refits on N - N / k samples, each one factorisation and one exact gradient
        X, y = synth.drillholes(N)
        for name, k in REFIT_K.items():
            n = N - N // k
            r = gpak.Gpak(0)
            r.set_train(X[:n], y[:n])
            ts = []
            for rep in range(reps + 1):
                r.set_params(E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2 * (1.0 + 1e-3 * rep), gpak.DIST_DIRECT)
                t0 = time.perf_counter()
                r.logLikelihood()
                r.GradLL_exact()
                ts.append(1e3 * (time.perf_counter() - t0))
            r.close()
            ts = ts[1:]
            print(f"N={N} {name}: one refit evaluation (factor + gpak_grad_exact, {n} samples, wall clock) {med(ts)}; "
                  f"x {k} = {k * statistics.median(ts):.1f} ms", flush=True)


def mix_alone(reps):
    """gpak_dev_mix_cols beside gather + gpak_dev_update_rect (the bulk GEMM: C -= A B^T on zeroed C) + scatter, on the same
    random operands; times from events on the stream, medians of `reps` alternating repetitions."""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                      # torch holds the buffers: its HIP runtime comes up before the library's
    lib = _lib.load()
    lib.gpak_dev_update_rect.restype = C.c_int
    lib.gpak_dev_update_rect.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long,
                                         C.c_int, C.c_int, C.c_int]
    st = torch.cuda.current_stream().cuda_stream
    for N in SIZES:
        Np = (N + 127) // 128 * 128
        gen = torch.Generator(device=dev).manual_seed(N)
        H0 = torch.randn(Np * Np, dtype=torch.float64, device=dev, generator=gen)          # column-major, ld = Np
        H = H0.clone()
        for name, m, how in (("fold-of-N/10-scattered", N // 10 + 1, "scattered"), ("fold-of-N/5-scattered", N // 5 + 1, "scattered"),
                             ("hole-of-200-contiguous", 200, "contiguous"), ("hole-of-250-contiguous", 250, "contiguous")):
            mp = (m + 127) // 128 * 128
            rng = np.random.default_rng(m)
            cols_h = np.sort(rng.choice(N, m, replace=False)) if how == "scattered" else N // 3 + np.arange(m)
            cols = torch.from_numpy(cols_h.astype(np.int32)).to(dev)
            cols64 = cols.long()
            Q = torch.zeros(mp * mp, dtype=torch.float64, device=dev)
            Q.view(mp, mp)[:m, :m] = torch.randn(m, m, dtype=torch.float64, device=dev, generator=gen)   # view row r = column r: ld = mp
            Qt = Q.view(mp, mp).t().contiguous().view(-1)                                   # B[c, k] = Q[k, c], column-major
            Z = torch.empty(Np * mp, dtype=torch.float64, device=dev)
            A = torch.zeros(Np * mp, dtype=torch.float64, device=dev)
            Hm, Am, Zm = H.view(Np, Np), A.view(mp, Np), Z.view(mp, Np)                     # view row c = column c

            def fused():
                rc = lib.gpak_dev_mix_cols(st, H.data_ptr(), Np, Np, cols.data_ptr(), m, Q.data_ptr(), mp, Z.data_ptr(), Np)
                assert rc == 0

            def composed():
                torch.index_select(Hm, 0, cols64, out=Am[:m])                               # the column gather
                Z.zero_()
                rc = lib.gpak_dev_update_rect(st, A.data_ptr(), Np, Qt.data_ptr(), mp, mp, Z.data_ptr(), Np, Np, mp, 0)
                assert rc == 0
                Hm.index_copy_(0, cols64, Zm[:m])                                           # the column scatter, of -A B (C -= A B^T)

            times = {"fused": [], "composed": []}
            outs = {}
            for rep in range(reps + 1):
                for tag, fn in (("fused", fused), ("composed", composed)):
                    H.copy_(H0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    if rep:
                        times[tag].append(a.elapsed_time(b))
                    else:
                        outs[tag] = Hm.index_select(0, cols64).clone()
            gap = float((outs["fused"] + outs["composed"]).abs().max() / outs["composed"].abs().max())
            flop = 2.0 * Np * m * m
            mf, mc = statistics.median(times["fused"]), statistics.median(times["composed"])
            print(f"N={N} {name} m={m}: {flop / 1e9:.1f} GFLOP; the two agree within {gap:.2g} of the largest entry")
            print(f"  gpak_dev_mix_cols (mix + write-back)   {med(times['fused'])}  -> {flop / mf / 1e9:.1f} TFLOP/s")
            print(f"  gather + bulk GEMM + scatter           {med(times['composed'])}  -> {flop / mc / 1e9:.1f} TFLOP/s (issued "
                  f"{2.0 * Np * mp * mp / mc / 1e9:.1f})", flush=True)
            del Q, Qt, Z, A
        del H, H0


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2 and sys.argv[2] == "mix":
        mix_alone(reps)
    else:
        table(reps)
