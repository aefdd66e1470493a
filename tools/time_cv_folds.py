"""k-fold cross-validation from the factor at N = 8192 and N = 32768, in one process: one JSON line.

Per size: gpak_cv_folds with 10 and with 5 random folds, best of 3 after a warm-up call, with the split the library keeps
of the context's last call (substitution for G = L^-T, batched small groups, pack, product, factor + inverse + finish; no
header declares that entry) and each pass against its floor:
  pack     the bytes of P written, 8 m_p (N_p - k0) per fold, at 5.5 TB/s (the rate the fill and the leave-one-out
           passes reach); what it reads is not in the floor
  product  the lower 128-tiles of S = P P^T, 2 * 128^2 * K flops each, at the fp64 MFMA rate of 78.6 TFLOP/s
  rest     the factorisation m_p^3 / 3 and the inverse m_p^3 / 3 at the same rate
At the largest size also:
  * 256 holes of 128 through gpak_cv_groups and through gpak_cv_folds, alternating, five calls each: the same kernels, so
    the two best times should agree within the spread of the gpak_cv_groups calls, which is recorded;
  * 256 holes of which 8 have 250 samples;
  * holes of 200 (one at a time every one of them): ms per group, and what 300 such groups would cost;
  * the refit baseline of the 10-fold case: per fold set_train on the kept samples + logLikelihood, counted as the
    factorisation alone (gpak_timing's factor_ms) and as wall time.

Usage: python tools/time_cv_folds.py [--out FILE] [N ...]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_ss_ak_amd import gpak, synth  # noqa: E402

ARGS = sys.argv[1:]
OUT = None
if "--out" in ARGS:
    OUT = ARGS[ARGS.index("--out") + 1]
    del ARGS[ARGS.index("--out"):ARGS.index("--out") + 2]
SIZES = [int(v) for v in ARGS] or [8192, 32768]
HBM_RATE = 5.5e12
MFMA_F64_RATE = 78.6e12
SPLIT = ("subst_ms", "batched_ms", "pack_ms", "product_ms", "rest_ms")


def set_defaults(g):
    g.set_params(np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, gpak.DIST_DIRECT)


def folds_call(g, labels):
    s = g.cv_folds(labels)[3]
    assert s["status"] == gpak.OK
    split = (C.c_double * 5)()
    assert g._lib.gpak_cv_folds_last_split(g._h, split) == gpak.OK
    return s["ms"], list(split)


def best(g, labels, reps=3):
    """The fastest of `reps` calls after a warm-up call: (ms, the five parts)."""
    folds_call(g, labels)
    return min(folds_call(g, labels) for _ in range(reps))


def floors(N, labels):
    """ms floors of the one-at-a-time groups of a labelling: pack, product, factor + inverse."""
    Np = (N + 127) // 128 * 128
    pack = prod = rest = 0.0
    for g in range(int(labels.max()) + 1):
        I = np.flatnonzero(labels == g)
        if I.size <= 128:
            continue
        mp, K = (I.size + 127) // 128 * 128, Np - int(I[0]) // 128 * 128
        mt = mp // 128
        pack += 8.0 * mp * K / HBM_RATE
        prod += mt * (mt + 1) / 2 * 2.0 * 128 * 128 * K / MFMA_F64_RATE
        rest += 2.0 * mp ** 3 / 3.0 / MFMA_F64_RATE
    return 1e3 * pack, 1e3 * prod, 1e3 * rest


def record(N, labels, ms, split):
    r = {"ms": round(ms, 3)}
    r.update({k: round(v, 3) for k, v in zip(SPLIT, split)})
    fl = floors(N, labels)
    for name, f, got in zip(("pack", "product", "rest"), fl, split[2:]):
        r[name + "_floor_ms"] = round(f, 3)
        r[name + "_fraction_of_floor_rate"] = round(f / got, 4) if got > 0 else None
    return r


res = {"hbm_bytes_per_s": HBM_RATE, "mfma_f64_flops_per_s": MFMA_F64_RATE, "N": {}}
for N in SIZES:
    X, y = synth.drillholes(N)
    g = gpak.Gpak(0)
    g.set_train(X, y)
    set_defaults(g)
    g.logLikelihood()
    r = {"subst_flops": N ** 3 / 3.0, "factor_ms": round(g.timing()["factor_ms"], 3)}
    fold_labels = {}
    for k in (10, 5):
        labels = np.random.default_rng(k).permutation(N) % k
        fold_labels[k] = labels
        r[f"folds{k}"] = record(N, labels, *best(g, labels))
    if N == max(SIZES):
        # 256 holes of 128 (N / 256 at another size): gpak_cv_groups against gpak_cv_folds, alternating
        holes = np.arange(N) // (N // 256)
        g.cv_groups(holes)
        g.cv_folds(holes)
        a, b = [], []
        for _ in range(5):
            a.append(g.cv_groups(holes)[3]["ms"])
            b.append(g.cv_folds(holes)[3]["ms"])
        r["holes256"] = {"cv_groups_ms": [round(v, 3) for v in a], "cv_folds_ms": [round(v, 3) for v in b],
                         "cv_groups_spread_ms": round(max(a) - min(a), 3), "best_difference_ms": round(min(b) - min(a), 3)}
        # 256 holes, 8 of them of 250 samples (every 32nd), 16 of 125 and 232 of 124 at N = 32768
        base = (N - 8 * 250) // 248
        sizes = np.full(256, base)
        sizes[::32] = 250
        left = N - int(sizes.sum())
        sizes[np.flatnonzero(sizes == base)[:left]] += 1
        mixed = np.repeat(np.arange(256), sizes)
        r["holes256_8_of_250"] = record(N, mixed, *best(g, mixed))
        # holes of 200: every group one at a time
        mid = np.arange(N) // 200
        ms, split = best(g, mid)
        n_mid = int(mid.max()) + 1
        r["holes200"] = dict(record(N, mid, ms, split), groups=n_mid, ms_per_group=round(sum(split[2:]) / n_mid, 4),
                             ms_for_300_groups=round(300 * sum(split[2:]) / n_mid, 2))
        # the refit baseline of the 10-fold case, on a context of its own
        labels = fold_labels[10]
        h = gpak.Gpak(0)
        refits = []
        for rep in range(4):                       # a warm-up round, then best of 3
            fac, t0 = 0.0, time.perf_counter()
            for f in range(10):
                keep = labels != f
                h.set_train(X[keep], y[keep])
                set_defaults(h)
                h.logLikelihood()
                fac += h.timing()["factor_ms"]
            refits.append((fac, 1e3 * (time.perf_counter() - t0)))
        h.close()
        fac, wall = min(refits[1:])
        r["refit10"] = {"factor_ms": round(fac, 3), "wall_ms": round(wall, 3),
                        "factor_over_cv_folds": round(fac / r["folds10"]["ms"], 3)}
    g.close()
    res["N"][str(N)] = r
line = json.dumps(res)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
