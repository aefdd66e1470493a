"""TEST INFRASTRUCTURE: gpak_dev_kmm (include/gpak_dev_condition.h) alone on caller-owned device buffers, in a process of its
own (torch holds the buffers, and its HIP runtime must come up before the library's).  Buffers are tests/dev_ops_cases.py's
Mat: guarded, skewed, sentinel-filled; HipOps uploads them, runs, synchronises and downloads them again.  One JSON record
per case on stdout.

The points are transformed by gpak_dev_transform_k (the library's own transform: what the kernel is defined on); the
nodes' points go in POINT-MAJOR, and every pad block of the node buffer holds NaN coordinates, so a read past block
nB - 1 that reaches an output shows.  The reference is Kbar in long double (block_ref.block_cross) times A in long double.

Bound per element (the issue's): (FILL_TOL max|K| + (n_chain + 2) u max|Kbar|) sum_j |A_js| + u |F0|, n_chain = N products
and the adds of the slab sums = N + slabs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import block_ref  # noqa: E402
import dev_ops_cases as dc  # noqa: E402
import exact_grad_ref as xref  # noqa: E402

OK, EINVAL = 0, 2
DISC = {1: (1, 1, 1), 2: (1, 1, 2), 8: (2, 2, 2), 27: (3, 3, 3)}
SIZE = (0.1, 0.1, 0.05)
N_SLABS2 = 600           # 640 padded rows: a slab of 512 samples and one of 88
# (composition, M, S, nd, N, distance mode, F0 set)
CASES = [(c, 130, 17, 8, 300, 1, True) for c in ("defaults", "theta2", "d4-defaults", "d4-theta2", "expans+exp", "rbf",
                                                 "expans+rbf+bias+white")]
CASES += [("defaults", 1, 1, 1, 300, 1, True), ("defaults", 257, 128, 2, 300, 1, False), ("defaults", 130, 129, 27, 300, 1, True),
          ("defaults", 257, 17, 1, N_SLABS2, 1, True), ("expans+exp", 130, 129, 8, N_SLABS2, 1, False),
          ("defaults", 130, 17, 8, 300, 0, True), ("expans+rbf+bias+white", 257, 129, 2, 300, 0, False),
          ("d4-theta2", 1, 128, 27, 300, 0, True)]


def case_id(c):
    return f"{c[0]}-M{c[1]}-S{c[2]}-nd{c[3]}-N{c[4]}-{'direct' if c[5] else 'expansion'}-{'F0' if c[6] else 'noF0'}"


def comps():
    import test_block_gpu as tb
    return tb


def run(ops, case):
    tb = comps()
    comp, M, S, nd, N, mode, with_f0 = case
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, _y = tb.data(N, cols)
    X = np.asarray(X, dtype=np.float64)
    rng = np.random.default_rng(7000 + 13 * M + S + nd + N)
    centres = rng.uniform(X.min(axis=0), X.max(axis=0), (M, cols))
    Xd, _ = block_ref.block_points(centres, SIZE, DISC[nd])
    Xd[(M - 1) * nd] = X[5]                                       # distance 0 in the cross-kernel
    Np, cap = (N + 127) // 128 * 128, (M + 255) // 256 * 256
    kern = dc.serialise([(k, list(p)) for k, p in terms], white)
    dmode = mode | dc.HYB | (dc.D4 if cols == 4 else 0)
    mu = np.zeros(4)
    mu[:cols] = (X.sum(axis=0) + Xd.sum(axis=0)) / (N + M * nd)
    xs = np.zeros((4, Np))
    xs[:cols, :N] = X.T
    u = np.zeros(15 * Np)
    rcs = [ops.call("transform_k", xs.ravel(), Np, N, Np, kern, dmode, mu, u)]
    xp = np.zeros((4, nd * cap))
    xp[:cols] = np.nan                                             # the pad blocks: NaN coordinates
    for a in range(nd):
        xp[:cols, a * cap:a * cap + M] = Xd[a::nd].T
    P = np.zeros(15 * nd * cap)
    rcs.append(ops.call("transform_k", xp.ravel(), nd * cap, nd * cap, nd * cap, kern, dmode, mu, P))

    Kbar = block_ref.block_cross(X, Xd, nd, terms, bias)           # N x M, long double
    A0 = rng.standard_normal((N, S))
    F0v = rng.standard_normal((M, S)) if with_f0 else None
    want = Kbar.T @ A0.astype(dc.LD)
    if with_f0:
        want = want + F0v.astype(dc.LD)
    slabs = int(ops.lib.gpak_dev_kmm_slabs(N))
    kmax = float(np.abs(Kbar).max())                               # max|Kbar| <= max|K|: the smaller of the two for both
    bound = (dc.FILL_TOL[mode] * kmax + (N + slabs + 2) * dc.U * kmax) * np.abs(A0).sum(axis=0)[None, :] * np.ones((M, 1))
    if with_f0:
        bound = bound + dc.U * np.abs(F0v)
    outs, rec = [], {"name": case_id(case), "slabs": slabs, "slab_len": int(ops.lib.gpak_dev_kmm_slab_len(N))}
    for rep in range(2):                                           # the second call on fresh buffers: the same bytes
        A, Z = dc.Mat(A0, ld=N + 5), dc.Mat(np.zeros((M, S)), ld=M + 3)
        Z.full[...] = dc.sentinel(Z.full.size)
        Z.before = Z.data.copy()
        F0 = dc.Mat(F0v, ld=M + 7) if with_f0 else None
        scratch = dc.Mat(np.zeros(slabs * M * S))
        Pm, um = dc.Mat(P), dc.Mat(u)
        args = [Pm, cap, M, nd, um, Np, N, kern, bias, dmode, A, A.ld, S, F0, F0.ld if with_f0 else 0, Z, Z.ld, scratch]
        rc = ops.call("kmm", *args)
        outs.append(Z.data.copy())
        if rep:
            continue

        def bad(i, v):
            a = list(args)
            a[i] = v
            return ops.call("kmm", *a)
        refused = [bad(0, None), bad(4, None), bad(10, None), bad(15, None), bad(17, None), bad(2, 0), bad(3, 0), bad(6, 0),
                   bad(12, 0), bad(1, M - 1), bad(5, N - 1), bad(11, N - 1), bad(16, M - 1)]
        check = dc.Check("Z", Z, ref=want, bound=bound, cmp=np.ones((M, S), dtype=bool))
        ratio = check.ratio()
        A1 = A0.copy()                                             # the check bites: two samples' rows of A swapped
        A1[[0, N - 1]] = A1[[N - 1, 0]]
        wrong = Kbar.T @ A1.astype(dc.LD) + (F0v.astype(dc.LD) if with_f0 else 0)
        rec.update({"rc": rcs == [OK, OK] and rc == OK, "refused": refused == [EINVAL] * len(refused), "ratio": ratio,
                    "worst_error": float(np.abs(Z.get().astype(dc.LD) - want).max()),
                    "bites": dc.Check("Z", Z, ref=wrong, bound=bound, cmp=np.ones((M, S), dtype=bool)).ratio(),
                    "skew_untouched": check.violations() == 0,
                    "guards": bool(Z.guards_ok() and scratch.guards_ok()),
                    "inputs_untouched": bool(all(m.guards_ok() and np.array_equal(dc.bits(m.data), dc.bits(m.before))
                                                 for m in (A, Pm, um) + ((F0,) if with_f0 else ())))})
    rec["repeatable"] = bool(np.array_equal(dc.bits(outs[0]), dc.bits(outs[1])))
    return rec


def main():
    ops = dc.HipOps()
    dc.SIG["kmm"] = "piiipiihdipliplplp"
    for case in CASES:
        print(json.dumps(run(ops, case)), flush=True)


if __name__ == "__main__":
    main()
