"""The cases of the design tests (tests/test_design.py on the CPU, tests/test_design_gpu.py on the GPU): data, targets,
candidate holes and the long-double restatement of each, computed once per process.

Training data, target blocks and compositions are those of tests/test_block_gpu.py.  A layout is a list of hole sizes;
hole h is a vertical string of that many points 0.011 apart under a collar drawn inside the data's box.  Layout "sizes"
carries 1, 15, 16, 17, 127 and 128 points (the 127 and the 128 each straddle a 128-row tile boundary of the stack: the
candidates' rows 49..175 and 176..303) and two holes of 20 points whose points alternate in the list (not contiguous).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402

LD = np.longdouble
LAYOUTS = {
    "sizes": ([1, 15, 16, 17, 127, 128], 20),     # contiguous holes, then two interleaved holes of 20
    "six": ([9, 12, 7, 10, 11, 8], 0),
    "one": ([40], 0),
    "twins": ([9, 12, 7], -1),                    # -1: hole 3 repeats hole 1's points exactly (a tie, under a larger label)
}
# name -> (N, composition, T, nd, layout, picks)
CASES = {
    "N513-defaults-T130-nd8-sizes": (513, "defaults", 130, 8, "sizes", 3),
    "N200-theta2-T17-nd1-six": (200, "theta2", 17, 1, "six", 3),
    "N200-white-T257-nd8-six": (200, "expans+rbf+bias+white", 257, 8, "six", 2),
    "N200-d4-T1-nd8-six": (200, "d4-defaults", 1, 8, "six", 2),
    "N200-defaults-T17-nd1-one": (200, "defaults", 17, 1, "one", 1),
    "N200-defaults-T17-nd8-twins": (200, "defaults", 17, 8, "twins", 2),
}


@functools.lru_cache(maxsize=None)
def candidates(N, cols, layout):
    """(Xc, hole): the candidate points (F-order, read-only) and their labels 0 .. H - 1"""
    sizes, extra = LAYOUTS[layout]
    X, _ = tb.data(N, cols)
    rng = np.random.default_rng(7000 + N + 10 * cols + len(sizes))
    lo, hi = X.min(axis=0), X.max(axis=0)
    pts, lab = [], []

    def string(m):
        p = np.tile(rng.uniform(0.9 * lo, 0.9 * hi), (m, 1))
        p[:, 2] = 0.9 * hi[2] - 0.011 * np.arange(m)
        if cols == 4:
            p[:, 3] = rng.integers(0, 4, m) * (2.0 / 3.0) - 1.0
        return p
    for h, m in enumerate(sizes):
        pts.append(string(m))
        lab += [h] * m
    H = len(sizes)
    if extra > 0:
        a, b = string(extra), string(extra)
        pts.append(np.stack([a, b], axis=1).reshape(2 * extra, -1))
        lab += [H, H + 1] * extra
    elif extra < 0:
        pts.append(pts[1].copy())
        lab += [H] * sizes[1]
    Xc = np.asfortranarray(np.vstack(pts))
    Xc.setflags(write=False)
    hole = np.array(lab, dtype=np.int32)
    hole.setflags(write=False)
    return Xc, hole


def weights(T):
    """non-uniform weights with exact zeros (every third target from the second on)"""
    w = 0.5 + np.arange(T) % 5 / 4.0
    w[1::3] = 0.0
    return w


def inputs(name):
    N, comp, T, nd, layout, k = CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y = tb.data(N, cols)
    Xt = tb.blocks(N, cols, T, nd)
    Xc, hole = candidates(N, cols, layout)
    return X, y, Xt, Xc, hole


@functools.lru_cache(maxsize=None)
def stack(name, dt=LD):
    N, comp, T, nd, layout, k = CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = inputs(name)
    P = design_ref.stack_cov(X, Xt, nd, Xc, terms, bias, white, sn2, dt)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def reference(name, weighted=False, dt=LD):
    """design_ref.design of the case in dtype dt with the case's picks; the stack covariance is shared between the
    weighted and the unweighted plan"""
    N, comp, T, nd, layout, k = CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = inputs(name)
    return design_ref.design(X, Xt, nd, Xc, hole, terms, bias, white, sn2, wt=weights(T) if weighted else None, k=k, dt=dt,
                             P=stack(name, dt))
