"""The cases of the moving-neighbourhood tests: what tests/test_local.py (CPU) and tests/test_local_gpu.py share.  The inputs
and the references are computed once per process and returned read-only.

A case = (Ns samples, M nodes, nd points per node, composition of test_block_gpu.COMPS).  The samples are
test_block_gpu.data, the nodes test_block_gpu.blocks (point 0 of the last node sits exactly on sample 5; from nd = 2 on
point 1 of the first node repeats its point 0).  Node b is given the S[b mod 13] nearest samples of its centre (plain
Euclidean distance, by local_ref.brute_neighbours), S straddling every tile and tier edge, in a list padded to k = 128: one
call holds nodes of every size."""
import functools

import numpy as np

import local_ref
import test_block_gpu as tb

S = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
COMPS = ("defaults", "theta2", "d4-defaults", "expans+exp", "rbf", "expans+rbf+bias+white")
# Ns 300 and 513, M 37 and 130, nd 1 / 2 / 8 / 27 and the six compositions, every value of each at least once with both shapes
CASES = {
    "N300-M37-nd1-defaults": (300, 37, 1, "defaults"),
    "N513-M130-nd8-defaults": (513, 130, 8, "defaults"),
    "N300-M37-nd27-theta2": (300, 37, 27, "theta2"),
    "N513-M130-nd2-theta2": (513, 130, 2, "theta2"),
    "N300-M37-nd8-d4-defaults": (300, 37, 8, "d4-defaults"),
    "N513-M37-nd2-expans+exp": (513, 37, 2, "expans+exp"),
    "N300-M130-nd1-rbf": (300, 130, 1, "rbf"),
    "N513-M37-nd27-rbf": (513, 37, 27, "rbf"),
    "N300-M37-nd8-expans+rbf+bias+white": (300, 37, 8, "expans+rbf+bias+white"),
    "N513-M130-nd1-expans+rbf+bias+white": (513, 130, 1, "expans+rbf+bias+white"),
}
K = 128


def centres(Xd, nd):
    Xd = np.asarray(Xd)
    return Xd.reshape(Xd.shape[0] // nd, nd, Xd.shape[1]).mean(axis=1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(Xs, ys, Xd, nbr): nbr M x 128 int32, node b with S[b mod 13] entries"""
    Ns, M, nd, comp = CASES[name]
    cols = tb.COMPS[comp][0]
    Xs, ys = tb.data(Ns, cols)
    Xd = tb.blocks(Ns, cols, M, nd)
    full, _ = local_ref.brute_neighbours(Xs, centres(Xd, nd), K)
    nbr = full.copy()
    for b in range(M):
        nbr[b, S[b % len(S)]:] = -1
    nbr.setflags(write=False)
    return Xs, ys, Xd, nbr


@functools.lru_cache(maxsize=None)
def reference(name, dt=local_ref.LD):
    Ns, M, nd, comp = CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = inputs(name)
    out = local_ref.local_predict(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2, dt)
    for v in out.values():
        v.setflags(write=False)
    return out


def errors(comp, ys, mean, var, ref, key="var"):
    """(mean error over max|y|, variance error over the prior variance), as test_block_gpu scales them"""
    em = np.abs(np.asarray(mean, dtype=np.longdouble) - ref["mean"]).max() / np.abs(ys).max()
    ev = np.abs(np.asarray(var, dtype=np.longdouble) - ref[key]).max() / tb.prior_variance(comp)
    return float(em), float(ev)
