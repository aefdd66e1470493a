"""TEST INFRASTRUCTURE: the groupings and compositions of the k-fold tests (tests/test_cv_folds.py holds the NumPy
restatement tests/cvg_ref.py to brute-force refits on them, tests/test_cv_folds_gpu.py holds gpak_cv_folds to the
restatement).  Shapes: the smallest at which each path of csrc/cv_folds.hip can go wrong -- a group one sample above the
batched kernels' 128, groups of exactly two tiles and one over, members scattered over every row tile, N = 1 (mod 128), a
larger group in the reused workspaces before a smaller one, both paths in one call, and an S of three 512-column panels.
"""
import os
import sys

import numpy as np

from gp_ss_ak_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_grad_ref as xref  # noqa: E402

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
BOUND = 1e-8     # the project's bound
DEFAULTS = ([(xref.EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2)
WHITE = ([(xref.EXPANS, THETA2), (xref.RBF, [0.5, 0.9, 0.5])], 0.2, 0.1, 0.016)
RBF = ([(xref.RBF, [0.4, 1.3, 0.8])], 0.0, 0.0, 0.03)
SUMMARY = ("mse", "mssr", "msmd", "log_pl")


def contiguous(*sizes):
    """Labels 0, 1, ... for consecutive runs of the given sizes."""
    return lambda n: np.repeat(np.arange(len(sizes)), sizes)[:n]


def random_folds(k, seed=0):
    return lambda n: np.random.default_rng(seed).permutation(n) % k


# (id, N, input columns, grouping, (terms, bias, white, sn2))
CASES = [
    ("N200-129+71", 200, 3, contiguous(129, 71), DEFAULTS),
    ("N513-2-random-folds", 513, 3, random_folds(2), DEFAULTS),
    ("N700-256+257+187", 700, 3, contiguous(256, 257, 187), DEFAULTS),
    ("N1000-5-random-folds", 1000, 3, random_folds(5), DEFAULTS),
    ("N1000-1+128+129+300+442", 1000, 3, contiguous(1, 128, 129, 300, 442), DEFAULTS),
    ("N1000-442+300+129+128+1", 1000, 3, contiguous(442, 300, 129, 128, 1), DEFAULTS),
    ("N1100-i-mod-3", 1100, 3, lambda n: np.arange(n) % 3, DEFAULTS),
    ("N2000-1300+700", 2000, 3, contiguous(1300, 700), DEFAULTS),
    ("N300-d4-129+171", 300, 4, contiguous(129, 171), DEFAULTS),
    ("N513-2-folds-expans+rbf+bias+white", 513, 3, random_folds(2), WHITE),
    ("N700-rbf", 700, 3, contiguous(256, 257, 187), RBF),
]


def data(N, cols=3):
    return synth.drillholes4(N) if cols == 4 else synth.drillholes(N)
