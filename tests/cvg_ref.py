"""NumPy restatement of leave-group-out cross-validation from one Cholesky factor (gpak_cv_groups) and the brute-force
refit it is checked against.  TEST INFRASTRUCTURE, written independently of the device code.

With Ky = K + sn2 I = sn2 B, B = L L', G = L^-T and alpha = Ky^-1 y (Rasmussen & Williams 5.4.2 in block form), for a group
with index set I of size s:

  S       = [B^-1]_II = G_I G_I' = R R'
  e_I     = sn2 S^-1 alpha_I,   mean_I = y_I - e_I
  Sigma_I = sn2 S^-1            covariance of y_I given every sample outside the group, noise included
  var_i   = [Sigma_I]_ii = sn2 sum_j (R^-1)_ji^2
  logp_g  = log N(y_I; mean_I, Sigma_I) = -1/2 alpha_I . e_I - 1/2 (s log sn2 - 2 sum_j log R_jj) - s/2 log 2 pi

K is the full prior covariance of the samples: a White child is already on its diagonal (loo_ref.add_white).  Groups are
given as integer labels 0 .. G - 1, one per sample; the members of a group are taken in ascending sample order.
"""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)


def members(group):
    group = np.asarray(group)
    return [np.flatnonzero(group == g) for g in range(int(group.max()) + 1)]


def cv_groups(K, y, sn2, group):
    """Returns (mean, var, logp, md): mean and var per sample, logp and md = e_I' Sigma_I^-1 e_I per group."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float).ravel()
    N = K.shape[0]
    L = np.linalg.cholesky(np.eye(N) + K / sn2)
    G = np.triu(np.linalg.solve(L, np.eye(N)).T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y / sn2))
    mean, var = np.zeros(N), np.zeros(N)
    logp, md = [], []
    for I in members(group):
        s = I.size
        GI = G[I]
        R = np.linalg.cholesky(GI @ GI.T)
        Ri = np.linalg.solve(R, np.eye(s))
        e = sn2 * (Ri.T @ (Ri @ alpha[I]))
        mean[I] = y[I] - e
        var[I] = sn2 * np.sum(Ri ** 2, axis=0)
        md.append(float(alpha[I] @ e))
        logp.append(-0.5 * md[-1] - 0.5 * (s * math.log(sn2) - 2.0 * float(np.sum(np.log(np.diag(R))))) - 0.5 * s * LOG2PI)
    return mean, var, np.array(logp), np.array(md)


def summary(y, mean, var, logp, md):
    """The four values of gpak_cv_groups_summary from their definitions."""
    y = np.asarray(y, dtype=float).ravel()
    r2 = (y - mean) ** 2
    return {"mse": float(np.mean(r2)), "mssr": float(np.mean(r2 / var)), "msmd": float(np.sum(md) / y.size),
            "log_pl": float(np.sum(logp))}


def refit(K, y, sn2, group, only=None):
    """Brute force: for each group delete its rows and columns, factor, predict the group jointly (noise included).
    Returns (mean, var, logp, md) like cv_groups; with `only` (a list of group numbers) for those groups alone: logp and
    md in that order, mean and var filled for their members and NaN elsewhere."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float).ravel()
    N = K.shape[0]
    mean, var = np.full(N, np.nan), np.full(N, np.nan)
    logp, md = [], []
    every = members(group)
    for I in (every if only is None else [every[int(g)] for g in only]):
        s = I.size
        keep = np.ones(N, dtype=bool)
        keep[I] = False
        C = K[np.ix_(I, I)] + sn2 * np.eye(s)
        m = np.zeros(s)
        if keep.any():
            L = np.linalg.cholesky(K[np.ix_(keep, keep)] + sn2 * np.eye(int(keep.sum())))
            V = np.linalg.solve(L, K[np.ix_(keep, I)])
            m = V.T @ np.linalg.solve(L, y[keep])
            C = C - V.T @ V
        C = 0.5 * (C + C.T)
        Lc = np.linalg.cholesky(C)
        z = np.linalg.solve(Lc, y[I] - m)
        mean[I] = m
        var[I] = np.diag(C)
        md.append(float(z @ z))
        logp.append(-0.5 * md[-1] - float(np.sum(np.log(np.diag(Lc)))) - 0.5 * s * LOG2PI)
    return mean, var, np.array(logp), np.array(md)


# ---- the groupings of the tests ---------------------------------------------------------------------------------------
def holes(N, size=128):
    return np.arange(N) // size


def random_groups(N, seed=0, about=37):
    rng = np.random.default_rng(seed)
    return rng.permutation(N) % int(math.ceil(N / about))


def singletons(N):
    return np.arange(N)


def mixed_sizes(N, sizes=(1, 2, 127, 128)):
    """Contiguous groups whose sizes cycle through `sizes`; the last group takes what is left."""
    out, g, k = np.zeros(N, dtype=int), 0, 0
    while k < N:
        s = min(sizes[g % len(sizes)], N - k)
        out[k:k + s] = g
        g, k = g + 1, k + s
    return out


def errors(y, got, want):
    """(mean relative to max|y|, variance per element, logp relative): the three figures every comparison bounds."""
    em = np.abs(got[0] - want[0]).max() / np.abs(y).max()
    ev = (np.abs(got[1] - want[1]) / np.abs(want[1])).max()
    el = (np.abs(got[2] - want[2]) / np.abs(want[2])).max()
    return em, ev, el
