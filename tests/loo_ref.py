"""NumPy restatement of leave-one-out cross-validation from one Cholesky factor (gpak_loo) and the brute-force refit it
is checked against.  TEST INFRASTRUCTURE, written independently of the device code.

With Ky = K + sn2 I = sn2 B, B = L L' and alpha = Ky^-1 y (Rasmussen & Williams, eq. 5.12):

  d_i   = [B^-1]_ii = sum_{k >= i} G_ik^2        G = L^-T (upper triangular)
  var_i = sn2 / d_i                               variance of y_i given all the other samples, noise included
  mu_i  = y_i - alpha_i var_i                     its mean

K is the full prior covariance of the samples: a White child is already on its diagonal (add_white).
"""
import math

import numpy as np


def add_white(K, white):
    """Kern_White adds its value where i == j of the same point set (as the CPU checker's gram_hyb does)."""
    return K + float(white) * np.eye(K.shape[0])


def loo(K, y, sn2):
    """Returns (mean, var) of every y_i given the others, from one factorisation of B = I + K / sn2."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float).ravel()
    N = K.shape[0]
    L = np.linalg.cholesky(np.eye(N) + K / sn2)
    G = np.linalg.solve(L, np.eye(N)).T
    d = np.sum(np.triu(G) ** 2, axis=1)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y / sn2))
    var = sn2 / d
    return y - alpha * var, var


def summary(y, mean, var):
    """The fields of gpak_loo_summary from their definitions."""
    y = np.asarray(y, dtype=float).ravel()
    r2 = (y - mean) ** 2
    return {"mse": float(np.mean(r2)), "mssr": float(np.mean(r2 / var)),
            "log_pl": float(np.sum(-0.5 * r2 / var - 0.5 * np.log(var) - 0.5 * math.log(2.0 * math.pi)))}


def refit(K, y, sn2, indices):
    """Brute force: for each i delete row and column i, solve the (N-1) system, predict y_i (noise included)."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float).ravel()
    N = K.shape[0]
    mean, var = [], []
    for i in indices:
        keep = np.arange(N) != i
        L = np.linalg.cholesky(K[np.ix_(keep, keep)] + sn2 * np.eye(N - 1))
        k = K[keep, i]
        v = np.linalg.solve(L, k)
        mean.append(float(v @ np.linalg.solve(L, y[keep])))
        var.append(float(K[i, i] + sn2 - v @ v))
    return np.array(mean), np.array(var)
