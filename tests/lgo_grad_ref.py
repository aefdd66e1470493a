"""NumPy restatement of the gradient of the leave-group-out criterion (gpak_cv_groups_grad).  TEST INFRASTRUCTURE, written
independently of the device code.

With Ky = K + sn2 I, Kinv = Ky^-1, alpha = Kinv y and, for a group with index set I, S = sn2 [Kinv]_II and
e_I = y_I - mean_I = sn2 S^-1 alpha_I (cvg_ref.py), the objective is

  F = -log_pl = sum_g [ 1/2 alpha_I . e_I - 1/2 log |S / sn2| ] + N/2 log 2 pi

and dF / d theta = 1/2 sum_ij W_ij d(Ky)_ij / d theta with

  C = blockdiag(C_I),  C_I = sn2 S^-1 + e_I e_I',   v = Kinv e,
  W = Kinv C Kinv - v alpha' - alpha v'

(from d alpha = -Kinv dK alpha and d(Kinv)_II = -[Kinv dK Kinv]_II).  W is symmetric, so exact_grad_ref.grad_exact, which
contracts any weight matrix with the full dK / d theta matrices, returns the gradient in gpak_grad_exact's layout.  With
groups of one sample W is loo_grad_ref's.  tests/test_cv_groups_grad.py checks this file against central differences of
cvg_ref's log_pl.

The "cholesky" route goes the device's way: S = R R', X = R^-1, w = X alpha_I and the closed-form factor
  Q_I = sqrt(sn2) X' + (beta / sqrt(sn2)) e_I w',   beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)),   Q_I Q_I' = C_I,
so that W = H H' - v alpha' - alpha v' with H[:, I] = Kinv[:, I] Q_I.  The "inv" route uses np.linalg.inv throughout and
forms C_I directly, without Q.
"""
import numpy as np

import cvg_ref
import exact_grad_ref as xref

BIN = 128


def closed_form_q(S, alpha_I, sn2):
    """(Q_I, C_I, e_I) of one group from its S = sn2 [Kinv]_II: Q by the closed form, C from its definition."""
    s = S.shape[0]
    R = np.linalg.cholesky(S)
    X = np.linalg.solve(R, np.eye(s))
    w = X @ alpha_I
    e = sn2 * (X.T @ w)
    beta = sn2 / (1.0 + np.sqrt(1.0 + sn2 * float(w @ w)))
    Q = np.sqrt(sn2) * X.T + (beta / np.sqrt(sn2)) * np.outer(e, w)
    C = sn2 * (X.T @ X) + np.outer(e, e)
    return Q, C, e


def weights(K, y, sn2, labels, route="cholesky"):
    """W of the grouped criterion.  route: "cholesky" (one factor and the closed-form Q, as the device) or "inv"
    (np.linalg.inv for every inverse and C_I formed directly: a second float64 route to the same matrix)."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float).ravel()
    N = K.shape[0]
    Ky = K + sn2 * np.eye(N)
    if route == "cholesky":
        L = np.linalg.cholesky(Ky)
        Li = np.linalg.solve(L, np.eye(N))
        Kinv = Li.T @ Li
    else:
        Kinv = np.linalg.inv(Ky)
    alpha = Kinv @ y
    e = np.zeros(N)
    M = np.zeros((N, N))
    if route == "cholesky":
        H = np.zeros((N, N))
        for I in cvg_ref.members(labels):
            Q, _, e[I] = closed_form_q(sn2 * Kinv[np.ix_(I, I)], alpha[I], sn2)
            H[:, I] = Kinv[:, I] @ Q
        M = H @ H.T
    else:
        for I in cvg_ref.members(labels):
            P = np.linalg.inv(Kinv[np.ix_(I, I)])          # sn2 S^-1
            e[I] = P @ alpha[I]
            M += Kinv[:, I] @ (P + np.outer(e[I], e[I])) @ Kinv[I, :]
    v = Kinv @ e
    return M - np.outer(v, alpha) - np.outer(alpha, v)


def grad_lgo(X, y, terms, bias, sn2, labels, route="cholesky", want_w=False):
    """dF / d theta, gpak_grad_exact's layout: the stationary children's blocks in order, bias, sn2."""
    W = weights(xref.gram(X, terms, bias), y, sn2, labels, route)
    g = xref.grad_exact(X, y, terms, bias, sn2, W=W)
    return (g, W) if want_w else g


def objective(X, y, terms, bias, sn2, labels):
    """F = -log_pl of cvg_ref."""
    return -float(np.sum(cvg_ref.cv_groups(xref.gram(X, terms, bias), y, sn2, labels)[2]))


def pack_bins(sizes, cap=BIN):
    """The bins of the column mix, restated: consecutive groups packed greedily, a group opening a new bin when it does
    not fit the current one.  Returns the first group of every bin, then len(sizes)."""
    first, fill = [], 0
    for g, s in enumerate(sizes):
        if g == 0 or fill + int(s) > cap:
            first.append(g)
            fill = 0
        fill += int(s)
    return first + [len(sizes)]
