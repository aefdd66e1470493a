"""NumPy restatement of the gradient of the leave-one-out pseudo-likelihood (gpak_loo_grad).  TEST INFRASTRUCTURE,
written independently of the device code.

With Ky = K + sn2 I, Kinv = Ky^-1, alpha = Kinv y and kappa_i = Kinv_ii the objective is (Rasmussen & Williams,
eq. 5.10-5.13)

  F = -log_pl = sum_i [ -1/2 log kappa_i + alpha_i^2 / (2 kappa_i) ] + N/2 log 2 pi

and dF / d theta = 1/2 sum_ij W_ij d(Ky)_ij / d theta with

  c_i = (1 / kappa_i + alpha_i^2 / kappa_i^2) / 2,   b_i = alpha_i / kappa_i,   v = Kinv b,
  W   = 2 Kinv diag(c) Kinv - v alpha' - alpha v'

(from d kappa_i = -[Kinv dK Kinv]_ii and d alpha = -Kinv dK alpha).  W is symmetric, so exact_grad_ref.grad_exact, which
contracts any weight matrix with the full dK / d theta matrices, returns the gradient in gpak_grad_exact's layout.
tests/test_loo_grad.py checks this file against central differences of loo_ref's log_pl.
"""
import numpy as np

import exact_grad_ref as xref
import loo_ref


def weights(K, y, sn2, route="cholesky"):
    """W of the pseudo-likelihood.  route: "cholesky" (one factor, as the device) or "inv" (np.linalg.inv: a second
    float64 route to the same matrix)."""
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
    kappa = Kinv.diagonal().copy()
    c = 0.5 * (1.0 / kappa + alpha ** 2 / kappa ** 2)
    b = alpha / kappa
    v = Kinv @ b
    M = (Kinv * c[None, :]) @ Kinv
    return 2.0 * M - np.outer(v, alpha) - np.outer(alpha, v)


def grad_loo(X, y, terms, bias, sn2, route="cholesky", want_w=False):
    """dF / d theta, gpak_grad_exact's layout: the stationary children's blocks in order, bias, sn2."""
    W = weights(xref.gram(X, terms, bias), y, sn2, route)
    g = xref.grad_exact(X, y, terms, bias, sn2, W=W)
    return (g, W) if want_w else g


def objective(X, y, terms, bias, sn2):
    """F = -log_pl of loo_ref."""
    mean, var = loo_ref.loo(xref.gram(X, terms, bias), y, sn2)
    return -loo_ref.summary(y, mean, var)["log_pl"]
