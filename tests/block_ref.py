"""NumPy reference of block-support prediction (gpak_predict_block / gpak_block_cross): mean and variance of the average
of the field over blocks given by nd discretisation points each.  TEST INFRASTRUCTURE, written independently of the
device code; tests/test_block.py pins it against the averaged full posterior covariance of the points.

Block b = rows b * nd .. b * nd + nd of Xd, uniform weights.  With Ky = K + sn2 I = sn2 B, B = L L' and alpha = Ky^-1 y:

  kbar_b   = (1/nd) sum_a k(X, x_{b,a})                        bias included, a White child contributes nothing
  mean_b   = kbar_b . alpha
  kbb_b    = (1/nd^2) sum_{a,a'} k(x_{b,a}, x_{b,a'}) + white / nd
  latent_b = max(0, kbb_b - |L^-1 kbar_b|^2 / sn2)
  var_b    = latent_b + sn2 / nd

Every kernel value comes from exact_grad_ref.gram on the stacked set [X; Xd] (the direct distance form, so no pooled
mean enters): its train x train, train x point and point x point parts.  A value depends on its two points alone, so a
long list of blocks is stacked a slice at a time to bound the size of that matrix; the values are the same.
"""
import numpy as np

import exact_grad_ref as xref

STACK_POINTS = 3000   # discretisation points stacked under X at once


def block_points(centres, size, disc):
    """The cell-centred discretisation, restated: x slowest, z fastest, further columns copied from the centre."""
    c = np.asarray(centres, dtype=float)
    nx, ny, nz = (int(v) for v in disc)
    rows = []
    for b in range(c.shape[0]):
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    p = c[b].copy()
                    p[0] += ((i + 0.5) / nx - 0.5) * size[0]
                    p[1] += ((j + 0.5) / ny - 0.5) * size[1]
                    p[2] += ((k + 0.5) / nz - 0.5) * size[2]
                    rows.append(p)
    return np.array(rows), nx * ny * nz


def _parts(X, Xd, nd, terms, bias):
    """Ktt (N x N), kbar (N x M) and the mean of every block's own nd x nd part (M), White apart."""
    X, Xd = np.asarray(X, dtype=float), np.asarray(Xd, dtype=float)
    N, M = X.shape[0], Xd.shape[0] // nd
    per = max(1, STACK_POINTS // nd)
    Ktt, kbar, self_mean = None, np.zeros((N, M)), np.zeros(M)
    for b0 in range(0, M, per):
        b1 = min(M, b0 + per)
        K = xref.gram(np.vstack([X, Xd[b0 * nd:b1 * nd]]), terms, bias)
        if Ktt is None:
            Ktt = K[:N, :N].copy()
        for b in range(b0, b1):
            lo = N + (b - b0) * nd
            kbar[:, b] = K[:N, lo:lo + nd].sum(axis=1) / nd
            self_mean[b] = K[lo:lo + nd, lo:lo + nd].sum() / (nd * nd)
    return Ktt, kbar, self_mean


def block_predict(X, y, Xd, nd, terms, bias, white, sn2):
    """Returns {mean, var, latent, kbar}: var = latent + sn2 / nd."""
    y = np.asarray(y, dtype=float).ravel()
    Ktt, kbar, self_mean = _parts(X, Xd, nd, terms, bias)
    N = Ktt.shape[0]
    L = np.linalg.cholesky(np.eye(N) + (Ktt + white * np.eye(N)) / sn2)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y / sn2))
    V = np.linalg.solve(L, kbar)
    latent = np.maximum(0.0, self_mean + white / nd - np.sum(V * V, axis=0) / sn2)
    return {"mean": kbar.T @ alpha, "var": latent + sn2 / nd, "latent": latent, "kbar": kbar}


def full_posterior(X, y, Xp, terms, bias, white, sn2):
    """Mean (P) and LATENT covariance (P x P) of the field at the points Xp: K** - K*' (K + sn2 I)^-1 K*, the White
    child on the diagonal of K** (a point-support nugget) and of the training covariance."""
    X, Xp = np.asarray(X, dtype=float), np.asarray(Xp, dtype=float)
    N = X.shape[0]
    K = xref.gram(np.vstack([X, Xp]), terms, bias)
    Ky = K[:N, :N] + (white + sn2) * np.eye(N)
    Ks = K[:N, N:]
    sol = np.linalg.solve(Ky, np.column_stack([np.asarray(y, dtype=float).ravel(), Ks]))
    return Ks.T @ sol[:, 0], K[N:, N:] + white * np.eye(Xp.shape[0]) - Ks.T @ sol[:, 1:]


def _k_long(kind, p, dcols, d):
    """One stationary term on longdouble coordinate differences (the formulas of the module docstring of
    exact_grad_ref; the metric A itself is formed in double as the device's is)."""
    p = [float(v) for v in p]
    if kind == xref.EXPANS:
        A, _ = xref.expans_metric(p)
        A2 = (A @ A).astype(np.longdouble)
        D = sum((A2[a, b] if a == b else 2 * A2[a, b]) * dcols[a] * dcols[b] for a in range(3) for b in range(a, 3))
        if d == 4:
            D = D + (np.longdouble(p[7]) * dcols[3]) ** 2
        return np.longdouble(p[6]) ** 2 * np.exp(-np.sqrt(np.maximum(D, 0)))
    d2 = sum(dcols[c] ** 2 for c in range(d)) / np.longdouble(p[0]) ** 2
    if kind == xref.EXP:
        return np.longdouble(p[1]) ** 2 * np.exp(-np.sqrt(d2))
    return np.longdouble(p[2]) ** 2 * np.exp(-np.longdouble(0.5) * np.longdouble(p[1]) * d2)


def block_cross(X, Xd, nd, terms, bias):
    """kbar (N x M) in np.longdouble."""
    X, Xd = np.asarray(X, dtype=np.longdouble), np.asarray(Xd, dtype=np.longdouble)
    N, d = X.shape
    M = Xd.shape[0] // nd
    dcols = [X[:, c][:, None] - Xd[:, c][None, :] for c in range(d)]
    K = np.full((N, M * nd), np.longdouble(bias))
    for kind, p in terms:
        K += _k_long(kind, p, dcols, d)
    return K.reshape(N, M, nd).sum(axis=2) / np.longdouble(nd)
