"""NumPy restatement of moving-neighbourhood kriging (gpak_predict_local).  TEST INFRASTRUCTURE, written independently of the
device code, in float64 and in np.longdouble (one code path, the dtype an argument); tests/test_local.py pins it against
block_ref.block_predict on a model that holds exactly a node's samples.

Node b = rows b * nd .. b * nd + nd of Xd, I = the entries of row b of nbr in front of the first -1, noise = sn2 + white:

  K_II   = k(x_i, x_j) + bias + noise I = L L'          kbar_i = (1/nd) sum_a k(p_a, x_i) + bias
  kbb    = (1/nd^2) sum_{a,a'} (k(p_a, p_a') + bias) + white / nd
  mean   = (L^-1 kbar) . (L^-1 y_I)
  latent = kbb - |L^-1 kbar|^2                          not clamped
  var    = latent + sn2 / nd

An empty list gives mean 0 and latent = kbb; a pivot that is not positive gives NaN and sets notpd[b].  The kernel values
come from design_ref.averaged (joint_ref._averaged in float64, block_ref._k_long in long double), the factor and the
substitution from design_ref.chol / solve_lower.
"""
import numpy as np

import design_ref

LD = np.longdouble


def local_predict(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2, dt=LD):
    """Returns {mean, var, latent (M, dtype dt), notpd (M bool), used (M)}."""
    Xs, Xd = np.asarray(Xs, dtype=float), np.asarray(Xd, dtype=float)
    ys = np.asarray(ys, dtype=float).ravel()
    nbr = np.asarray(nbr)
    M = Xd.shape[0] // nd
    assert nbr.shape[0] == M and Xd.shape[0] == M * nd
    mean, latent = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
    notpd, used = np.zeros(M, dtype=bool), np.zeros(M, dtype=int)
    noise = dt(sn2) + dt(white)
    for b in range(M):
        row = nbr[b]
        s = int(np.argmax(row < 0)) if np.any(row < 0) else row.size
        assert np.all(row[s:] == -1) and np.all(row[:s] < Xs.shape[0])
        used[b] = s
        pts = Xd[b * nd:(b + 1) * nd]
        kbb = design_ref.averaged(pts, pts, nd, nd, terms, bias, dt)[0, 0] + dt(white) / dt(nd)
        if s == 0:
            latent[b] = kbb
            continue
        I = row[:s]
        K = design_ref.averaged(Xs[I], Xs[I], 1, 1, terms, bias, dt) + noise * np.eye(s, dtype=dt)
        kbar = design_ref.averaged(Xs[I], pts, 1, nd, terms, bias, dt)[:, 0]
        try:
            L = design_ref.chol(np.asarray(K, dtype=dt))
        except np.linalg.LinAlgError:
            notpd[b] = True
            mean[b] = latent[b] = np.nan
            continue
        Z = design_ref.solve_lower(L, np.column_stack([ys[I].astype(dt), kbar]))
        mean[b] = Z[:, 1] @ Z[:, 0]
        latent[b] = kbb - Z[:, 1] @ Z[:, 1]
    return {"mean": mean, "var": latent + dt(sn2) / dt(nd), "latent": latent, "notpd": notpd, "used": used}


def brute_neighbours(Xs, Xc, k, G=None, radius=0.0):
    """(nbr M x k int32, used M int32) of gpak_local_neighbours by a full sort, in the arithmetic its header states:
    t_j = ((x_0 G_0j + x_1 G_1j) + x_2 G_2j) [+ x_3 G_3j], dist2 = ((e_0^2 + e_1^2) + e_2^2) [+ e_3^2], every product and sum
    rounded on its own; ascending (dist2, index); dist2 <= radius^2 when radius > 0."""
    Xs, Xc = np.asarray(Xs, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
    d = Xs.shape[1]

    def transform(X):
        if G is None:
            return X
        Gm = np.asarray(G, dtype=np.float64)
        cols = []
        for j in range(d):
            t = X[:, 0] * Gm[0, j]
            for r in range(1, d):
                t = t + X[:, r] * Gm[r, j]
            cols.append(t)
        return np.column_stack(cols)

    Ts, Tc = transform(Xs), transform(Xc)
    M = Xc.shape[0]
    nbr = np.full((M, k), -1, dtype=np.int32)
    used = np.zeros(M, dtype=np.int32)
    for b in range(M):
        e = Ts[:, 0] - Tc[b, 0]
        d2 = e * e
        for j in range(1, d):
            e = Ts[:, j] - Tc[b, j]
            d2 = d2 + e * e
        order = np.lexsort((np.arange(Xs.shape[0]), d2))       # by d2, then by index
        if radius > 0.0:
            order = order[d2[order] <= radius * radius]
        n = min(k, order.size)
        nbr[b, :n] = order[:n]
        used[b] = n
    return nbr, used
