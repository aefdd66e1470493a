"""NumPy restatements of ordinary kriging in a moving neighbourhood (gpak_predict_local_ok) and of the octant search
(gpak_local_neighbours_octant).  TEST INFRASTRUCTURE, written independently of the device code, in float64 and in
np.longdouble (one code path, the dtype an argument).

local_predict_ok is the block elimination include/gpak_local_ok.h states, on local_ref.local_predict's building blocks
(design_ref.averaged / chol / solve_lower), K_II, kbar, kbb exactly those of local_ref (bias, noise, white / nd included):

  w_y = L^-1 y_I, w_k = L^-1 kbar, w_1 = L^-1 1,   a = w_1 . w_1, b_y = w_1 . w_y, b_k = w_1 . w_k
  mu = b_y / a,  mean = w_k . w_y + (1 - b_k) mu,  latent = kbb - w_k . w_k + (1 - b_k)^2 / a,  var = latent + sn2 / nd

local_predict_ok_augmented is a second route that shares none of that: the (s + 1) x (s + 1) ordinary-kriging system

  [K0 1; 1' 0] [lambda; nu] = [kbar0; 1]         K0, kbar0, kbb0 from the kernel values ALONE, without the bias constant

solved by Gaussian elimination with partial pivoting (the matrix is indefinite), mean = lambda . y_I,
latent = kbb0 - lambda . kbar0 - nu, and the local mean from the same matrix with the right-hand side [0; 1].  The bias
drops out of ordinary kriging because the weights sum to one; that the two routes agree is tests/test_local_ok.py's.

An empty list has no estimate: NaN in mean, var, latent and mu, used = 0, notpd False.
"""
import functools

import numpy as np

import design_ref
import local_ref

LD = np.longdouble


def _lists(nbr, b, Ns):
    row = np.asarray(nbr)[b]
    s = int(np.argmax(row < 0)) if np.any(row < 0) else row.size
    assert np.all(row[s:] == -1) and np.all(row[:s] < Ns)
    return row[:s]


def local_predict_ok(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2, dt=LD):
    """Returns {mean, var, latent, mu, sk_latent (M, dtype dt), wsum (the weights' sum), notpd (M bool), used (M)}."""
    Xs, Xd = np.asarray(Xs, dtype=float), np.asarray(Xd, dtype=float)
    ys = np.asarray(ys, dtype=float).ravel()
    M = Xd.shape[0] // nd
    assert np.asarray(nbr).shape[0] == M and Xd.shape[0] == M * nd
    out = {key: np.full(M, np.nan, dtype=dt) for key in ("mean", "latent", "mu", "sk_latent", "wsum")}
    notpd, used = np.zeros(M, dtype=bool), np.zeros(M, dtype=int)
    noise = dt(sn2) + dt(white)
    for b in range(M):
        I = _lists(nbr, b, Xs.shape[0])
        s = used[b] = len(I)
        if s == 0:
            continue
        pts = Xd[b * nd:(b + 1) * nd]
        kbb = design_ref.averaged(pts, pts, nd, nd, terms, bias, dt)[0, 0] + dt(white) / dt(nd)
        K = design_ref.averaged(Xs[I], Xs[I], 1, 1, terms, bias, dt) + noise * np.eye(s, dtype=dt)
        kbar = design_ref.averaged(Xs[I], pts, 1, nd, terms, bias, dt)[:, 0]
        try:
            L = design_ref.chol(np.asarray(K, dtype=dt))
        except np.linalg.LinAlgError:
            notpd[b] = True
            continue
        Z = design_ref.solve_lower(L, np.column_stack([ys[I].astype(dt), kbar, np.ones(s, dtype=dt)]))
        wy, wk, w1 = Z[:, 0], Z[:, 1], Z[:, 2]
        a, by, bk = w1 @ w1, w1 @ wy, w1 @ wk
        mu = by / a
        r = dt(1) - bk
        out["mu"][b] = mu
        out["mean"][b] = wk @ wy + r * mu
        out["sk_latent"][b] = kbb - wk @ wk
        out["latent"][b] = kbb - wk @ wk + r * r / a
        # the weights: lambda = K^-1 (kbar + nu 1), nu = (1 - b_k) / a;  1' lambda = b_k + nu a
        out["wsum"][b] = bk + (r / a) * a
    out["var"] = out["latent"] + dt(sn2) / dt(nd)
    out["notpd"], out["used"] = notpd, used
    return out


def solve_pivoted(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting, in A's dtype"""
    A, B = np.array(A), np.array(B, dtype=A.dtype)
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], B[[j, p]] = A[[p, j]], B[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:, j:] -= np.outer(f, A[j, j:])
        B[j + 1:] -= np.outer(f, B[j])
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X


def local_predict_ok_augmented(Xs, ys, Xd, nd, nbr, terms, white, sn2, dt=LD):
    """The second route (no bias argument: it does not enter).  Returns {mean, var, latent, mu, wsum (M, dtype dt), used}."""
    Xs, Xd = np.asarray(Xs, dtype=float), np.asarray(Xd, dtype=float)
    ys = np.asarray(ys, dtype=float).ravel()
    M = Xd.shape[0] // nd
    out = {key: np.full(M, np.nan, dtype=dt) for key in ("mean", "latent", "mu", "wsum")}
    used = np.zeros(M, dtype=int)
    noise = dt(sn2) + dt(white)
    for b in range(M):
        I = _lists(nbr, b, Xs.shape[0])
        s = used[b] = len(I)
        if s == 0:
            continue
        pts = Xd[b * nd:(b + 1) * nd]
        A = np.zeros((s + 1, s + 1), dtype=dt)
        A[:s, :s] = design_ref.averaged(Xs[I], Xs[I], 1, 1, terms, 0.0, dt) + noise * np.eye(s, dtype=dt)
        A[:s, s] = A[s, :s] = dt(1)
        rhs = np.zeros((s + 1, 2), dtype=dt)
        rhs[:s, 0] = design_ref.averaged(Xs[I], pts, 1, nd, terms, 0.0, dt)[:, 0]
        rhs[s, :] = dt(1)
        kbb0 = design_ref.averaged(pts, pts, nd, nd, terms, 0.0, dt)[0, 0] + dt(white) / dt(nd)
        sol = solve_pivoted(A, rhs)
        lam, nu, g = sol[:s, 0], sol[s, 0], sol[:s, 1]
        y = ys[I].astype(dt)
        out["mean"][b] = lam @ y
        out["latent"][b] = kbb0 - lam @ rhs[:s, 0] - nu
        out["mu"][b] = g @ y
        out["wsum"][b] = lam.sum()
    out["var"] = out["latent"] + dt(sn2) / dt(nd)
    out["used"] = used
    return out


def brute_octant_neighbours(Xs, Xc, k, per_octant, G=None, radius=0.0):
    """(nbr M x k int32, used M int32) of gpak_local_neighbours_octant by a full sort, in the arithmetic its header states
    (that of local_ref.brute_neighbours): octant = sum_j 2^j [e_j < 0] over the first three transformed differences; of the
    samples with dist2 <= radius^2 the per_octant first of each octant by (dist2, index), of those the k first."""
    Xs, Xc = np.asarray(Xs, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
    d = Xs.shape[1]
    assert radius > 0.0 and 1 <= per_octant <= k

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
    index = np.arange(Xs.shape[0])
    for b in range(M):
        e = Ts[:, 0] - Tc[b, 0]
        octant = (e < 0.0).astype(int)
        d2 = e * e
        for j in range(1, d):
            e = Ts[:, j] - Tc[b, j]
            if j < 3:
                octant += (e < 0.0).astype(int) << j
            d2 = d2 + e * e
        order = np.lexsort((index, d2))                        # by d2, then by index
        order = order[d2[order] <= radius * radius]
        keep = np.concatenate([order[octant[order] == o][:per_octant] for o in range(8)]).astype(int)
        keep = keep[np.lexsort((keep, d2[keep]))][:k]
        nbr[b, :keep.size] = keep
        used[b] = keep.size
    return nbr, used


@functools.lru_cache(maxsize=None)
def reference(name, dt=LD):
    """local_predict_ok on a case of local_cases.CASES: computed once per process, read-only"""
    import local_cases as lc
    import test_block_gpu as tb
    Ns, M, nd, comp = lc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys, Xd, nbr = lc.inputs(name)
    out = local_predict_ok(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2, dt)
    for v in out.values():
        v.setflags(write=False)
    return out


def errors(comp, ys, got, ref, key):
    """max |got - ref[key]|: means and mu over max|y|, variances over the prior variance (local_cases.errors)"""
    import test_block_gpu as tb
    scale = np.abs(ys).max() if key in ("mean", "mu") else tb.prior_variance(comp)
    return float(np.abs(np.asarray(got, dtype=LD) - ref[key]).max() / scale)
