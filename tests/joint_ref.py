"""NumPy reference of the joint posterior of block averages (gpak_predict_joint / gpak_sample_joint).  TEST
INFRASTRUCTURE, written independently of the device code; tests/test_joint.py pins it against block_ref.block_predict and
block_ref.full_posterior.

Block b = rows b * nd .. b * nd + nd of Xd, uniform weights.  The latent covariance between two block averages is the
mean of the nd x nd part of the full posterior covariance of all M * nd points that the two blocks span.  The White
child is a point-support nugget of the BLOCK path's kind: white / nd on the diagonal of the block covariance (the nd
coincident pairs of a block with itself) and nothing between different blocks, even where two blocks share a point --
so it is taken out of what block_ref.full_posterior puts on the diagonal of the point covariance and added per block.
"""
import numpy as np

import block_ref
import exact_grad_ref as xref

LD = np.longdouble


def prior_long(Xd, nd, terms, bias, white, slab_elems=2_000_000):
    """The prior covariance between the block averages (M x M, np.longdouble): (1/nd^2) sum_{a,a'} k + white/nd on b == b'.
    Formed a slab of blocks at a time to bound the size of the long-double point matrix; the values are the same."""
    Xd = np.asarray(Xd, dtype=LD)
    P, d = Xd.shape
    M = P // nd
    per = max(1, slab_elems // (P * nd))
    Kbb = np.zeros((M, M), dtype=LD)
    for b0 in range(0, M, per):
        b1 = min(M, b0 + per)
        rows = Xd[b0 * nd:b1 * nd]
        dcols = [rows[:, c][:, None] - Xd[:, c][None, :] for c in range(d)]
        K = np.full((rows.shape[0], P), LD(bias))
        for kind, p in terms:
            K += block_ref._k_long(kind, p, dcols, d)
        Kbb[b0:b1] = K.reshape(b1 - b0, nd, M, nd).sum(axis=(1, 3)) / (LD(nd) * LD(nd))
    return Kbb + LD(white) / LD(nd) * np.eye(M, dtype=LD)


def _k_double(kind, p, dcols, d):
    """block_ref._k_long in double: one stationary term on coordinate differences."""
    p = [float(v) for v in p]
    if kind == xref.EXPANS:
        A, _ = xref.expans_metric(p)
        A2 = A @ A
        D = sum((A2[a, b] if a == b else 2 * A2[a, b]) * dcols[a] * dcols[b] for a in range(3) for b in range(a, 3))
        if d == 4:
            D = D + (p[7] * dcols[3]) ** 2
        return p[6] ** 2 * np.exp(-np.sqrt(np.maximum(D, 0)))
    d2 = sum(dcols[c] ** 2 for c in range(d)) / p[0] ** 2
    if kind == xref.EXP:
        return p[1] ** 2 * np.exp(-np.sqrt(d2))
    return p[2] ** 2 * np.exp(-0.5 * p[1] * d2)


def _averaged(A, B, nda, ndb, terms, bias, slab_elems=4_000_000):
    """(1 / (nda ndb)) sum_{a,a'} k(A_{i,a}, B_{j,a'}) in double, a slab of rows at a time."""
    d = A.shape[1]
    ma, mb = A.shape[0] // nda, B.shape[0] // ndb
    out = np.zeros((ma, mb))
    per = max(1, slab_elems // (B.shape[0] * nda))
    for i0 in range(0, ma, per):
        i1 = min(ma, i0 + per)
        rows = A[i0 * nda:i1 * nda]
        dcols = [rows[:, c][:, None] - B[:, c][None, :] for c in range(d)]
        K = np.full((rows.shape[0], B.shape[0]), float(bias))
        for kind, p in terms:
            K += _k_double(kind, p, dcols, d)
        out[i0:i1] = K.reshape(i1 - i0, nda, mb, ndb).mean(axis=(1, 3))
    return out


def joint(X, y, Xd, nd, terms, bias, white, sn2, want_prior=True, method="points"):
    """Returns {mean (M), latent (M x M), prior (M x M, longdouble; None unless want_prior)}; the noisy covariance is
    latent + sn2/nd I.
    method "points": the definition -- the nd x nd block averages of block_ref.full_posterior on all M * nd points.
    method "blocks": the same quantity with the averages taken first (averaging is linear: Kbb - Kbar' Ky^-1 Kbar),
    for sets whose point covariance is too large to form; tests/test_joint.py pins it against "points"."""
    X, Xd = np.asarray(X, dtype=float), np.asarray(Xd, dtype=float)
    P = Xd.shape[0]
    M = P // nd
    prior = prior_long(Xd, nd, terms, bias, white) if want_prior else None
    if method == "blocks":
        N = X.shape[0]
        Ky = _averaged(X, X, 1, 1, terms, bias) + (white + sn2) * np.eye(N)
        Kbar = _averaged(X, Xd, 1, nd, terms, bias)
        sol = np.linalg.solve(Ky, np.column_stack([np.asarray(y, dtype=float).ravel(), Kbar]))
        Kbb = _averaged(Xd, Xd, nd, nd, terms, bias)
        latent = Kbb + white / nd * np.eye(M) - Kbar.T @ sol[:, 1:]
        return {"mean": Kbar.T @ sol[:, 0], "latent": (latent + latent.T) / 2, "prior": prior}
    mu, S = block_ref.full_posterior(X, y, Xd, terms, bias, white, sn2)
    S = S - white * np.eye(P)                         # full_posterior's point nugget, whatever it did between coincident points
    latent = S.reshape(M, nd, M, nd).mean(axis=(1, 3)) + white / nd * np.eye(M)
    return {"mean": mu.reshape(M, nd).mean(axis=1), "latent": latent, "prior": prior}
