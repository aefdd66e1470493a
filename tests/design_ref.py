"""NumPy restatement of infill drilling design (gpak_design).  TEST INFRASTRUCTURE, written independently of the device
code, in float64 and in np.longdouble (one code path, the dtype an argument); tests/test_design.py pins it against refits
through block_ref.block_predict.

Stack z = [block averages of the T targets; latent values at the Mc candidate points].  Its prior covariance comes from
joint_ref._averaged (float64) or block_ref._k_long (long double) on the two segments with nd and 1 point(s) per entry; the
White child is white / nd on a target's own diagonal entry and nothing anywhere else.  With Ky = K + (white + sn2) I = L L',
V = L^-1 Kbar:   P = prior - V' V.   For hole h with rows I:  A = P_II + (sn2 + white) I = R R',
reduction[:, h] = column sums of (R^-1 P_{I, targets})^2,  gain = wt . reduction.  A pick: U = R^-1 P_{I, :},  P -= U' U.
"""
import numpy as np

import block_ref
import joint_ref

LD = np.longdouble


def averaged(A, B, nda, ndb, terms, bias, dt):
    """(1 / (nda ndb)) sum_{a,a'} k(A_{i,a}, B_{j,a'}) in dtype dt"""
    if dt is not LD:
        return joint_ref._averaged(np.asarray(A, dtype=float), np.asarray(B, dtype=float), nda, ndb, terms, bias)
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    d = A.shape[1]
    ma, mb = A.shape[0] // nda, B.shape[0] // ndb
    out = np.zeros((ma, mb), dtype=LD)
    per = max(1, 2_000_000 // (B.shape[0] * nda))
    for i0 in range(0, ma, per):
        i1 = min(ma, i0 + per)
        rows = A[i0 * nda:i1 * nda]
        dcols = [rows[:, c][:, None] - B[:, c][None, :] for c in range(d)]
        K = np.full((rows.shape[0], B.shape[0]), LD(bias))
        for kind, p in terms:
            K += block_ref._k_long(kind, p, dcols, d)
        out[i0:i1] = K.reshape(i1 - i0, nda, mb, ndb).sum(axis=(1, 3)) / (LD(nda) * LD(ndb))
    return out


def chol(A):
    """lower Cholesky factor in A's dtype (left-looking, a column at a time)"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j:, j] = c / np.sqrt(c[0])
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution, a row at a time"""
    X = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def stack_cov(X, Xt, nd, Xc, terms, bias, white, sn2, dt=LD):
    """P (S x S, S = T + Mc) in dtype dt"""
    T = np.asarray(Xt).shape[0] // nd
    N = np.asarray(X).shape[0]
    one = dt(1)
    prior = np.block([[averaged(Xt, Xt, nd, nd, terms, bias, dt) + dt(white) / dt(nd) * np.eye(T, dtype=dt),
                       averaged(Xt, Xc, nd, 1, terms, bias, dt)],
                      [averaged(Xc, Xt, 1, nd, terms, bias, dt), averaged(Xc, Xc, 1, 1, terms, bias, dt)]])
    Kbar = np.hstack([averaged(X, Xt, 1, nd, terms, bias, dt), averaged(X, Xc, 1, 1, terms, bias, dt)])
    Ky = averaged(X, X, 1, 1, terms, bias, dt) + (dt(white) + dt(sn2)) * one * np.eye(N, dtype=dt)
    V = solve_lower(chol(Ky), Kbar)
    P = prior - V.T @ V
    return (P + P.T) / dt(2)


def score(P, T, members, live, noise, wt):
    """(gain over all holes (NaN where not live), {h: reduction column}, {h: R}) of the live holes"""
    dt = P.dtype.type
    gain = np.full(len(members), np.nan, dtype=P.dtype)
    red, fac = {}, {}
    for h in live:
        I = T + members[h]
        R = chol(P[np.ix_(I, I)] + dt(noise) * np.eye(len(I), dtype=P.dtype))
        Z = solve_lower(R, P[I, :T])
        red[h] = (Z * Z).sum(axis=0)
        gain[h] = wt @ red[h]
        fac[h] = R
    return gain, red, fac


def design(X, Xt, nd, Xc, hole, terms, bias, white, sn2, wt=None, k=0, dt=LD, P=None):
    """Returns {gain (H), reduction (T x H), var (T), var_after (T), picked, pick_gain, rounds: the gain vector every pick
    was taken from (NaN at retired holes), var_before, var_after_sum}.  hole: labels 0 .. H - 1, every one used."""
    hole = np.asarray(hole)
    H = int(hole.max()) + 1
    members = [np.flatnonzero(hole == h) for h in range(H)]
    T = np.asarray(Xt).shape[0] // nd
    P = stack_cov(X, Xt, nd, Xc, terms, bias, white, sn2, dt) if P is None else np.array(P, dtype=dt)
    w = np.ones(T, dtype=dt) if wt is None else np.asarray(wt, dtype=dt)
    noise = dt(sn2) + dt(white)
    live = list(range(H))
    gain0, red0, fac = score(P, T, members, live, noise, w)
    out = {"gain": gain0, "reduction": np.column_stack([red0[h] for h in range(H)]), "var": np.diag(P)[:T].copy(),
           "picked": [], "pick_gain": [], "rounds": []}
    gain = gain0
    for p in range(k):
        best = live[0]
        for h in live[1:]:                      # ascending h, strict >: a tie goes to the smallest h
            if gain[h] > gain[best]:
                best = h
        out["picked"].append(best)
        out["pick_gain"].append(gain[best])
        out["rounds"].append(gain.copy())
        I = T + members[best]
        U = solve_lower(fac[best], P[I, :])
        P = P - U.T @ U
        live.remove(best)
        if p + 1 < k:
            gain, _, fac = score(P, T, members, live, noise, w)
    out["var_after"] = np.diag(P)[:T].copy()
    out["var_before"] = w @ out["var"]
    out["var_after_sum"] = w @ out["var_after"]
    out["P_after"] = P
    return out


def pick_gaps(rounds):
    """per pick: (largest - second largest) / largest of the gains the pick was taken from (inf with one hole left)"""
    gaps = []
    for g in rounds:
        v = np.sort(np.asarray(g, dtype=LD)[~np.isnan(np.asarray(g, dtype=float))])[::-1]
        gaps.append(float((v[0] - v[1]) / v[0]) if v.size > 1 else np.inf)
    return gaps
