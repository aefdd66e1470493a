"""NumPy reference (np.longdouble) of conditioning by kriging and of the spectral prior (gpak_condition /
gpak_sample_path).  TEST INFRASTRUCTURE, written independently of the device code; tests/test_path.py pins it against
joint_ref's latent covariance (the restatement is Matheron's rule) and against the closed form of the spectral version.

With Ky = K + (white + sn2) I, alpha = Ky^-1 y and Kbar the averaged cross-kernel (N x M, block_ref.block_cross):

  Z = Fsim + Kbar' (alpha 1' - Ky^-1 Ysim),   mean = Kbar' alpha

Spectral prior: feature f of term t = feat_term[f] has frequency omega[f] in the term's transformed coordinates
u_t(x) = (x - mu) A_t (mu: the pooled mean of the training set and all node points), amplitude sqrt(var2_t / F_t):

  f_s(x) = sum_f amp_f (ab[2f, s] cos(omega_f . u_t(x)) + ab[2f + 1, s] sin(omega_f . u_t(x))) + sqrt(bias) b0[s]
  Fsim = block averages of f_s,   Ysim = f_s(X) + sqrt(sn2 + white) E
"""
import numpy as np

import block_ref
import design_ref
import exact_grad_ref as xref
import joint_ref

LD = np.longdouble


def ky_long(X, terms, bias, white, sn2):
    """K + (white + sn2) I in long double"""
    N = np.asarray(X).shape[0]
    return joint_ref.prior_long(X, 1, terms, bias, white) + LD(sn2) * np.eye(N, dtype=LD)


def solve_ky(L, B):
    """Ky^-1 B from the lower factor L of Ky (long double)"""
    V = design_ref.solve_lower(L, B)
    Lt = L.T[::-1, ::-1]                                   # L' x = v backwards = a forward substitution on the reversal
    return design_ref.solve_lower(Lt, V[::-1])[::-1]


class Model:
    """The factor of Ky, alpha and Kbar of one (training set, composition, nodes), in long double"""

    def __init__(self, X, y, Xd, nd, terms, bias, white, sn2):
        self.X, self.Xd, self.nd = np.asarray(X, dtype=float), np.asarray(Xd, dtype=float), int(nd)
        self.terms, self.bias, self.white, self.sn2 = terms, bias, white, sn2
        self.N, self.d = self.X.shape
        self.M = self.Xd.shape[0] // self.nd
        self.y = np.asarray(y, dtype=LD).ravel()
        self.L = design_ref.chol(ky_long(self.X, terms, bias, white, sn2))
        self.alpha = solve_ky(self.L, self.y[:, None])[:, 0]
        self.Kbar = block_ref.block_cross(self.X, self.Xd, self.nd, terms, bias)          # N x M
        self.mean = self.Kbar.T @ self.alpha

    def gain(self):
        """G = Kbar' Ky^-1 (M x N)"""
        return solve_ky(self.L, self.Kbar).T

    def condition(self, Ysim, Fsim=None):
        """(Z, mean), long double"""
        Ysim = np.asarray(Ysim, dtype=LD).reshape(self.N, -1)
        A = self.alpha[:, None] - solve_ky(self.L, Ysim)
        Z = self.Kbar.T @ A
        if Fsim is not None:
            Z = Z + np.asarray(Fsim, dtype=LD).reshape(self.M, -1)
        return Z, self.mean

    # ---- the spectral prior ------------------------------------------------------------------------------------------
    def pooled_mean(self):
        return (self.X.sum(axis=0) + self.Xd.sum(axis=0)) / (self.N + self.Xd.shape[0])

    def metric(self, t):
        """(A (d x d, long double), var2) of stationary term t: u = (x - mu) A"""
        kind, p = self.terms[t]
        p = [float(v) for v in p]
        A = np.zeros((self.d, self.d), dtype=LD)
        if kind == xref.EXPANS:
            A3, _ = xref.expans_metric(p)
            A[:3, :3] = A3
            if self.d == 4:
                A[3, 3] = p[7]
            return A, LD(p[6]) ** 2
        A[np.arange(self.d), np.arange(self.d)] = LD(1) / LD(p[0])
        return A, LD(p[1] if kind == xref.EXP else p[2]) ** 2

    def features(self, points, nd, feat_term, omega):
        """(Phi (rows x 2F, block-averaged cos / sin), amp (F), the largest sum_k |omega_fk u_k| per feature)"""
        P = np.asarray(points, dtype=LD) - self.pooled_mean().astype(LD)
        ft = np.asarray(feat_term)
        F = ft.size
        rows = P.shape[0] // nd
        Phi, amp, arg = np.zeros((rows, 2 * F), dtype=LD), np.zeros(F, dtype=LD), np.zeros(F)
        for t in range(len(self.terms)):
            idx = np.flatnonzero(ft == t)
            if idx.size == 0:
                continue
            A, var2 = self.metric(t)
            U = P @ A
            W = np.asarray(omega, dtype=LD)[idx][:, :self.d]
            th = U @ W.T
            Phi[:, 2 * idx] = np.cos(th).reshape(rows, nd, idx.size).mean(axis=1)
            Phi[:, 2 * idx + 1] = np.sin(th).reshape(rows, nd, idx.size).mean(axis=1)
            amp[idx] = np.sqrt(var2 / LD(idx.size))
            arg[idx] = (np.abs(U)[:, None, :] * np.abs(W)[None, :, :]).sum(axis=2).max(axis=0).astype(float)
        return Phi, amp, arg

    def prior_draw(self, feat_term, omega, ab, b0, E):
        """(Fsim (M x S), Ysim (N x S)) of the spectral prior, long double"""
        ab = np.asarray(ab, dtype=LD)
        S = ab.shape[1]
        const = np.sqrt(LD(self.bias)) * (np.zeros(S, dtype=LD) if b0 is None else np.asarray(b0, dtype=LD))
        Pn, amp, _ = self.features(self.Xd, self.nd, feat_term, omega)
        Px, _, _ = self.features(self.X, 1, feat_term, omega)
        W = np.repeat(amp, 2)[:, None] * ab
        Fsim = Pn @ W + const[None, :]
        Ysim = Px @ W + const[None, :] + np.sqrt(LD(self.sn2) + LD(self.white)) * np.asarray(E, dtype=LD)
        return Fsim, Ysim

    def sample_path(self, feat_term, omega, ab, b0, E):
        Fsim, Ysim = self.prior_draw(feat_term, omega, ab, b0, E)
        return self.condition(Ysim, Fsim)

    def spectral_cov(self, feat_term, omega):
        """The closed form of the covariance of sample_path's Z under unit normals:
        K^** - G K^x* - K^*x G' + G (K^xx + (sn2 + white) I) G',  K^(h) = sum_t (var2_t / F_t) sum_f cos(omega_f . h) + bias,
        the cosines of DIFFERENCES of transformed points (averaged over the blocks' points), G from the exact kernel."""
        ft = np.asarray(feat_term)
        pts = np.vstack([self.Xd, self.X]).astype(LD)
        n = pts.shape[0]
        Khat = np.full((n, n), LD(self.bias))
        for t in range(len(self.terms)):
            idx = np.flatnonzero(ft == t)
            if idx.size == 0:
                continue
            A, var2 = self.metric(t)
            U = pts @ A
            for f in idx:
                w = np.asarray(omega, dtype=LD)[f][:self.d]
                ph = U @ w
                Khat += var2 / LD(idx.size) * np.cos(ph[:, None] - ph[None, :])
        Mn = self.M * self.nd
        nn = Khat[:Mn, :Mn].reshape(self.M, self.nd, self.M, self.nd).mean(axis=(1, 3))
        nx = Khat[:Mn, Mn:].reshape(self.M, self.nd, self.N).mean(axis=1)
        xx = Khat[Mn:, Mn:] + (LD(self.sn2) + LD(self.white)) * np.eye(self.N, dtype=LD)
        G = self.gain()
        return nn - G @ nx.T - nx @ G.T + G @ xx @ G.T


def exact_prior_factor(m):
    """The lower factor (long double) of the exact joint prior of [node averages; noisy observations] of Model m:
    [[Kbb + white / nd I, Kbar'], [Kbar, Ky]]"""
    Kbb = joint_ref.prior_long(m.Xd, m.nd, m.terms, m.bias, m.white)
    Ky = ky_long(m.X, m.terms, m.bias, m.white, m.sn2)
    C = np.block([[Kbb, m.Kbar.T], [m.Kbar, Ky]])
    return design_ref.chol(C)
