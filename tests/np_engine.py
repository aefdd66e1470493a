"""CPU stand-in for HipEngine, TEST INFRASTRUCTURE ONLY (uses numpy/scipy and the oracle's sigInv).

It lets the world_size>1 gloo tests drive tests/py_schedule.py's DistGP -- the ownership map, the
look-ahead schedule, the panel pack/broadcast and the solve collectives -- on a machine without
a GPU.  It mirrors the semantics of include/gpak_dev.h function by function.
"""
import numpy as np
import scipy.linalg as sl
import torch

TILE = 128


PANEL_MID = 512          # csrc/potrf_plan.h GPAK_PANEL_MID


def potrf16(S):
    """One 16 x 16 diagonal block as csrc/potrf.hip's diag_block does it: Gaussian elimination by rows on [S | I] (S
    symmetric), pivot r scaled by 1 / sqrt(d), a pivot that is not > 0 replaced by 1.  Returns (U^T = L with leftovers
    above the diagonal, L^-1 with exact zeros above it, first bad pivot or 16)."""
    X = np.hstack([S, np.eye(16)])
    bad = 16
    for r in range(16):
        d = X[r, r]
        if not d > 0.0:
            bad = min(bad, r)
            d = 1.0
        g = np.sqrt(d)
        xr = X[r] * (1.0 / g)
        xr[r] = g
        X[r] = xr
        if r < 15:
            X[r + 1:] -= np.outer(xr[r + 1:16], xr)
    return X[:, :16].T, X[:, 16:], bad


def potrf128(D):
    """The 128 x 128 block kernel restated: 16-wide right-looking steps, the panel formed as a product with the explicit
    inverse of the 16 x 16 diagonal block, the block's inverse by block forward substitution on R = I in right-looking
    form.  D: only its lower triangle is read.  Returns (L lower with exact zeros above the diagonal of its diagonal
    16-tiles, L^-1, [failing local columns, 1-based, one per 16-block that failed])."""
    T = np.tril(D) + np.tril(D, -1).T
    Y, R, reports = np.zeros((TILE, TILE)), np.eye(TILE), []
    for kb in range(8):
        c = slice(16 * kb, 16 * kb + 16)
        below = slice(16 * kb + 16, TILE)
        Lkk, Dinv, bad = potrf16(T[c, c])
        if bad < 16:
            reports.append(16 * kb + bad + 1)
        T[c, c] = np.tril(Lkk)
        done = slice(0, 16 * kb + 16)
        Y[c, done] = Dinv @ R[c, done]                 # phase A (and the diagonal inverse itself: R[c, c] = I)
        if kb < 7:
            P = T[below, c] @ Dinv.T                   # P := P inv(D)^T
            T[below, c] = P
            T[below, below] -= P @ P.T                 # the upper half is never read again
            R[below, done] -= P @ Y[c, done]           # phase B
    return np.tril(T), np.tril(Y), reports


def blocked_factor_panel(M, W, inv, col0):
    """gpak_factor_panel of csrc/potrf.hip in float64 on M = rows [J, Np) of the block column (a view, written in place):
    pieces of PANEL_MID columns, inside them 128-column steps (potrf128, P := P inv^T, the K = 128 update of the rest of
    the piece), after each piece the K = piece update of the rest of the panel -- lower 128-tiles only, the 16-tiles above
    the diagonal of a diagonal 128-block neither read nor written.  inv: (W / 128, 2, 128, 128) view, both images written
    whole.  Returns the failing columns reported (1-based, global through col0), in launch order: *info gets their
    minimum (atomicMin)."""
    rows = M.shape[0]
    reports = []

    def update(c0, c1, k0, k1):
        """columns [c0, c1) -= P[:, k0:k1] P[c0:c1, k0:k1]^T for the rows from c0 on, lower 128-tiles"""
        for t0 in range(c0, c1, TILE):
            M[t0:, t0:t0 + TILE] -= M[t0:, k0:k1] @ M[t0:t0 + TILE, k0:k1].T

    for p0 in range(0, W, PANEL_MID):
        p1 = min(W, p0 + PANEL_MID)
        for j in range(p0, p1, TILE):
            blk = M[j:j + TILE, j:j + TILE]
            L, X, rep = potrf128(blk)
            reports += [col0 + j + r for r in rep]
            keep = np.kron(np.triu(np.ones((8, 8), dtype=bool), 1), np.ones((16, 16), dtype=bool))
            blk[...] = np.where(keep, blk, L)
            iv = inv[j // TILE]
            iv[0] = X.T                                # memory [c][r] of L^-1 (column-major, ld 128)
            iv[1] = X                                  # ... of L^-T
            if j + TILE < rows:
                M[j + TILE:, j:j + TILE] = M[j + TILE:, j:j + TILE] @ X.T
                if j + TILE < p1:
                    update(j + TILE, p1, j, j + TILE)
        if p1 < W and p1 < rows:
            update(p1, W, p0, p1)
    return reports


class NumpyEngine:
    def empty(self, n, dtype=None):
        return torch.zeros(int(n), dtype=dtype or torch.float64)

    zeros = empty

    def from_numpy(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).copy())

    def sync(self):
        pass

    @staticmethod
    def _A(expans):
        from oracle import oracle as orc
        par = [expans[0], expans[2], expans[4], expans[1], expans[3], expans[5]]
        return orc.siginv(par)

    def transform(self, x_soa, xs, n, cap, expans, mu, u):
        # FOUR raw columns (include/gpak_dev.h): the 4th is zero for 3-D inputs, its image u3 = InversewidthR * (x3 - mu3)
        X4 = x_soa.numpy().reshape(4, xs)[:, :n].T
        mu = list(mu) + [0.0] * (4 - len(mu))
        U = (X4[:, :3] - np.asarray(mu[:3])[None, :]) @ self._A(expans)
        u3 = expans[7] * (X4[:, 3] - mu[3])
        un = self._un(u, cap)
        un[:5] = 0
        un[:3, :n] = U.T
        un[4, :n] = u3
        un[3, :n] = (U * U).sum(1) + u3 * u3

    @staticmethod
    def decode_kern(kern):
        """gpak_dev.h GPAK_DIST_HYB serialization -> (terms [(kind, params)], white)."""
        n = int(kern[0])
        kinds = [int(kern[1 + t]) for t in range(n)]
        terms, p = [], 5
        for k in kinds:
            m = {0: 8, 1: 2, 2: 3}[k]
            terms.append((k, [float(kern[p + i]) for i in range(m)]))
            p += m
        return terms, float(kern[4])

    def transform_k(self, x_soa, xs, n, cap, kern, mode, mu, u):
        """5 arrays per child: ExpAns -> (x - mu) sigInv and InversewidthR * x3; Exp / RBF -> every column / Hayper."""
        if not mode & 0x20:
            return self.transform(x_soa, xs, n, cap, kern, mu, u)
        terms, _ = self.decode_kern(kern)
        X4 = x_soa.numpy().reshape(4, xs)[:, :n].T
        mu = np.asarray(list(mu) + [0.0] * (4 - len(mu)))
        un = self._un(u, cap)[:15].reshape(3, 5, cap)
        un[:] = 0
        for t, (kind, p) in enumerate(terms):
            if kind == 0:
                U3 = (X4[:, :3] - mu[None, :3]) @ self._A(p)
                u3 = p[7] * (X4[:, 3] - mu[3])
            else:
                U3 = (X4[:, :3] - mu[None, :3]) / p[0]
                u3 = (X4[:, 3] - mu[3]) / p[0]
            un[t, :3, :n] = U3.T
            un[t, 4, :n] = u3
            un[t, 3, :n] = (U3 * U3).sum(1) + u3 * u3

    @classmethod
    def _kfun(cls, un, rows, cols, expans, bias, mode):
        if mode & 0x20:                   # GPAK_DIST_HYB: `expans` is the serialized composition, un has 5 arrays per child
            terms, _white = cls.decode_kern(expans)
            cap = un.shape[1]
            unt = un[:15].reshape(3, 5, cap)
            K = np.full((len(range(*rows.indices(cap))), len(range(*cols.indices(cap)))), float(bias))
            for t, (kind, p) in enumerate(terms):
                sel = [0, 1, 2, 4] if mode & 0x10 else [0, 1, 2]
                P, Q = unt[t][sel][:, rows].T, unt[t][sel][:, cols].T
                if (mode & 0xF) == 1:
                    D2 = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
                else:
                    D2 = unt[t][3, rows][:, None] + unt[t][3, cols][None, :] - 2 * P @ Q.T
                    D2[D2 < 0] = 0
                if kind == 2:
                    K += p[2] ** 2 * np.exp(-0.5 * p[1] * D2)
                else:
                    K += (p[6] if kind == 0 else p[1]) ** 2 * np.exp(-np.sqrt(D2))
            return K
        d4 = bool(mode & 0x10)            # GPAK_DIST_D4: the transformed 4th column takes part in the distance
        mode &= 0xF
        sel = [0, 1, 2, 4] if d4 else [0, 1, 2]
        P, Q = un[sel][:, rows].T, un[sel][:, cols].T
        if mode == 1:
            D2 = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
        else:
            D2 = un[3, rows][:, None] + un[3, cols][None, :] - 2 * P @ Q.T
            D2[D2 < 0] = 0
        return expans[6] ** 2 * np.exp(-np.sqrt(D2)) + bias

    @staticmethod
    def _un(u, cap):
        """the transformed points as (arrays x cap): 5 arrays, or 15 when the buffer holds a composition's three children"""
        a = u.numpy()
        rows = a.size // cap
        return a[:rows * cap].reshape(rows, cap)

    def fill_b(self, u, cap, n, Np, J, W, expans, bias, sn2, mode, blk, ld):
        un = self._un(u, cap)
        M = blk.numpy().reshape(W, ld).T  # (ld x W) column-major view
        # gpak_dev.h: the LOWER tiles; a 128-tile strictly above the diagonal keeps what it held
        upper = [(tj, M[:J + tj * TILE, tj * TILE:(tj + 1) * TILE].copy()) for tj in range(W // TILE)]
        M[:Np, :] = 0
        nc = max(0, min(W, n - J))
        if nc > 0:
            M[:n, :nc] = self._kfun(un, slice(0, n), slice(J, J + nc), expans, bias, mode) / sn2
        white = self.decode_kern(expans)[1] if mode & 0x20 else 0.0     # Kern_White: Sigma_White on the diagonal
        for c in range(W):
            M[J + c, c] += 1.0 + (white / sn2 if J + c < n else 0.0)
        for tj, keep in upper:
            M[:J + tj * TILE, tj * TILE:(tj + 1) * TILE] = keep

    def factor_panel(self, blk, ld, Np, J, W, inv, info):
        M = blk.numpy().reshape(W, ld).T
        reports = blocked_factor_panel(M[J:Np], W, inv.numpy().reshape(W // TILE, 2, TILE, TILE), J)
        if reports:                                    # the first failing column, 1-based and global: atomicMin
            info[0] = min(int(info[0]), min(reports))

    def pack(self, src, ld, row0, nrows, ncols, dst):
        dst.view(ncols, nrows).copy_(src.view(ncols, ld)[:, row0:row0 + nrows])

    def update_block(self, panel, ldp, prow0, W, blk, ld, Np, Jc, Wc):
        P = panel.numpy().reshape(W, ldp).T
        C = blk.numpy().reshape(Wc, ld).T
        a = P[Jc - prow0:Np - prow0, :]
        upd = a @ a[:Wc, :].T
        for tj in range(Wc // TILE):   # gpak_dev.h: lower tiles only; a tile strictly above the diagonal is not written
            upd[:tj * TILE, tj * TILE:(tj + 1) * TILE] = 0.0
        C[Jc:Np, :] -= upd

    def update_cyclic(self, panel, ldp, prow0, W, local, ld, Np, nb, P, rank, lb0, n_local, last_width):
        for lb in range(lb0, n_local):
            Wc = last_width if lb == n_local - 1 else nb
            Jc = (lb * P + rank) * nb
            blk = local[lb * nb * ld: lb * nb * ld + Wc * ld]
            self.update_block(panel, ldp, prow0, W, blk, ld, Np, Jc, Wc)

    # row0: global row held in element 0 of each column (0: full block column; J: packed panel from its diagonal)
    def trsv_fwd_block(self, blk, ld, Np, J, W, inv, x, out, row0=0):
        M = self._rows_from(blk, W, ld, row0, Np)
        iv = inv.numpy().reshape(W // TILE, 2, TILE, TILE)
        xn, on = x.numpy(), out.numpy()
        for k in range(W // TILE):
            j0 = J + k * TILE
            z = iv[k, 0].T @ xn[j0:j0 + TILE]
            on[j0:j0 + TILE] = z
            xn[j0 + TILE:Np] -= M[j0 + TILE:Np, k * TILE:(k + 1) * TILE] @ z

    @staticmethod
    def _rows_from(blk, W, ld, row0, Np):
        """(Np x W) view-like array addressed by GLOBAL row; rows above row0 are never read by the callers."""
        M = blk.numpy().reshape(W, ld).T
        if row0 == 0:
            return M
        full = np.zeros((Np, W))
        full[row0:Np] = M[:Np - row0]
        return full

    def coldot(self, blk, ld, Np, J, W, x, s, row0=0):
        M = self._rows_from(blk, W, ld, row0, Np)
        s.numpy()[:W] = M[J + W:Np, :].T @ x.numpy()[J + W:Np]

    def trsv_bwd_block(self, blk, ld, J, W, inv, x, out, row0=0):
        M = self._rows_from(blk, W, ld, row0, J + W)
        iv = inv.numpy().reshape(W // TILE, 2, TILE, TILE)
        xn, on = x.numpy(), out.numpy()
        for k in range(W // TILE - 1, -1, -1):
            j0 = J + k * TILE
            w = iv[k, 1].T @ xn[j0:j0 + TILE]      # inv(L_jj)^T x_j
            on[j0:j0 + TILE] = w
            if k > 0:
                xn[J:j0] -= M[j0:j0 + TILE, :k * TILE].T @ w

    def trsv_bwd_packed(self, panel, ldp, row0, Np, J, W, inv, z, scratch, out, rinv=None):
        s = torch.zeros(W, dtype=torch.float64)
        if J + W < Np:
            self.coldot(panel, ldp, Np, J, W, out, s, row0=row0)
        v = z.clone()
        v[J:J + W] -= s
        self.trsv_bwd_block(panel, ldp, J, W, inv, v, out, row0=row0)

    def logdiag_block(self, blk, ld, J, W, N, out):
        M = blk.numpy().reshape(W, ld).T
        nc = max(0, min(W, N - J))
        out[0] = float(np.log(np.diag(M[J:J + nc, :nc])).sum()) if nc else 0.0

    def kmatvec(self, u, cap, n, i0, i1, w, expans, bias, mode, scratch, out):
        un = self._un(u, cap)
        K = self._kfun(un, slice(i0, i1), slice(0, n), expans, bias, mode)
        out.numpy()[:n] = w.numpy()[i0:i1] @ K

    def nlz_terms(self, N, y, f, alpha, sn2, out):
        yn, fn, an = y.numpy()[:N], f.numpy()[:N], alpha.numpy()[:N]
        out[0] = float((an * 0.5 * fn).sum())
        out[1] = float((-(yn - fn) ** 2 / (2 * sn2) - np.log(2 * np.pi * sn2) / 2).sum())
