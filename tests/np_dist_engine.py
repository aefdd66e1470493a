"""Callback tables for gpak_dist_create (include/gpak_dist.h) on a box WITHOUT a GPU -- TEST INFRASTRUCTURE ONLY.

`NumpyDistEngine.table` is a gpak_dist_engine whose "device" buffers are host arrays and whose tile operations are
NumPy/SciPy restatements of include/gpak_dev.h (tests/np_engine.py, written against the same header);
`GlooTransport.table` is a gpak_dist_transport over a torch.distributed (gloo) group.  With them the world_size-2/3/4
CPU tests drive the C++ schedule of csrc/dist.hip itself: ownership map, look-ahead order, sub-panel broadcasts,
the solves on packed panels and the reductions.
"""
import ctypes as C

import numpy as np
import torch

from gp_ss_ak_amd import dist as gd
from np_engine import NumpyEngine, TILE, blocked_factor_panel


def _arr(ptr, n, dtype=np.float64):
    ct = C.c_double if dtype == np.float64 else C.c_int32
    return np.ctypeslib.as_array((ct * int(n)).from_address(int(ptr)))


def _t(ptr, n, dtype=np.float64):
    return torch.from_numpy(_arr(ptr, n, dtype))


def _strided(ptr, rows, cols, ld):
    """(rows x cols) column-major view with leading dimension ld starting at ptr."""
    base = _arr(ptr, (cols - 1) * ld + rows)
    return np.lib.stride_tricks.as_strided(base, shape=(rows, cols), strides=(8, 8 * ld))


def grad_consts(e):
    """M_p (6 x 3 x 3) and m2 (6 x 3) of the as-written pass, from the library (host code: gpak_dev_grad_consts)"""
    lib = gd._load()
    e = np.ascontiguousarray(e, dtype=np.float64)
    M36, m2 = np.zeros(36), np.zeros(18)
    lib.gpak_dev_grad_consts.argtypes = [gd._dp, gd._dp, gd._dp]
    lib.gpak_dev_grad_consts(e.ctypes.data_as(gd._dp), M36.ctypes.data_as(gd._dp), m2.ctypes.data_as(gd._dp))
    Mp = np.zeros((6, 3, 3))
    for p in range(6):
        v = M36[6 * p:6 * p + 6]
        Mp[p] = [[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]]
    return Mp, m2.reshape(6, 3)


def decode_composition(kern, mode):
    """`kern` of a gpak_dev_* call -> (terms [(kind, params)], white): the serialisation of gpak_dev.h under
    GPAK_DIST_HYB, the plain ExpAns list otherwise"""
    if mode & 0x20:
        return NumpyEngine.decode_kern(kern)
    return [(0, [float(kern[i]) for i in range(8)])], 0.0


def pair_rows(Np, P, a):
    """global rows of rank a's 128-row blocks in slab order (P == 0: every row)"""
    T = Np // TILE
    if P == 0:
        return np.arange(Np)
    Ta = (T - a + P - 1) // P if T > a else 0
    return (np.arange(Ta)[:, None] * P * TILE + a * TILE + np.arange(TILE)[None, :]).ravel().astype(int)


def pair_sums(passno, u, cap, x_soa, xs, n, Np, alpha, binv, ld, P, a, kern, bias, sn2, mode, out, mut=()):
    """gpak_dev_grad_pair_sums in float64 on host arrays: out[0..16) <- the sums of pass 0 (as written: the comment above
    RefPass in csrc/grad.hip) or 1 (exact: above ExactPass) over the pairs i >= j of the rows this call owns.  `mut`:
    deliberate faults, for tests that prove a check bites (tests/test_dev_ops.py)."""
    terms, _white = decode_composition(kern, mode)
    nt = len(terms)
    d4, mode = bool(mode & 0x10), mode & 0xF
    un = u[:5 * nt * cap].reshape(nt, 5, cap)
    X4 = x_soa[:4 * xs].reshape(4, xs)[:, :n].T
    al = alpha[:n]
    rows = pair_rows(Np, P, a)
    loc = np.arange(len(rows))[rows < n]
    rows = rows[rows < n]
    out[:16] = 0.0
    if not len(rows):
        return
    cols = np.arange(n)
    if P == 0:
        Q = np.lib.stride_tricks.as_strided(binv, shape=(n, n), strides=(8, 8 * ld))
    else:
        Ta, Tmax = len(pair_rows(Np, P, a)), len(pair_rows(Np, P, 0)) // TILE
        cperm = ((cols // TILE % P) * Tmax + cols // TILE // P) * TILE + cols % TILE
        if "unpermuted" in mut:
            cperm = cols
        Q = binv[:Ta * P * Tmax * TILE].reshape(P * Tmax * TILE, Ta).T[loc][:, cperm]
    low = rows[:, None] >= cols[None, :]
    diag = rows[:, None] == cols[None, :]
    if "last row" in mut:
        low = low & (rows[:, None] != n - 1)
    if "upper" in mut:
        low = low.copy()
        low[0, rows[0] + 1] = True                         # one element with i < j
    wgt = np.where(diag, 2.0 if "diag2" in mut else 1.0, 2.0) * low
    Qm = np.where(low, Q, 0.0)
    ali = al[rows][:, None]
    QW = np.where(low, Qm * (1.0 / sn2) - ali * (ali if "alpha row" in mut else al[None, :]), 0.0)
    sel = [0, 1, 2, 4]                                     # the 4th transformed coordinate is 0 for 3-column inputs

    def dist2(m, direct):
        Pu, Qu = un[m][sel][:, rows].T, un[m][sel][:, :n].T
        if direct:
            return ((Pu[:, None, :] - Qu[None, :, :]) ** 2).sum(-1)
        return np.maximum(un[m][3, rows][:, None] + un[m][3, :n][None, :] - 2 * Pu @ Qu.T, 0.0)

    def dk_of(sd, ek):
        zero = diag if "dk" in mut else (sd == 0) | diag
        return np.where(zero, 0.0, ek * (-0.5 / sd))

    te = [k for k, _ in terms].index(0) if 0 in [k for k, _ in terms] else -1
    acc = np.zeros(16)
    with np.errstate(divide="ignore", invalid="ignore"):
        if passno == 0:
            d2 = [dist2(m, mode == 1) for m in range(nt)]
            d2s = sum(d2)
            kfull = bias + sum((p[2] ** 2 * np.exp(-0.5 * p[1] * d2[m])) if k == 2 else
                               ((p[6] if k == 0 else p[1]) ** 2 * np.exp(-np.sqrt(d2[m]))) for m, (k, p) in enumerate(terms))
            acc[7] = (wgt * Qm * kfull).sum()
            acc[8] = (QW * diag).sum()
            if te >= 0:
                e = np.asarray(terms[te][1])
                Mp, m2 = grad_consts(e)
                X = X4[:, :3]
                sd = np.sqrt(d2[te])
                ek = np.exp(-sd)
                rm = e[6] ** 2 * QW * dk_of(sd, ek)
                for p in range(6):
                    pa_i, pa_j = (X[rows] ** 2) @ m2[p], (X ** 2) @ m2[p]
                    di2 = pa_i[:, None] + pa_j[None, :] - 4.0 * (X[rows] @ Mp[p] @ X.T)
                    acc[p] = (wgt * rm * di2).sum()
                acc[6] = (wgt * QW * ek).sum()
                dx = (X4[rows, 3][:, None] - X4[:, 3][None, :]) if d4 else np.zeros_like(sd)
                acc[15] = (wgt * ek * dx * dx).sum()
            for m, (k, p) in enumerate(terms):
                if k == 1:       # Kern_Exponential on the summed D2
                    sd = np.sqrt(d2s)
                    kd = np.exp(-sd)
                    acc[9 + 2 * m] = (wgt * QW * dk_of(sd, kd) * d2s).sum()
                    acc[10 + 2 * m] = (wgt * QW * kd * kd).sum()
                elif k == 2:     # Kern_RBF on the summed D2
                    kd = np.exp(-0.5 * p[1] * d2s)
                    acc[9 + 2 * m] = (wgt * QW * kd * d2s).sum()
                    acc[10 + 2 * m] = (wgt * QW * kd).sum()
        else:
            W = wgt * QW
            acc[0] = W.sum()
            acc[1] = (QW * diag).sum()
            for m, (k, p) in enumerate(terms):
                d2 = dist2(m, True)
                if k == 2:
                    we = W * np.exp(-0.5 * p[1] * d2)
                    acc[2 + m] = we.sum()
                    acc[5 + m] = (we * d2).sum()
                    continue
                sd = np.sqrt(d2)
                ek = np.exp(-sd)
                wdk = W * dk_of(sd, ek)
                acc[2 + m] = (W * ek).sum()
                if m == te:
                    D = [X4[rows, c][:, None] - X4[:, c][None, :] for c in range(4)]
                    if not d4:
                        D[3] = np.zeros_like(sd)
                    for s, (ca, cb) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                        acc[8 + s] = (wdk * D[ca] * D[cb]).sum()
                    acc[14] = (wdk * D[3] * D[3]).sum()
                else:
                    acc[5 + m] = (wdk * d2).sum()
    if "swap 9 10" in mut:
        acc[[9, 10]] = acc[[10, 9]]
    out[:16] = acc + 0.0                                   # -0.0 + 0.0 = +0.0: an unused slot is +0.0 as on the device


class NumpyDistEngine:
    def __init__(self, poison_upper=True):
        """poison_upper: a diagonal fill_rect piece gets NaN in the tiles above its diagonal, which the device leaves as
        they were (gpak_dev.h) -- so that a schedule that READS them shows; False restates the device exactly."""
        self.np = NumpyEngine()
        self.mem = {}
        self.calls = []          # (operation, stream) in issue order, for schedule assertions
        eng = self.np
        F = dict(gd.ENGINE_FIELDS)

        def ok(fn):
            def wrapped(*a):
                fn(*a)
                return 0
            return wrapped

        def alloc(_s, nbytes):
            a = np.zeros(max(1, (int(nbytes) + 7) // 8), dtype=np.float64)
            self.mem[a.ctypes.data] = a
            return a.ctypes.data

        def release(_s, p):
            self.mem.pop(int(p), None)

        def upload(_s, st, dst, src, nbytes):
            C.memmove(dst, src, nbytes)

        def zero(_s, st, dst, nbytes):
            C.memset(dst, 0, nbytes)

        def elapsed(_s, e0, e1, ms):
            ms[0] = 0.0

        def transform(st, x, xs, n, cap, expans, mu, u):
            eng.transform(_t(x, 4 * xs), xs, n, cap, [expans[i] for i in range(8)], [mu[i] for i in range(4)], _t(u, 15 * cap))

        def fill_b(st, u, cap, n, Np, J, W, expans, bias, sn2, mode, blk, ld):
            eng.fill_b(_t(u, 15 * cap), cap, n, Np, J, W, [expans[i] for i in range(32 if mode & 0x20 else 8)], bias, sn2, mode,
                       _t(blk, W * ld), ld)

        def factor_panel(st, blk, ld, Np, J, W, inv, info):
            # rows J .. Np of the block column through a strided view: `blk` may be a VIRTUAL base (the grid layout passes
            # block - J so that global row J is the block's first local row), which a reshape by ld cannot address
            self.calls.append(("factor", J, st))
            M = _strided(int(blk) + 8 * J, Np - J, W, ld)
            reports = blocked_factor_panel(M, W, inv_blocks(inv, W), J)
            self.last_reports = reports                # launch order: what a last-writer-wins report would keep
            if reports:
                infon = _arr(info, 1, np.int32)
                infon[0] = min(int(infon[0]), min(reports))

        def update_block(st, panel, ldp, prow0, W, blk, ld, Np, Jc, Wc):
            self.calls.append(("update_block", Jc, st))
            eng.update_block(_t(panel, W * ldp), ldp, prow0, W, _t(blk, Wc * ld), ld, Np, Jc, Wc)

        def update_cyclic(st, panel, ldp, prow0, W, local, ld, Np, nb, P, rank, lb0, n_local, last_width):
            self.calls.append(("update_cyclic", lb0, st))
            eng.update_cyclic(_t(panel, W * ldp), ldp, prow0, W, _t(local, ((n_local - 1) * nb + last_width) * ld), ld, Np,
                              nb, P, rank, lb0, n_local, last_width)

        def inv_blocks(inv, W):
            return _arr(inv, W // TILE * 2 * TILE * TILE).reshape(W // TILE, 2, TILE, TILE)

        def trsv_fwd_block(st, blk, ld, Np, J, W, inv, x, out):
            # gpak_dev.h: L[r, J+k] = blk[r + k*ld] for r >= J
            M = _strided(int(blk) + 8 * J, Np - J, W, ld)
            iv, xn, on = inv_blocks(inv, W), _arr(x, Np), _arr(out, Np)
            for k in range(W // TILE):
                j0 = J + k * TILE
                z = iv[k, 0].T @ xn[j0:j0 + TILE]
                on[j0:j0 + TILE] = z
                xn[j0 + TILE:Np] -= M[j0 + TILE - J:, k * TILE:(k + 1) * TILE] @ z

        def trsv_bwd_packed(st, panel, ldp, row0, Np, J, W, inv, z, scratch, out, rinv):
            M = _strided(panel, Np - row0, W, ldp)
            iv, zn, on = inv_blocks(inv, W), _arr(z, Np), _arr(out, Np)
            v = zn[J:J + W].copy()
            if J + W < Np:
                v -= M[J + W - row0:, :].T @ on[J + W:Np]
            if rinv:
                R = _strided(rinv, W, W, 512)
                on[J:J + W] = R @ v                       # R = (L_bb^-1)^T
                return
            for k in range(W // TILE - 1, -1, -1):
                j0 = J + k * TILE
                w = iv[k, 1].T @ v[k * TILE:(k + 1) * TILE]
                on[j0:j0 + TILE] = w
                if k > 0:
                    v[:k * TILE] -= M[j0 - row0:j0 - row0 + TILE, :k * TILE].T @ w

        def diag_inverse(st, panel, ldp, row0, J, W, inv, rinv):
            M = _strided(panel, W + (J - row0), W, ldp)
            L = np.tril(M[J - row0:J - row0 + W, :])
            try:
                _strided(rinv, W, W, 512)[:] = np.linalg.inv(L).T
            except np.linalg.LinAlgError:
                # only after a FAILED factorisation, which the schedules run to the end: what follows the failing column is
                # garbage on the device too (a failed pivot is replaced by 1 and the arithmetic goes on; it may overflow)
                _strided(rinv, W, W, 512)[:] = np.nan

        def logdiag_block(st, blk, ld, J, W, N, out):
            nc = max(0, min(W, N - J))
            M = _strided(int(blk) + 8 * J, W, W, ld)
            _arr(out, 1)[0] = float(np.log(np.diag(M)[:nc]).sum()) if nc else 0.0

        def kmatvec(st, u, cap, n, i0, i1, w, expans, bias, mode, scratch, out):
            eng.kmatvec(_t(u, 15 * cap), cap, n, i0, i1, _t(w, cap), [expans[i] for i in range(32 if mode & 0x20 else 8)], bias, mode, None,
                        _t(out, cap))

        def nlz_terms(st, N, y, f, alpha, sn2, out):
            eng.nlz_terms(N, _t(y, N), _t(f, N), _t(alpha, N), sn2, _t(out, 2))

        def pack(st, src, ld, row0, nrows, ncols, dst):
            _strided(dst, nrows, ncols, nrows)[:] = _strided(int(src) + 8 * row0, nrows, ncols, ld)

        # ---- distributed gradient (gpak_dev_grad_*): dense restatements on the reconstructed factor ----------
        def my_tiles(Np, P, a):
            T = Np // TILE
            return (T - a + P - 1) // P if T > a else 0

        def my_rows(Np, P, a):
            return np.concatenate([np.arange((t * P + a) * TILE, (t * P + a + 1) * TILE) for t in range(my_tiles(Np, P, a))]
                                  or [np.zeros(0, dtype=int)]).astype(int)

        def grad_g_rows(st, Np, nb, P, a, panels, invs, slab):
            L = np.zeros((Np, Np))
            for b, J in enumerate(range(0, Np, nb)):
                W = min(nb, Np - J)
                L[J:, J:J + W] = _strided(panels[b], Np - J, W, Np - J)
            G = np.linalg.inv(np.tril(L)).T
            rows = my_rows(Np, P, a)
            if len(rows):
                _strided(slab, len(rows), Np, len(rows))[:] = G[rows, :]

        def grad_binv_rows(st, Np, P, a, b, slab_a, slab_b, binv):
            rows, rb, Tmax = my_rows(Np, P, a), my_rows(Np, P, b), my_tiles(Np, P, 0)
            if not len(rows) or not len(rb):
                return
            Ga = _strided(slab_a, len(rows), Np, len(rows))
            Gb = _strided(slab_b, len(rb), Np, len(rb))
            Bi = Ga @ Gb.T                                           # my rows of B^-1 = G G^T, columns of rank b
            out = _strided(binv, len(rows), P * Tmax * TILE, len(rows))
            for u in range(len(rb) // TILE):
                c0 = (b * Tmax + u) * TILE
                out[:, c0:c0 + TILE] = Bi[:, u * TILE:(u + 1) * TILE]

        def grad_pairs_rows(st, u, cap, x_soa, xs, n, Np, y, f, alpha, binv, P, a, expans, bias, sn2, mode, part, out):
            Ta, Tmax = my_tiles(Np, P, a), my_tiles(Np, P, 0)
            acc = np.zeros(17)
            pair_sums(0, _arr(u, 5 * cap), cap, _arr(x_soa, 4 * xs), xs, n, Np, _arr(alpha, n),
                      _arr(binv, max(Ta, 1) * TILE * P * Tmax * TILE), 0, P, a, [expans[i] for i in range(8)], bias, sn2,
                      mode & ~0x20, acc[:16])
            yn, fn = _arr(y, n), _arr(f, n)
            acc[16] = float(((yn - fn) ** 2 / sn2 - 1.0).sum())
            _arr(out, 17)[:] = acc

        # ---- the row-block x column-block layout (gpak_grid_*): rectangular pieces of LOCAL storage -------------
        def fill_rect(st, u, cap, n, row0, nrows, col0, ncols, expans, bias, sn2, mode, dst, ld):
            un = _arr(u, 15 * cap).reshape(15, cap)
            D = _strided(dst, nrows, ncols, ld)
            upper = [(tj, D[:tj * TILE, tj * TILE:(tj + 1) * TILE].copy()) for tj in range(ncols // TILE)]
            D[:] = 0.0
            r1, c1 = min(n, row0 + nrows), min(n, col0 + ncols)
            ex = [expans[i] for i in range(32 if mode & 0x20 else 8)]
            if r1 > row0 and c1 > col0:
                D[:r1 - row0, :c1 - col0] = eng._kfun(un, slice(row0, r1), slice(col0, c1), ex, bias, mode) / sn2
            white = eng.decode_kern(ex)[1] if mode & 0x20 else 0.0     # Kern_White: Sigma_White on the diagonal
            for a in range(nrows):
                c = row0 + a - col0
                if 0 <= c < ncols:
                    D[a, c] += 1.0 + (white / sn2 if row0 + a < n else 0.0)
            if row0 == col0:                      # a diagonal piece: only its lower 128-tiles are written
                for tj, keep in upper:
                    D[:tj * TILE, tj * TILE:(tj + 1) * TILE] = np.nan if poison_upper else keep

        def solve_rows(st, P, ld, nrows, W, Lbb, ldl, inv):
            import scipy.linalg as sl
            Pm = _strided(P, nrows, W, ld)
            L = np.tril(_strided(Lbb, W, W, ldl))
            Pm[:] = sl.solve_triangular(L, Pm.T, lower=True).T

        def update_rect(st, A, lda, B, ldb, K, Cp, ldc, mrows, ncols, diag_first):
            self.calls.append(("update_rect", ncols, st))
            Am, Bm, Cm = _strided(A, mrows, K, lda), _strided(B, ncols, K, ldb), _strided(Cp, mrows, ncols, ldc)
            upd = Am @ Bm.T
            if diag_first:
                for tj in range(ncols // TILE):
                    upd[:tj * TILE, tj * TILE:(tj + 1) * TILE] = 0.0     # tiles strictly above the diagonal: untouched
            Cm -= upd

        def gemv_n_add(st, A, ld, nrows, W, x, y):
            if nrows > 0:
                _arr(y, nrows)[:] += _strided(A, nrows, W, ld) @ _arr(x, W)

        def gemv_t(st, A, ld, nrows, W, x, y):
            _arr(y, W)[:] = _strided(A, nrows, W, ld).T @ _arr(x, nrows) if nrows > 0 else 0.0

        def vec_axpy(st, n, a, x, y):
            _arr(y, n)[:] += a * _arr(x, n)

        def transform_k(st, x, xs, n, cap, kern, mode, mu, u):
            eng.transform_k(_t(x, 4 * xs), xs, n, cap, [kern[i] for i in range(32)], mode, [mu[i] for i in range(4)],
                            _t(u, 15 * cap))

        def vec_scale(st, n, a, s, out):
            _arr(out, n)[:] = _arr(a, n) * s

        def vec_sum(st, n, a, out):
            _arr(out, 1)[0] = float(np.sum(_arr(a, n)))

        impl = {
            "alloc": alloc, "release": release, "upload": ok(upload), "download": ok(upload), "zero": ok(zero),
            "copy": ok(upload), "stream_create": lambda _s, kind: 100 + kind, "stream_destroy": lambda _s, st: None,
            "event_create": lambda _s, timing: 1, "event_destroy": lambda _s, e: None, "event_record": lambda *a: 0,
            "stream_wait_event": lambda *a: 0, "stream_sync": lambda *a: 0, "event_elapsed_ms": ok(elapsed),
            "transform": ok(transform), "fill_b": ok(fill_b), "factor_panel": ok(factor_panel),
            "update_block": ok(update_block), "update_cyclic": ok(update_cyclic), "trsv_fwd_block": ok(trsv_fwd_block),
            "trsv_bwd_packed": ok(trsv_bwd_packed), "diag_inverse": ok(diag_inverse), "logdiag_block": ok(logdiag_block),
            "kmatvec": ok(kmatvec), "nlz_terms": ok(nlz_terms), "pack": ok(pack), "vec_scale": ok(vec_scale),
            "vec_sum": ok(vec_sum), "grad_g_rows": ok(grad_g_rows), "grad_binv_rows": ok(grad_binv_rows),
            "grad_pairs_rows": ok(grad_pairs_rows), "fill_rect": ok(fill_rect), "solve_rows": ok(solve_rows),
            "update_rect": ok(update_rect), "gemv_n_add": ok(gemv_n_add), "gemv_t": ok(gemv_t), "vec_axpy": ok(vec_axpy),
            "transform_k": ok(transform_k),
        }
        self._keep = {name: F[name](fn) for name, fn in impl.items()}
        self.table = gd.Engine(None, *[self._keep[name] for name, _ in gd.ENGINE_FIELDS[1:]])


class GlooTransport:
    """gpak_dist_transport over a gloo group for HOST buffers (the NumPy engine's memory)."""

    def __init__(self, group=None, corrupt_first=0):
        """corrupt_first: flip one word of the first k broadcasts AFTER delivery (on the receivers) -- what a broken
        side-stream collective would look like to the start-up self-check."""
        import torch.distributed as dist
        self.bytes = 0
        self.n_bcast = 0

        def bcast(_s, st, buf, count, root):
            self.bytes += 8 * int(count)
            t = _t(buf, count)
            dist.broadcast(t, src=root, group=group)
            self.n_bcast += 1
            if self.n_bcast <= corrupt_first and dist.get_rank(group) != root:
                t[int(count) // 2] += 1.0
            return 0

        def ar_sum(_s, st, buf, count):
            dist.all_reduce(_t(buf, count), group=group)
            return 0

        def ar_min(_s, st, buf, count):
            dist.all_reduce(_t(buf, count, np.int32), op=dist.ReduceOp.MIN, group=group)
            return 0

        self.groups = {}
        self.group_bytes = 0

        def grid_setup(_s, Pr, Pc):
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            if Pr * Pc != world:
                return 2
            pr, pc = rank % Pr, rank // Pr
            for r in range(Pr):                                   # new_group is collective over the world
                members = [r + Pr * c for c in range(Pc)]
                g = dist.new_group(members)
                if r == pr:
                    self.groups[1] = (g, members)
            for c in range(Pc):
                members = [r + Pr * c for r in range(Pr)]
                g = dist.new_group(members)
                if c == pc:
                    self.groups[2] = (g, members)
            return 0

        def bcast_g(_s, st, buf, count, root, grp):
            g, members = self.groups[grp]
            self.group_bytes += 8 * int(count)
            dist.broadcast(_t(buf, count), src=members[root], group=g)
            return 0

        def ar_sum_g(_s, st, buf, count, grp):
            g, _m = self.groups[grp]
            dist.all_reduce(_t(buf, count), group=g)
            return 0

        T = gd.Transport._fields_
        self._keep = (T[1][1](bcast), T[2][1](ar_sum), T[3][1](ar_min), T[4][1](grid_setup), T[5][1](bcast_g),
                      T[6][1](ar_sum_g))
        self.table = gd.Transport(None, *self._keep)
