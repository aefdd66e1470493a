"""Python face of the C-ABI (include/gpak.h), used by tests/, bench.py and the smoke test.

Method names follow the reference members they stand in for (GP_utils::logLikelihood,
GP_utils::posteriorMeanVar, Kernels::computeK, ...); every call goes through
libgpak_hip.so -- nothing is computed in Python.
"""
import ctypes as C
import math

import numpy as np

from . import _lib

OK, ENOTPD, EINVAL, ESTATE, ENOMEM, ENOTIMPL, EHIP = 0, 1, 2, 3, 4, 5, -1
F64, F32 = 0, 1
DIST_EXPANSION, DIST_DIRECT = 0, 1
COMPAT_VARCLAMP, COMPAT_SN2SKIP = 1, 2
OPT_MEMOISE, OPT_NB_OUTER, OPT_PROFILE, OPT_LOOKAHEAD = 1, 2, 3, 4
OPT_NB_WIDE, OPT_NB_WIDE_ROWS, OPT_TAIL_ROWS, OPT_FIRST_NARROW, OPT_INV512, OPT_POTRF_CO, OPT_PRED_BATCH = 5, 6, 7, 8, 9, 10, 11
OPT_BWD_FUSED = 12
OPT_TAIL_MAX_NP = 13
OPT_LOO_ROWS = 14
KERN_EXPANS, KERN_EXP, KERN_RBF = 0, 1, 2
BLOCK_LATENT = 1
JOINT_LATENT, JOINT_PRIOR = 1, 2
NO_BATCH = 1      # GPAK_CV_FOLDS_NO_BATCH
COND_UNFUSED = 1
LOCAL_LATENT, LOCAL_MAX = 1, 128

_dp = C.POINTER(C.c_double)


class GpakError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"gpak status {status}: {msg}")
        self.status = status


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def block_points(centres, size, disc):
    """Cell-centred discretisation of M rectangular blocks: returns (Xd, nd) for Gpak.predict_block / block_cross.

    centres is M x d (d = 3 or 4), size = (dx, dy, dz) the block's edge lengths, disc = (nx, ny, nz) the points per axis.
    Point (i, j, k) of a block sits at centre + (((i + 0.5) / nx - 0.5) dx, ((j + 0.5) / ny - 0.5) dy,
    ((k + 0.5) / nz - 0.5) dz); row b * nd + a of Xd is point a = (i * ny + j) * nz + k of block b (x slowest, z
    fastest).  A fourth column is copied from the centre."""
    c = np.asarray(centres, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError("centres must be M x 3 or M x 4")
    n = [int(v) for v in disc]
    if len(n) != 3 or len(size) != 3 or min(n) < 1:
        raise ValueError("size and disc take three values, disc positive counts")
    off = [((np.arange(n[k]) + 0.5) / n[k] - 0.5) * float(size[k]) for k in range(3)]
    nd = n[0] * n[1] * n[2]
    grid = np.stack(np.meshgrid(off[0], off[1], off[2], indexing="ij"), axis=-1).reshape(nd, 3)
    Xd = np.repeat(c, nd, axis=0)
    Xd[:, :3] = (c[:, None, :3] + grid[None, :, :]).reshape(-1, 3)
    return np.asfortranarray(Xd), nd


def group_labels(labels, n=None):
    """Any integer labels -> (group, values): group[i] in 0 .. G - 1 is the rank of labels[i] among the sorted unique
    values (int32, what gpak_cv_groups takes), values those G sorted labels.  Raises ValueError for labels that are not
    a one-dimensional integer array (of length n when n is given)."""
    a = np.asarray(labels)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise ValueError("labels must be a one-dimensional array of integers")
    if n is not None and a.size != int(n):
        raise ValueError(f"labels must hold one entry per training sample: {a.size} for {int(n)}")
    values, group = np.unique(a, return_inverse=True)
    return np.ascontiguousarray(group.reshape(-1), dtype=np.int32), values


def local_neighbours(Xs, Xc, k, G=None, radius=0.0, threads=0, octant=0):
    """The k nearest samples of every centre (gpak_local_neighbours; host code, no context): returns (nbr, used), nbr
    M x k int32 -- row b the sample indices of centre b by ascending distance |(x - c) G|, then ascending index, -1 in the
    unused slots -- and used (M) the counts.  G: d x d, or the 4 x 4 of Gpak.local_metric (its leading d x d part is
    taken), or None for the identity; radius > 0 keeps only samples within it; threads <= 0: min(cores, 16).
    octant > 0: the octant search (gpak_local_neighbours_octant) -- at most `octant` samples from each of the eight octants
    around a centre, of those the k nearest; it needs a positive radius and octant <= k."""
    Xs, Xc = _f(Xs), _f(Xc)
    if Xs.ndim != 2 or Xc.ndim != 2 or Xs.shape[1] != Xc.shape[1]:
        raise GpakError(EINVAL, "Xs and Xc must be matrices with as many columns")
    d, M, k = Xs.shape[1], Xc.shape[0], int(k)
    if G is not None:
        G = np.asarray(G, dtype=np.float64)
        if G.shape == (4, 4) and d == 3:
            G = G[:3, :3]
        if G.shape != (d, d):
            raise GpakError(EINVAL, "G must be d x d (or the 4 x 4 of local_metric)")
        G = np.asfortranarray(G)
    nbr = np.full((max(M, 0), max(k, 0)), -1, dtype=np.int32)
    used = np.zeros(max(M, 0), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    octant = int(octant)
    if octant < 0:
        raise GpakError(EINVAL, "octant is a count of samples per octant, or 0 for the plain search")
    if octant > 0:
        if not float(radius) > 0.0:
            raise GpakError(EINVAL, "the octant search needs a positive radius")
        rc = _lib.load().gpak_local_neighbours_octant(_p(Xs), Xs.shape[0], d, _p(Xc), M, _p(G), k, octant, float(radius),
                                                      int(threads), nbr.ctypes.data_as(ip), used.ctypes.data_as(ip))
        if rc != OK:
            raise GpakError(rc, "gpak_local_neighbours_octant refused its arguments (shapes, k outside 1..128, octant outside "
                                "1..k, a radius or a coordinate that is not finite)")
        return nbr, used
    rc = _lib.load().gpak_local_neighbours(_p(Xs), Xs.shape[0], d, _p(Xc), M, _p(G), k, float(radius), int(threads),
                                           nbr.ctypes.data_as(ip), used.ctypes.data_as(ip))
    if rc != OK:
        raise GpakError(rc, "gpak_local_neighbours refused its arguments (shapes, k outside 1..128, a coordinate that is not finite)")
    return nbr, used


class Gpak:
    """One context = one GPU. Mirrors the slice of GP_utils that sits on the hot path."""

    def __init__(self, device=0, precision=F64, devices=None):
        """devices: a list of HIP ordinals -> gpak_create_multi (one process driving several GPUs; an ordinal may
        repeat on a test box, the ranks then share that GPU)."""
        self._lib = _lib.load()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(v) for v in devices])
            rc = self._lib.gpak_create_multi(C.byref(h), len(devices), arr, precision)
        else:
            rc = self._lib.gpak_create(C.byref(h), device, precision)
        if rc != OK:
            raise GpakError(rc, self._lib.gpak_global_error().decode())
        self._h = h
        self.N = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpak_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, allow=()):
        if rc != OK and rc not in allow:
            raise GpakError(rc, self._lib.gpak_last_error(self._h).decode())
        return rc

    # -- state ---------------------------------------------------------------------------
    def set_option(self, opt, value):
        self._check(self._lib.gpak_set_option(self._h, opt, int(value)))

    def set_train(self, X, y):
        X = _f(X)
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        N, d = X.shape
        self._check(self._lib.gpak_set_train(self._h, _p(X), _p(y), N, d))
        self.N, self.d = N, d      # only once the library accepted the set: the outputs below are sized by them

    def set_params(self, expans, bias, sn2, dist_mode=DIST_DIRECT):
        e = np.ascontiguousarray(expans, dtype=np.float64)
        assert e.size == 8
        self._check(self._lib.gpak_set_params(self._h, _p(e), float(bias), float(sn2), int(dist_mode)))

    def set_kernel(self, terms, bias, white, sn2, dist_mode=DIST_DIRECT):
        """General HybKerns composition: terms = [(KERN_*, [parameters in the reference's order]), ...]."""
        kinds = (C.c_int * len(terms))(*[int(k) for k, _ in terms])
        pars = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64) for _, p in terms]))
        self._check(self._lib.gpak_set_kernel(self._h, len(terms), kinds, _p(pars), float(bias), float(white),
                                              float(sn2), int(dist_mode)))

    # -- hot path ------------------------------------------------------------------------
    def gram(self, want_d2=False):
        K = np.zeros((self.N, self.N), order="F")
        D2 = np.zeros((self.N, self.N), order="F") if want_d2 else None
        self._check(self._lib.gpak_gram(self._h, _p(K), _p(D2)))
        return (K, D2) if want_d2 else K

    def compute_k(self, X1, X2, want_d2=False):
        X1, X2 = _f(X1), _f(X2)
        n, d = X1.shape
        m = X2.shape[0]
        K = np.zeros((n, m), order="F")
        D2 = np.zeros((n, m), order="F") if want_d2 else None
        self._check(self._lib.gpak_compute_k(self._h, _p(X1), n, _p(X2), m, d, _p(K), _p(D2)))
        return (K, D2) if want_d2 else K

    def factor(self):
        """Returns True on success, False on Chol_fail (not positive definite)."""
        return self._check(self._lib.gpak_factor(self._h), allow=(ENOTPD,)) == OK

    def failed_column(self):
        return self._lib.gpak_failed_column(self._h)

    def chol_upper(self):
        R = np.zeros((self.N, self.N), order="F")
        self._check(self._lib.gpak_get_chol_upper(self._h, _p(R)))
        return R

    def solve_alpha(self):
        a = np.zeros(self.N)
        self._check(self._lib.gpak_solve_alpha(self._h, _p(a)))
        return a

    def solve_chol(self, X):
        X = np.array(X, dtype=np.float64, order="F", copy=True)
        k = 1 if X.ndim == 1 else X.shape[1]
        self._check(self._lib.gpak_solve_chol(self._h, _p(X), k))
        return X

    def logLikelihood(self):
        """GP_utils::logLikelihood(): the negative log marginal likelihood, NaN on Chol_fail."""
        v = C.c_double()
        rc = self._check(self._lib.gpak_nlz(self._h, C.byref(v)), allow=(ENOTPD,))
        return v.value if rc == OK else math.nan

    def nlz_terms(self):
        q, s, l = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.gpak_nlz_terms(self._h, C.byref(q), C.byref(s), C.byref(l)))
        return q.value, s.value, l.value

    def posteriorMeanVar(self, Xte, want_var=True, compat=0):
        Xte = _f(Xte)
        M, d = Xte.shape
        mean = np.zeros(M)
        var = np.zeros(M) if want_var else None
        self._check(self._lib.gpak_predict(self._h, _p(Xte), M, d, _p(mean), _p(var), compat))
        return mean, var

    def GradLL(self):
        g = np.zeros(10)
        self._check(self._lib.gpak_grad(self._h, _p(g)))
        return g

    def GradLL_hyb(self, ng):
        """Gradient of a general composition: children's blocks in order, bias, sn2."""
        g = np.zeros(int(ng))
        self._check(self._lib.gpak_grad_hyb(self._h, _p(g), int(ng)))
        return g

    def GradLL_exact(self, ng=10):
        """The exact gradient of logLikelihood() (gpak_grad_exact): same layout as GradLL_hyb."""
        g = np.zeros(int(ng))
        self._check(self._lib.gpak_grad_exact(self._h, _p(g), int(ng)))
        return g

    def loo(self):
        """Leave-one-out cross-validation from the current factor (gpak_loo): (mean, var, summary) with
        summary = {mse, mssr, log_pl, ms, passes, status}.  On Chol_fail status is ENOTPD and every number is NaN."""
        mean, var = np.zeros(self.N), np.zeros(self.N)
        s = _lib.LooSummary()
        rc = self._check(self._lib.gpak_loo(self._h, _p(mean), _p(var), C.byref(s)), allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        return mean, var, out

    def loo_grad(self, ng=10):
        """The gradient of -log_pl of loo() (gpak_loo_grad): (g, summary), g in GradLL_exact's layout and summary as
        loo()'s.  On Chol_fail status is ENOTPD and every number is NaN."""
        g = np.zeros(int(ng))
        s = _lib.LooSummary()
        rc = self._check(self._lib.gpak_loo_grad(self._h, _p(g), int(ng), C.byref(s)), allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        return g, out

    def cv_groups(self, labels):
        """Leave-group-out cross-validation from the current factor (gpak_cv_groups): (mean, var, logp, summary).
        labels: one integer per training sample, any values; the groups are numbered by sorted unique label and logp
        (one joint log predictive density per group) follows that order.  summary = {mse, mssr, msmd, log_pl, ms,
        groups, max_size, status, labels}, labels the sorted unique values.  On Chol_fail status is ENOTPD and every
        number is NaN."""
        group, values = group_labels(labels, self.N)
        mean, var, logp = np.zeros(self.N), np.zeros(self.N), np.zeros(values.size)
        s = _lib.CvGroupsSummary()
        rc = self._check(self._lib.gpak_cv_groups(self._h, group.ctypes.data_as(C.POINTER(C.c_int)), int(values.size),
                                                  _p(mean), _p(var), _p(logp), C.byref(s)), allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        out["labels"] = values
        return mean, var, logp, out

    def cv_groups_grad(self, labels, ng=10):
        """The gradient of -log_pl of cv_groups(labels) (gpak_cv_groups_grad): (g, summary), g in GradLL_exact's layout,
        labels and summary as cv_groups takes and returns them (the summary's ms is the call's grad_ms).  On Chol_fail
        status is ENOTPD and every number is NaN."""
        group, values = group_labels(labels, self.N)
        g = np.zeros(int(ng))
        s = _lib.CvGroupsSummary()
        rc = self._check(self._lib.gpak_cv_groups_grad(self._h, group.ctypes.data_as(C.POINTER(C.c_int)), int(values.size),
                                                       _p(g), int(ng), C.byref(s)), allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        out["labels"] = values
        return g, out

    def cv_folds(self, labels, no_batch=False):
        """k-fold cross-validation from the current factor (gpak_cv_folds): cv_groups for groups of any size, the same
        (mean, var, logp, summary) with the same summary keys.  no_batch: every group, whatever its size, takes the
        one-group-at-a-time path (GPAK_CV_FOLDS_NO_BATCH)."""
        group, values = group_labels(labels, self.N)
        mean, var, logp = np.zeros(self.N), np.zeros(self.N), np.zeros(values.size)
        s = _lib.CvGroupsSummary()
        rc = self._check(self._lib.gpak_cv_folds(self._h, group.ctypes.data_as(C.POINTER(C.c_int)), int(values.size),
                                                 _p(mean), _p(var), _p(logp), C.byref(s), NO_BATCH if no_batch else 0),
                         allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        out["labels"] = values
        return mean, var, logp, out

    def cv_folds_grad(self, labels, ng=10, no_batch=False):
        """The gradient of -log_pl of cv_folds(labels, no_batch) (gpak_cv_folds_grad): (g, summary), g in GradLL_exact's
        layout, labels and summary as cv_folds takes and returns them (the summary's ms is the call's grad_ms): groups
        of any size.  On Chol_fail status is ENOTPD and every number is NaN."""
        group, values = group_labels(labels, self.N)
        g = np.zeros(int(ng))
        s = _lib.CvGroupsSummary()
        rc = self._check(self._lib.gpak_cv_folds_grad(self._h, group.ctypes.data_as(C.POINTER(C.c_int)), int(values.size),
                                                      _p(g), int(ng), C.byref(s), NO_BATCH if no_batch else 0),
                         allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        out["labels"] = values
        return g, out

    def _blocks(self, Xd, nd):
        Xd = _f(Xd)
        nd = int(nd)
        if Xd.ndim != 2 or nd <= 0 or Xd.shape[0] % nd:
            raise GpakError(EINVAL, "Xd must hold nd rows per block")
        return Xd, Xd.shape[0] // nd, nd

    def block_cross(self, Xd, nd):
        """The block-averaged cross-kernel (gpak_block_cross): N x M, column b = the mean over block b's nd points (rows
        b * nd .. b * nd + nd of Xd) of k(X, x)."""
        Xd, M, nd = self._blocks(Xd, nd)
        K = np.zeros((self.N, M), order="F")
        self._check(self._lib.gpak_block_cross(self._h, _p(Xd), M, nd, Xd.shape[1], _p(K)))
        return K

    def predict_block(self, Xd, nd, want_var=True, latent=False):
        """Mean and variance of the block averages (gpak_predict_block); var includes sn2 / nd unless latent.  On
        Chol_fail both are NaN."""
        Xd, M, nd = self._blocks(Xd, nd)
        mean = np.zeros(M)
        var = np.zeros(M) if want_var else None
        self._check(self._lib.gpak_predict_block(self._h, _p(Xd), M, nd, Xd.shape[1], _p(mean), _p(var),
                                                 BLOCK_LATENT if latent else 0), allow=(ENOTPD,))
        return mean, var

    def local_metric(self, term=0):
        """G (4 x 4) with |(x - x') G|^2 = D2 of stationary term `term` of the composition in force (gpak_local_metric)."""
        G = np.zeros((4, 4), order="F")
        self._check(self._lib.gpak_local_metric(self._h, int(term), _p(G)))
        return G

    def predict_local(self, Xs, ys, Xd, nd, nbr, want_var=True, latent=False):
        """Moving-neighbourhood kriging (gpak_predict_local): node b (rows b * nd .. b * nd + nd of Xd) from the samples
        (Xs, ys) that row b of nbr (M x k, -1 padded: local_neighbours) names.  Returns (mean, var, summary), summary a
        dict of gpak_local_summary; var includes sn2 / nd unless latent.  The context needs parameters only."""
        Xs = _f(Xs)
        ys = np.ascontiguousarray(ys, dtype=np.float64).ravel()
        Xd, M, nd = self._blocks(Xd, nd)
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        if Xs.ndim != 2 or ys.size != Xs.shape[0] or nbr.ndim != 2 or nbr.shape[0] != M or Xd.shape[1] != Xs.shape[1]:
            raise GpakError(EINVAL, "Xs is Ns x d with Ns values ys, Xd has as many columns, nbr one row per node")
        mean = np.zeros(M)
        var = np.zeros(M) if want_var else None
        s = _lib.LocalSummary()
        self._check(self._lib.gpak_predict_local(self._h, _p(Xs), _p(ys), Xs.shape[0], Xs.shape[1], _p(Xd), M, nd,
                                                 nbr.ctypes.data_as(C.POINTER(C.c_int)), nbr.shape[1], _p(mean), _p(var),
                                                 LOCAL_LATENT if latent else 0, C.byref(s)))
        return mean, var, {f: getattr(s, f) for f, _ in s._fields_}

    def local_neighbours_dev(self, Xs, Xc, k, G=None, radius=0.0, want_dist2=False):
        """local_neighbours with the search on this context's device (gpak_local_neighbours_dev): the same lists, byte for
        byte.  Returns (nbr, used, dist2, summary): nbr and used as local_neighbours returns them, dist2 (M x k, None
        unless asked for) the squared distance of every listed sample and 0.0 in the unused slots, summary a dict of
        gpak_local_search_summary.  The context needs neither parameters nor a training set."""
        Xs, Xc = _f(Xs), _f(Xc)
        if Xs.ndim != 2 or Xc.ndim != 2 or Xs.shape[1] != Xc.shape[1]:
            raise GpakError(EINVAL, "Xs and Xc must be matrices with as many columns")
        d, M, k = Xs.shape[1], Xc.shape[0], int(k)
        if G is not None:
            G = np.asarray(G, dtype=np.float64)
            if G.shape == (4, 4) and d == 3:
                G = G[:3, :3]
            if G.shape != (d, d):
                raise GpakError(EINVAL, "G must be d x d (or the 4 x 4 of local_metric)")
            G = np.asfortranarray(G)
        nbr = np.full((max(M, 0), max(k, 0)), -1, dtype=np.int32)
        used = np.zeros(max(M, 0), dtype=np.int32)
        dist2 = np.zeros((max(M, 0), max(k, 0))) if want_dist2 else None
        ip = C.POINTER(C.c_int)
        s = _lib.LocalSearchSummary()
        self._check(self._lib.gpak_local_neighbours_dev(self._h, _p(Xs), Xs.shape[0], d, _p(Xc), M, _p(G), k, float(radius),
                                                        nbr.ctypes.data_as(ip), used.ctypes.data_as(ip), _p(dist2), C.byref(s)))
        return nbr, used, dist2, {f: getattr(s, f) for f, _ in s._fields_}

    def predict_local_ok(self, Xs, ys, Xd, nd, nbr, want_var=True, want_mu=False, latent=False):
        """Ordinary kriging in a moving neighbourhood (gpak_predict_local_ok): the arguments of predict_local; the mean is
        re-estimated from every node's own samples and the weights sum to one.  Returns (mean, var, mu, summary), mu the
        local means; var and mu are None unless asked for.  A node without a sample gets NaN in all three."""
        Xs = _f(Xs)
        ys = np.ascontiguousarray(ys, dtype=np.float64).ravel()
        Xd, M, nd = self._blocks(Xd, nd)
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        if Xs.ndim != 2 or ys.size != Xs.shape[0] or nbr.ndim != 2 or nbr.shape[0] != M or Xd.shape[1] != Xs.shape[1]:
            raise GpakError(EINVAL, "Xs is Ns x d with Ns values ys, Xd has as many columns, nbr one row per node")
        mean = np.zeros(M)
        var = np.zeros(M) if want_var else None
        mu = np.zeros(M) if want_mu else None
        s = _lib.LocalSummary()
        self._check(self._lib.gpak_predict_local_ok(self._h, _p(Xs), _p(ys), Xs.shape[0], Xs.shape[1], _p(Xd), M, nd,
                                                    nbr.ctypes.data_as(C.POINTER(C.c_int)), nbr.shape[1], _p(mean), _p(var),
                                                    _p(mu), LOCAL_LATENT if latent else 0, C.byref(s)))
        return mean, var, mu, {f: getattr(s, f) for f, _ in s._fields_}

    def predict_joint(self, Xd, nd, want_cov=True, latent=False, prior=False):
        """Mean (M) and full covariance (M x M, exactly symmetric) of the block averages (gpak_predict_joint); the
        diagonal includes sn2 / nd unless latent and is not clamped.  prior: the prior covariance between the block
        averages alone (GPAK_JOINT_PRIOR).  On Chol_fail of the training factor both are NaN."""
        Xd, M, nd = self._blocks(Xd, nd)
        mean = np.zeros(M)
        cov = np.zeros((M, M), order="F") if want_cov else None
        flags = (JOINT_LATENT if latent else 0) | (JOINT_PRIOR if prior else 0)
        self._check(self._lib.gpak_predict_joint(self._h, _p(Xd), M, nd, Xd.shape[1], _p(mean), _p(cov), flags),
                    allow=(ENOTPD,))
        return mean, cov

    def sample_joint(self, Xd, nd, xi, nugget=0.0, latent=False):
        """Conditional simulation (gpak_sample_joint): Z = mean 1' + Lc xi (M x S) for the caller's standard normals xi
        (M x S), Lc the lower Cholesky factor of the joint covariance + nugget I.  Returns (Z, mean).  Where that matrix is not
        positive definite Z is NaN and the mean valid (last_error() names the failing column); on Chol_fail of the
        training factor both are NaN."""
        Xd, M, nd = self._blocks(Xd, nd)
        xi = _f(xi)
        if xi.ndim == 1:
            xi = xi.reshape(-1, 1, order="F")
        if xi.ndim != 2 or xi.shape[0] != M:
            raise GpakError(EINVAL, "xi must hold one row per block")
        S = xi.shape[1]
        Z, mean = np.zeros((M, S), order="F"), np.zeros(M)
        self._check(self._lib.gpak_sample_joint(self._h, _p(Xd), M, nd, Xd.shape[1], _p(xi), S, float(nugget), _p(Z),
                                                _p(mean), JOINT_LATENT if latent else 0), allow=(ENOTPD,))
        return Z, mean

    def _realisations(self, a, rows, what):
        a = _f(a)
        if a.ndim == 1:
            a = a.reshape(-1, 1, order="F")
        if a.ndim != 2 or a.shape[0] != rows:
            raise GpakError(EINVAL, f"{what} must hold {rows} rows")
        return a

    def _condition_out(self, rc, s):
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        return out

    def condition(self, Xd, nd, Ysim, Fsim=None, unfused=False):
        """Conditioning by kriging (gpak_condition): Z = Fsim + Kbar (alpha 1' - Ky^-1 Ysim) for an unconditional draw
        (Fsim: M x S at the nodes, None = zeros; Ysim: N x S of the noisy observations).  Returns (Z, mean, summary): Z is
        M x S, mean = Kbar alpha, summary = {solve_ms, prior_ms, product_ms, batches, fused, status}.  unfused: the
        comparison path (averaged fill + GEMM).  On Chol_fail status is ENOTPD and Z and mean are NaN."""
        Xd, M, nd = self._blocks(Xd, nd)
        Ysim = self._realisations(Ysim, self.N, "Ysim")
        S = Ysim.shape[1]
        if Fsim is not None:
            Fsim = self._realisations(Fsim, M, "Fsim")
            if Fsim.shape[1] != S:
                raise GpakError(EINVAL, "Fsim and Ysim must hold as many realisations")
        Z, mean = np.zeros((M, S), order="F"), np.zeros(M)
        s = _lib.ConditionSummary()
        rc = self._check(self._lib.gpak_condition(self._h, _p(Xd), M, nd, Xd.shape[1], _p(Ysim), _p(Fsim), S, _p(Z), _p(mean),
                                                  COND_UNFUSED if unfused else 0, C.byref(s)), allow=(ENOTPD,))
        return Z, mean, self._condition_out(rc, s)

    def sample_path(self, Xd, nd, feat_term, omega, ab, b0, E, unfused=False):
        """The spectral prior sampler followed by the conditioning (gpak_sample_path): feat_term[f] = the stationary term
        of feature f, omega nfeat x 4 (row f = its frequency in that term's transformed coordinates), ab (2 nfeat) x S,
        b0 S entries or None, E N x S unit normals.  Returns (Z, mean, summary) as condition does."""
        Xd, M, nd = self._blocks(Xd, nd)
        ft = np.ascontiguousarray(feat_term, dtype=np.int32).ravel()
        nfeat = int(ft.size)
        om = np.ascontiguousarray(omega, dtype=np.float64)
        if om.shape != (nfeat, 4):
            raise GpakError(EINVAL, "omega must be nfeat x 4")
        ab = self._realisations(ab, 2 * nfeat, "ab")
        S = ab.shape[1]
        E = self._realisations(E, self.N, "E")
        if E.shape[1] != S:
            raise GpakError(EINVAL, "E and ab must hold as many realisations")
        if b0 is not None:
            b0 = np.ascontiguousarray(b0, dtype=np.float64).ravel()
            if b0.size != S:
                raise GpakError(EINVAL, "b0 must hold one entry per realisation")
        Z, mean = np.zeros((M, S), order="F"), np.zeros(M)
        s = _lib.ConditionSummary()
        rc = self._check(self._lib.gpak_sample_path(self._h, _p(Xd), M, nd, Xd.shape[1], nfeat, ft.ctypes.data_as(C.POINTER(C.c_int)),
                                                    _p(om), _p(ab), _p(b0), _p(E), S, _p(Z), _p(mean),
                                                    COND_UNFUSED if unfused else 0, C.byref(s)), allow=(ENOTPD,))
        return Z, mean, self._condition_out(rc, s)

    def design(self, Xt, nd, Xc, holes, weights=None, pick=0, want_reduction=False):
        """Infill drilling design (gpak_design): rank candidate holes by the estimation variance they would remove from the
        target blocks.  Xt holds nd rows per target block (nd = 1: points), Xc one row per candidate point, holes one
        integer label per candidate point (any values; the holes are numbered by sorted unique label and every output
        follows that order), weights one non-negative number per target (None: all ones).  Returns (gain, picked,
        pick_gain, extras): gain[h] = the weighted variance hole h alone removes, picked / pick_gain = the greedy plan of
        `pick` holes (hole numbers and conditional gains in pick order), extras = {reduction (T x H, or None), var,
        var_after, summary}, summary = {var_before, var_after, ms, holes, max_size, picks, status, labels}.  On
        Chol_fail status is ENOTPD and every number is NaN."""
        Xt, T, nd = self._blocks(Xt, nd)
        Xc = _f(Xc)
        if Xc.ndim != 2 or Xc.shape[1] != Xt.shape[1]:
            raise GpakError(EINVAL, "Xc must have as many columns as Xt")
        hole, values = group_labels(holes, Xc.shape[0])
        H, k = int(values.size), int(pick)
        wt = None
        if weights is not None:
            wt = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if wt.size != T:
                raise GpakError(EINVAL, "weights must hold one entry per target")
        gain = np.zeros(H)
        red = np.zeros((T, H), order="F") if want_reduction else None
        var, var_after = np.zeros(T), np.zeros(T)
        picked, pick_gain = np.full(max(k, 0), -1, dtype=np.int32), np.zeros(max(k, 0))
        s = _lib.DesignSummary()
        rc = self._check(self._lib.gpak_design(self._h, _p(Xt), T, nd, _p(Xc), Xc.shape[0], Xt.shape[1],
                                               hole.ctypes.data_as(C.POINTER(C.c_int)), H, _p(wt), k, _p(gain), _p(red), _p(var),
                                               picked.ctypes.data_as(C.POINTER(C.c_int)), _p(pick_gain), _p(var_after),
                                               C.byref(s)), allow=(ENOTPD,))
        out = {name: getattr(s, name) for name, _ in s._fields_}
        out["status"] = rc
        out["labels"] = values
        return gain, picked, pick_gain, {"reduction": red, "var": var, "var_after": var_after, "summary": out}

    def last_error(self):
        return self._lib.gpak_last_error(self._h).decode()

    # -- measurement ---------------------------------------------------------------------
    def timing(self):
        t = _lib.PhaseTimes()
        self._check(self._lib.gpak_timing(self._h, C.byref(t)))
        out = {name: getattr(t, name) for name, _ in t._fields_}
        out["accumulated_ms"] = list(t.accumulated_ms)
        return out

    def n_gpus(self):
        return self._lib.gpak_n_gpus(self._h)

    def transport(self):
        return self._lib.gpak_transport(self._h).decode()

    def rank_stats(self, rank):
        """gpak_dist_stats of one rank of a multi-GPU context (last step)."""
        from . import dist as _dist
        _dist._load()
        st = _dist.Stats()
        self._check(self._lib.gpak_group_rank_stats(self._h, int(rank), C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def calibrate(self):
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.gpak_calibrate(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
