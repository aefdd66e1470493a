"""What a context of include/gpak.h must answer, whatever it was asked before.  TEST INFRASTRUCTURE.

ModelGpak has the method names of gp_ss_ak_amd.gpak.Gpak and no memory beyond the last training set, the last kernel call
and the options: every answer is computed from those alone, on the CPU, from the references the suite already holds the
single features to (the CPU checker in oracle/, exact_grad_ref, loo_ref, block_ref, joint_ref; for the feature calls
loo_grad_ref, cvg_ref, lgo_grad_ref, design_ref, path_ref, local_ref, local_ok_ref, local_search_ref).  Results are cached by
(training set, kernel, operation), so a long sequence costs each distinct state once.  It restates the statuses the header
promises (GPAK_ESTATE before a training set or parameters, GPAK_ENOTIMPL, GPAK_EINVAL, GPAK_ENOTPD with quiet NaN).

CachingModel is the opposite: a Python restatement of the VALIDITY LOGIC of a context -- CtxState (csrc/ctx_state.h) and
the calls of csrc/api.hip that raise its events: which call builds what, which call drops it -- that answers every
question from the state its flags point at.  Unmutated it equals ModelGpak step for step.  Each name in MUTATIONS drops
one invalidation; tests/test_ctx_sequences.py proves on the CPU that every one of them is caught by a named sequence, i.e.
that the sequences would notice the corresponding slip.  It logs the events it passes through under the names of
CtxState's members: tests/test_ctx_state.py replays them through the C++ struct itself and compares the two, flag by flag.
FEATURE_MUTATIONS (after the class) do the same for the feature calls, with FEATURE_REDUNDANT for a reset another one covers.

GroupCaching does the same for a group (gpak_create_multi): the flags of csrc/multi.hip, RankCore::have_result of
csrc/dist.hip and the replica contexts' flags, with GROUP_MUTATIONS; it also counts the evaluations gpak_timing reports.
ModelGpak(ranks > 1) is the stateless model of a group: the calls built for one GPU alone are refused.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref  # noqa: E402
import exact_grad_ref as xref  # noqa: E402
import joint_ref  # noqa: E402
import loo_ref  # noqa: E402

OK, ENOTPD, EINVAL, ESTATE, ENOMEM, ENOTIMPL = 0, 1, 2, 3, 4, 5
F64, F32 = 0, 1
DIST_EXPANSION, DIST_DIRECT = 0, 1
OPT_MEMOISE, OPT_NB_OUTER, OPT_NB_WIDE, OPT_POTRF_CO, OPT_TAIL_MAX_NP, OPT_BWD_FUSED, OPT_LOO_ROWS = 1, 2, 5, 10, 13, 12, 14
OPT_INV512 = 9
NPARS = {xref.EXPANS: 8, xref.EXP: 2, xref.RBF: 3}
SIGMA_AT = {xref.EXPANS: 6, xref.EXP: 1, xref.RBF: 2}

MUTATIONS = ("memo ignores composition", "gram keeps factor", "set_train keeps alpha", "set_kernel keeps U",
             "failed factor keeps alpha", "solve_chol keeps z", "predict leaks pooled mean", "f32 image kept",
             "recovery keeps failed_column")


class ModelError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__(f"model status {status}: {msg}")
        self.status = status


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


class ModelGpak:
    def __init__(self, precision=F64, cache=None, ranks=1):
        self.precision = precision
        self.ranks = int(ranks)               # > 1: a group (gpak_create_multi): the calls built for one GPU alone are refused
        self.cache = {} if cache is None else cache
        self.opts = {}
        self.X = self.y = self.tkey = None
        self.kern = self.kkey = None
        self.N = self.d = 0

    def close(self):
        pass

    # -- state ---------------------------------------------------------------------------------------------------
    def set_option(self, opt, value):
        value = int(value)
        bad = {OPT_NB_OUTER: value < 128 or value % 128, OPT_NB_WIDE: value < 0 or value % 128,
               OPT_POTRF_CO: not 0 <= value <= 2, OPT_TAIL_MAX_NP: value < 0, OPT_BWD_FUSED: not 0 <= value <= 2,
               OPT_LOO_ROWS: value < 0 or value % 128}
        if not 1 <= opt <= 14 or bad.get(opt, False):
            raise ModelError(EINVAL, "option")
        self.opts[opt] = value

    def set_train(self, X, y):
        X = np.asfortranarray(X, dtype=np.float64)
        if X.shape[1] not in (3, 4):
            raise ModelError(ENOTIMPL, "inputs must have 3 or 4 columns")
        self.X, self.y = X, np.ascontiguousarray(y, dtype=np.float64).ravel()
        self.N, self.d = X.shape
        self.tkey = _digest(self.X, self.y)

    def set_params(self, expans, bias, sn2, dist_mode=DIST_DIRECT):
        ModelGpak.set_kernel(self, [(xref.EXPANS, expans)], bias, 0.0, sn2, dist_mode)

    def set_kernel(self, terms, bias, white, sn2, dist_mode=DIST_DIRECT):
        if dist_mode not in (DIST_EXPANSION, DIST_DIRECT) or not 1 <= len(terms) <= 3:
            raise ModelError(EINVAL, "kernel")
        terms = tuple((int(k), tuple(float(v) for v in p)) for k, p in terms)
        if any(k not in NPARS for k, _ in terms):
            raise ModelError(EINVAL, "unknown kernel kind")
        self.kern = dict(terms=terms, bias=float(bias), white=float(white), sn2=float(sn2), mode=int(dist_mode))
        self.kkey = (terms, float(bias), float(white), float(sn2), int(dist_mode))

    # -- what the answers are computed from ---------------------------------------------------------------------
    def _cached(self, op, fn):
        key = (self.tkey, self.kkey, op)
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def _need(self, train=True, params=True):
        if train and self.X is None:
            raise ModelError(ESTATE, "no training set")
        if params and self.kern is None:
            raise ModelError(ESTATE, "no parameters")

    @property
    def expans_only(self):
        k = self.kern
        return k is None or (len(k["terms"]) == 1 and k["terms"][0][0] == xref.EXPANS and k["white"] == 0.0)

    def prior_variance(self):
        k = self.kern
        return k["bias"] + k["white"] + sum(p[SIGMA_AT[kind]] ** 2 for kind, p in k["terms"])

    def _gram(self, X1, X2, white, want_d2=False):
        k, orc = self.kern, _orc()
        if self.expans_only:
            return orc.gram(X1, X2, np.array(k["terms"][0][1]), k["bias"], k["mode"], want_d2=want_d2)
        return orc.gram_hyb(X1, X2, [(kd, list(p)) for kd, p in k["terms"]], k["bias"], white, k["mode"], want_d2=want_d2)

    def _fit(self):
        """{K (White on the diagonal), col (failing column, 0: none), info, alpha, L}"""
        def build():
            orc, k = _orc(), self.kern
            K = self._gram(self.X, self.X, k["white"])
            _, col = orc.potrf_lower(np.eye(self.N) + K / k["sn2"])
            if col:
                return dict(K=K, col=int(col))
            info, alpha, L = orc.nlz_lean(K, self.y, k["sn2"])
            return dict(K=K, col=0, info=info, alpha=alpha, L=L)
        self._need()
        return self._cached("fit", build)

    def _fit_ok(self):
        f = self._fit()
        if f["col"]:
            raise ModelError(ENOTPD, "B = I + K/sn2 is not positive definite")
        return f

    def _terms(self):
        return [(kd, list(p)) for kd, p in self.kern["terms"]]

    # -- hot path -------------------------------------------------------------------------------------------------
    def gram(self, want_d2=False):
        self._need()
        K, D2 = self._cached("gram", lambda: self._gram(self.X, self.X, self.kern["white"], want_d2=True))
        return (K, D2) if want_d2 else K

    def compute_k(self, X1, X2, want_d2=False):
        X1, X2 = np.asfortranarray(X1, dtype=float), np.asfortranarray(X2, dtype=float)
        if X1.shape[1] not in (3, 4):
            raise ModelError(ENOTIMPL, "inputs must have 3 or 4 columns")
        self._need(train=False)
        key = (None, self.kkey, ("compute_k", _digest(X1), _digest(X2)))
        if key not in self.cache:
            self.cache[key] = self._gram(X1, X2, self.kern["white"], want_d2=True)
        K, D2 = self.cache[key]
        return (K, D2) if want_d2 else K

    def factor(self):
        return self._fit()["col"] == 0

    def failed_column(self):
        """Of the factorisation of the current state: the sequences ask right after a call that factors."""
        if self.X is None or self.kern is None:
            return 0
        return self._fit()["col"]

    def chol_upper(self):
        return np.asfortranarray(self._fit_ok()["L"].T)

    def solve_alpha(self):
        return self._fit_ok()["alpha"].copy()

    def solve_chol(self, X):
        L = self._fit_ok()["L"]
        return _orc().solve_chol(L, np.asarray(X, dtype=float))

    def logLikelihood(self):
        f = self._fit()
        return float("nan") if f["col"] else f["info"].nlz

    def nlz_terms(self):
        i = self._fit_ok()["info"]
        return i.quad, i.sumlp, i.logdet

    def posteriorMeanVar(self, Xte, want_var=True, compat=0):
        Xte = np.asfortranarray(Xte, dtype=float)
        if self.X is None:
            raise ModelError(ESTATE, "no training set")
        if Xte.shape[1] != self.d:
            raise ModelError(EINVAL, "test points must have as many columns as the training set")
        f = self._fit_ok()

        def build():
            import scipy.linalg as sl
            k, orc = self.kern, _orc()
            if self.expans_only:
                return orc.predict(self.X, Xte, np.array(k["terms"][0][1]), k["bias"], k["sn2"], f["alpha"], f["L"], k["mode"],
                                   compat, True)
            assert compat == 0
            kX = self._gram(self.X, Xte, k["white"])                     # the checker leaves White out of a cross block
            V = sl.solve_triangular(f["L"], kX, lower=True)
            var = np.maximum(self.prior_variance() - np.sum(V * V, axis=0) / k["sn2"], 0.0) + k["sn2"]
            return kX.T @ f["alpha"], var
        mean, var = self._cached(("predict", _digest(Xte), compat), build)
        return mean.copy(), (var.copy() if want_var else None)

    def _ng(self):
        return sum(NPARS[kd] for kd, _ in self.kern["terms"]) + 2

    def _grad_checks(self, ng):
        if sum(kd == xref.EXPANS for kd, _ in self.kern["terms"]) > 1:
            raise ModelError(ENOTIMPL, "at most one ExpAns child")
        if int(ng) != self._ng():
            raise ModelError(EINVAL, "gradient vector has the wrong length")
        if self.kern["white"] != 0.0:
            raise ModelError(ENOTIMPL, "no gradient for a White child")

    def GradLL(self):
        if not self.expans_only:
            raise ModelError(ENOTIMPL, "gpak_grad handles the ExpAns(+Bias) composition only")
        f, k = self._fit_ok(), self.kern
        return self._cached("grad", lambda: _orc().grad_ref(self.X, self.y, f["K"], f["L"], f["alpha"], np.array(k["terms"][0][1]),
                                                            k["bias"], k["sn2"], k["mode"])).copy()

    def GradLL_hyb(self, ng):
        f, k = self._fit_ok(), self.kern
        self._grad_checks(ng)
        return self._cached("grad_hyb", lambda: _orc().grad_hyb(self.X, self.y, f["K"], f["L"], f["alpha"], self._terms(), True,
                                                                k["sn2"], k["mode"])).copy()

    def _single_only(self, name):
        if self.ranks > 1:
            raise ModelError(ENOTIMPL, f"{name} is built for the single-GPU context only")

    def n_gpus(self):
        return self.ranks

    def transport(self):
        return "none" if self.ranks == 1 else "in-process peer copies"       # every rank of a test's group sits on device 0

    def loo_grad(self, ng=10):
        self._single_only("gpak_loo_grad")
        self._need()
        self._grad_checks(ng)
        nan = float("nan")
        if self._fit()["col"]:
            return np.full(int(ng), nan), dict(mse=nan, mssr=nan, log_pl=nan, ms=0.0, passes=0, status=ENOTPD)
        return self._loo_grad()[0].copy(), self.loo()[2]

    def GradLL_exact(self, ng=10):
        self._single_only("gpak_grad_exact")
        self._fit_ok()
        self._grad_checks(ng)
        k = self.kern
        return self._cached("grad_exact", lambda: xref.grad_exact(self.X, self.y, self._terms(), k["bias"], k["sn2"])).copy()

    def loo(self):
        self._single_only("gpak_loo")
        f = self._fit()
        nan = float("nan")
        if f["col"]:
            return np.full(self.N, nan), np.full(self.N, nan), dict(mse=nan, mssr=nan, log_pl=nan, ms=0.0, passes=0, status=ENOTPD)

        def build():
            m, v = loo_ref.loo(f["K"], self.y, self.kern["sn2"])
            return m, v, loo_ref.summary(self.y, m, v)
        m, v, s = self._cached("loo", build)
        return m.copy(), v.copy(), dict(s, status=OK)

    def _block_pre(self, Xd, nd):
        self._single_only("the block and joint calls")
        Xd = np.asfortranarray(Xd, dtype=float)
        if self.X is None:
            raise ModelError(ESTATE, "no training set")
        if Xd.shape[1] != self.d:
            raise ModelError(EINVAL, "block points must have as many columns as the training set")
        self._need()
        return Xd, Xd.shape[0] // int(nd), int(nd)

    def _block(self, Xd, nd):
        k = self.kern
        return self._cached(("block", _digest(Xd), nd), lambda: block_ref.block_predict(self.X, self.y, Xd, nd, self._terms(), k["bias"],
                                                                                        k["white"], k["sn2"]))

    def block_cross(self, Xd, nd):
        Xd, M, nd = self._block_pre(Xd, nd)
        self._fit_ok()        # the C call fills Kbar with NaN and returns GPAK_ENOTPD; Gpak.block_cross raises it
        return self._cached(("cross", _digest(Xd), nd), lambda: block_ref.block_cross(self.X, Xd, nd, self._terms(), self.kern["bias"]))

    def predict_block(self, Xd, nd, want_var=True, latent=False):
        Xd, M, nd = self._block_pre(Xd, nd)
        if self._fit()["col"]:
            return np.full(M, np.nan), (np.full(M, np.nan) if want_var else None)
        r = self._block(Xd, nd)
        return r["mean"].copy(), ((r["latent"] if latent else r["var"]).copy() if want_var else None)

    def _joint(self, Xd, nd):
        k = self.kern
        method = "points" if self.N + Xd.shape[0] <= 2400 else "blocks"
        return self._cached(("joint", _digest(Xd), nd), lambda: joint_ref.joint(self.X, self.y, Xd, nd, self._terms(), k["bias"], k["white"],
                                                                                k["sn2"], want_prior=False, method=method))

    def predict_joint(self, Xd, nd, want_cov=True, latent=False, prior=False):
        Xd, M, nd = self._block_pre(Xd, nd)
        assert not prior
        if self._fit()["col"]:
            return np.full(M, np.nan), (np.full((M, M), np.nan) if want_cov else None)
        r = self._joint(Xd, nd)
        cov = r["latent"] + (0.0 if latent else self.kern["sn2"] / nd) * np.eye(M)
        return r["mean"].copy(), (cov if want_cov else None)

    def sample_joint(self, Xd, nd, xi, nugget=0.0, latent=False):
        Xd, M, nd = self._block_pre(Xd, nd)
        xi = np.asarray(xi, dtype=float).reshape(M, -1)
        if self._fit()["col"]:
            return np.full(xi.shape, np.nan), np.full(M, np.nan)
        mean, cov = self.predict_joint(Xd, nd, latent=latent)
        Lc = np.linalg.cholesky(cov + nugget * np.eye(M))
        return mean[:, None] + Lc @ xi, mean

    def timing(self):
        return None      # how often a context factored is not a function of its state: CachingModel counts

    # -- the feature calls (include/gpak_loo_grad.h, gpak_cv_groups*.h, gpak_cv_folds*.h, gpak_design.h, gpak_condition.h,
    # gpak_local*.h): stateless, on the references their own tests hold them to; the statuses in the order of csrc/api.hip --
    def _loo_grad(self):
        """(gradient, 1/2 sum |W|) of loo_grad_ref, as tests/loo_grad_model.py"""
        import loo_grad_ref
        k = self.kern

        def build():
            g, W = loo_grad_ref.grad_loo(self.X, self.y, self._terms(), k["bias"], k["sn2"], want_w=True)
            return g, 0.5 * float(np.abs(W).sum())
        return self._cached("loo_grad", build)

    def _labels(self, labels, limit, what="group"):
        values, group = np.unique(np.asarray(labels), return_inverse=True)
        group = group.reshape(-1)
        sizes = np.bincount(group)
        if limit and sizes.max() > limit:
            raise ModelError(EINVAL, f"a {what} has more than {limit} members")
        return values, group, sizes

    def _cv(self, name, labels, limit):
        import cvg_ref
        self._single_only(name)
        self._need()
        values, group, sizes = self._labels(labels, limit)
        nan = float("nan")
        if self._fit()["col"]:
            return (np.full(self.N, nan), np.full(self.N, nan), np.full(sizes.size, nan),
                    dict(mse=nan, mssr=nan, msmd=nan, log_pl=nan, ms=0.0, groups=int(sizes.size), max_size=0, status=ENOTPD, labels=values))

        def build():
            mean, var, logp, md = cvg_ref.cv_groups(self._fit()["K"], self.y, self.kern["sn2"], group)
            return mean, var, logp, cvg_ref.summary(self.y, mean, var, logp, md)
        mean, var, logp, s = self._cached(("cv", _digest(group)), build)
        return mean.copy(), var.copy(), logp.copy(), dict(s, ms=0.0, groups=int(sizes.size), max_size=int(sizes.max()), status=OK, labels=values)

    def cv_groups(self, labels):
        return self._cv("gpak_cv_groups", labels, 128)

    def cv_folds(self, labels, no_batch=False):
        return self._cv("gpak_cv_folds", labels, 0)

    def _cv_grad_ref(self, group):
        """(gradient, 1/2 sum |W|) of lgo_grad_ref on the direct-form Gram matrix, as tests/lgo_grad_model.py"""
        import lgo_grad_ref
        k = self.kern

        def build():
            g, W = lgo_grad_ref.grad_lgo(self.X, self.y, self._terms(), k["bias"], k["sn2"], group, want_w=True)
            return g, 0.5 * float(np.abs(W).sum())
        return self._cached(("cv_grad", _digest(group)), build)

    def _cv_grad(self, name, labels, ng, limit):
        self._single_only(name)
        self._need()
        self._grad_checks(ng)
        values, group, sizes = self._labels(labels, limit)
        nan = float("nan")
        if self._fit()["col"]:
            return np.full(int(ng), nan), dict(mse=nan, mssr=nan, msmd=nan, log_pl=nan, ms=0.0, groups=int(sizes.size), max_size=0,
                                               status=ENOTPD, labels=values)
        return self._cv_grad_ref(group)[0].copy(), self._cv(name, labels, 0)[3]

    def cv_groups_grad(self, labels, ng=10):
        return self._cv_grad("gpak_cv_groups_grad", labels, ng, 128)

    def cv_folds_grad(self, labels, ng=10, no_batch=False):
        return self._cv_grad("gpak_cv_folds_grad", labels, ng, 0)

    def design(self, Xt, nd, Xc, holes, weights=None, pick=0, want_reduction=False):
        import design_ref
        self._single_only("gpak_design")
        self._need()
        Xt, Xc, nd, k = np.asfortranarray(Xt, dtype=float), np.asfortranarray(Xc, dtype=float), int(nd), int(pick)
        if Xc.shape[1] != Xt.shape[1] or Xt.shape[1] != self.d:
            raise ModelError(EINVAL, "target and candidate points must have as many columns as the training set")
        values, hole, sizes = self._labels(holes, 128, "hole")
        T, H = Xt.shape[0] // nd, int(sizes.size)
        wt = None if weights is None else np.asarray(weights, dtype=float).ravel()
        if wt is not None and not np.all(np.isfinite(wt) & (wt >= 0.0)):
            raise ModelError(EINVAL, "a weight is negative or not finite")
        if not 0 <= k <= H:
            raise ModelError(EINVAL, "k is outside [0, H]")
        nan = float("nan")
        if self._fit()["col"]:
            s = dict(var_before=nan, var_after=nan, ms=0.0, holes=H, max_size=0, picks=0, status=ENOTPD, labels=values)
            return (np.full(H, nan), np.full(k, -1, dtype=np.int32), np.full(k, nan),
                    {"reduction": np.full((T, H), nan) if want_reduction else None, "var": np.full(T, nan), "var_after": np.full(T, nan),
                     "summary": s})
        kn = self.kern
        r = self._cached(("design", _digest(Xt), nd, _digest(Xc), _digest(hole), None if wt is None else _digest(wt), k),
                         lambda: design_ref.design(self.X, Xt, nd, Xc, hole, self._terms(), kn["bias"], kn["white"], kn["sn2"], wt=wt, k=k))
        f = lambda a: np.asarray(a).astype(float)      # noqa: E731
        s = dict(var_before=float(r["var_before"]), var_after=float(r["var_after_sum"]), ms=0.0, holes=H, max_size=int(sizes.max()), picks=k,
                 status=OK, labels=values)
        return (f(r["gain"]), np.array(r["picked"], dtype=np.int32), f(r["pick_gain"]).reshape(k),
                {"reduction": f(r["reduction"]) if want_reduction else None, "var": f(r["var"]), "var_after": f(r["var_after"]), "summary": s,
                 "gaps": design_ref.pick_gaps(r["rounds"]), "weight_sum": float(T if wt is None else wt.sum())})

    def _nodes(self, name, Xd, nd):
        """the prologue of gpak_condition / gpak_sample_path: a training set, then the columns (parameters: ensure_nlz)"""
        self._single_only(name)
        Xd = np.asfortranarray(Xd, dtype=float)
        if self.X is None:
            raise ModelError(ESTATE, "no training set")
        if Xd.shape[1] != self.d:
            raise ModelError(EINVAL, "block points must have as many columns as the training set")
        return Xd, Xd.shape[0] // int(nd), int(nd)

    def path_model(self, Xd, nd):
        import path_ref
        k = self.kern
        return self._cached(("path", _digest(Xd), int(nd)), lambda: path_ref.Model(self.X, self.y, Xd, int(nd), self._terms(), k["bias"],
                                                                                  k["white"], k["sn2"]))

    def _conditioned(self, Xd, M, nd, S, unfused, key, fn):
        nan = float("nan")
        s = dict(solve_ms=0.0, prior_ms=0.0, product_ms=0.0, batches=0, fused=0 if unfused else 1)
        if self._fit()["col"]:
            return np.full((M, S), nan), np.full(M, nan), dict(s, status=ENOTPD)
        Z, mean = self._cached(key, lambda: tuple(np.asarray(a).astype(float) for a in fn(self.path_model(Xd, nd))))
        return Z.copy(), mean.copy(), dict(s, status=OK)

    def condition(self, Xd, nd, Ysim, Fsim=None, unfused=False):
        Xd, M, nd = self._nodes("gpak_condition", Xd, nd)
        self._need()
        Ysim = np.asarray(Ysim, dtype=float).reshape(self.N, -1)
        key = ("condition", _digest(Xd), nd, _digest(Ysim), None if Fsim is None else _digest(Fsim))
        return self._conditioned(Xd, M, nd, Ysim.shape[1], unfused, key, lambda pm: pm.condition(Ysim, Fsim))

    def sample_path(self, Xd, nd, feat_term, omega, ab, b0, E, unfused=False):
        Xd, M, nd = self._nodes("gpak_sample_path", Xd, nd)
        self._need()
        ft = np.asarray(feat_term).ravel()
        if ft.min() < 0 or ft.max() >= len(self.kern["terms"]):
            raise ModelError(EINVAL, "a feature names a term outside the composition")
        if b0 is None and self.kern["bias"] != 0.0:
            raise ModelError(EINVAL, "b0 is NULL and the constant is not 0")
        ab = np.asarray(ab, dtype=float).reshape(2 * ft.size, -1)
        key = ("path draw", _digest(Xd), nd, _digest(ft), _digest(omega), _digest(ab), None if b0 is None else _digest(b0), _digest(E))
        return self._conditioned(Xd, M, nd, ab.shape[1], unfused, key, lambda pm: pm.sample_path(ft, omega, ab, b0, E))

    def _local_pre(self, name, Xs, Xd):
        self._single_only(name)
        Xs, Xd = np.asfortranarray(Xs, dtype=float), np.asfortranarray(Xd, dtype=float)
        if Xd.shape[1] != Xs.shape[1]:
            raise ModelError(EINVAL, "Xd has as many columns as Xs")
        if Xs.shape[1] not in (3, 4) or (self.X is not None and Xs.shape[1] != self.d):
            raise ModelError(ENOTIMPL, "the samples have 3 or 4 columns, as many as the context's training set")
        if self.kern is None:
            raise ModelError(ESTATE, "no parameters")
        return Xs, Xd

    def _local_cached(self, what, Xs, ys, Xd, nd, nbr, fn):
        k = self.kern
        key = (None, self.kkey[:4], (what, _digest(Xs), _digest(ys), _digest(Xd), int(nd), _digest(nbr)))   # the direct form whatever the mode
        if key not in self.cache:
            self.cache[key] = fn(Xs, ys, Xd, int(nd), nbr, self._terms(), k["bias"], k["white"], k["sn2"])
        return self.cache[key]

    def local_metric(self, term=0):
        """G with |(x - x') G|^2 = D2 of the term (any such G: the answers are compared through D2, see cs.model_errors)"""
        import path_ref
        self._single_only("gpak_local_metric")
        if self.kern is None:
            raise ModelError(ESTATE, "no parameters")
        if not 0 <= int(term) < len(self.kern["terms"]):
            raise ModelError(EINVAL, "term is outside the composition")
        kind, p = self.kern["terms"][int(term)]
        G = np.zeros((4, 4))
        if kind == xref.EXPANS:
            G[:3, :3] = np.asarray(xref.expans_metric([float(v) for v in p])[0], dtype=float)
            G[3, 3] = p[7]
        else:
            G[np.arange(4), np.arange(4)] = 1.0 / p[0]
        return G

    def predict_local(self, Xs, ys, Xd, nd, nbr, want_var=True, latent=False):
        import local_ref
        Xs, Xd = self._local_pre("gpak_predict_local", Xs, Xd)
        r = self._local_cached("local", Xs, ys, Xd, nd, nbr, local_ref.local_predict)
        f = lambda a: np.asarray(a).astype(float)      # noqa: E731
        s = dict(nodes=int(r["used"].size), empty=int((r["used"] == 0).sum()), notpd=int(r["notpd"].sum()), max_used=int(r["used"].max()))
        return f(r["mean"]), (f(r["latent"] if latent else r["var"]) if want_var else None), s

    def predict_local_ok(self, Xs, ys, Xd, nd, nbr, want_var=True, want_mu=False, latent=False):
        import local_ok_ref
        Xs, Xd = self._local_pre("gpak_predict_local_ok", Xs, Xd)
        r = self._local_cached("local ok", Xs, ys, Xd, nd, nbr, local_ok_ref.local_predict_ok)
        f = lambda a: np.asarray(a).astype(float)      # noqa: E731
        s = dict(nodes=int(r["used"].size), empty=int((r["used"] == 0).sum()), notpd=int(r["notpd"].sum()), max_used=int(r["used"].max()))
        return f(r["mean"]), (f(r["latent"] if latent else r["var"]) if want_var else None), (f(r["mu"]) if want_mu else None), s

    def local_neighbours_dev(self, Xs, Xc, k, G=None, radius=0.0, want_dist2=False):
        import local_ref
        import local_search_ref as sr
        self._single_only("gpak_local_neighbours_dev")
        Xs, Xc = np.asfortranarray(Xs, dtype=float), np.asfortranarray(Xc, dtype=float)
        if Xs.shape[1] != Xc.shape[1] or Xs.shape[1] not in (3, 4) or not 1 <= int(k) <= 128:
            raise ModelError(EINVAL, "the samples have 3 or 4 columns, k is in 1..128")
        key = (None, None, ("search", _digest(Xs), _digest(Xc), int(k), None if G is None else _digest(G), float(radius)))
        if key not in self.cache:
            nbr, used = local_ref.brute_neighbours(Xs, Xc, int(k), G, radius)
            self.cache[key] = (nbr, used, sr.dist2_lists(sr.transform(Xs, G), sr.transform(Xc, G), nbr))
        nbr, used, d2 = self.cache[key]
        return nbr.copy(), used.copy(), (d2.copy() if want_dist2 else None), dict(max_used=int(used.max()))


# -------------------------------------------------------------------------------------------------------------------------
def _spoil(out):
    """What a kernel reading the wrong buffer returns: not the right numbers."""
    if isinstance(out, tuple):
        return tuple(_spoil(o) for o in out)
    if isinstance(out, dict):
        return {k: (v if k in ("status", "passes", "ms") else _spoil(v)) for k, v in out.items()}
    if out is None or isinstance(out, (bool, np.bool_, int, np.integer, list)) or (isinstance(out, np.ndarray) and out.dtype.kind in "iu"):
        return out                                # counts, labels, lists of hole numbers: the wrong buffer does not change them
    return np.asarray(out, dtype=float) * (1.0 + 1e-3) if isinstance(out, np.ndarray) else out * (1.0 + 1e-3)


class CachingModel(ModelGpak):
    """The facts of CtxState (csrc/ctx_state.h) as its events change them, and the calls of csrc/api.hip as they raise the
    events.  The ladder: the transformed points U, the factor in dM, alpha, the nlZ terms; off the factor hang z (L^-1 y/sn2
    sits in dWork), the back substitution it supports and the fp32 image.  Where the struct keeps a flag the model keeps a
    `snapshot`, the state (training set, kernel) the quantity was built from: uS, fS, aS, nS, lfS.  Answers come from
    ModelGpak AT that snapshot; `taint` holds the buffers whose contents are not what their flag says.  `events` lists
    every event passed through, as the line tests/ctx_state_driver.cpp reads; flags() is what the driver prints."""

    def __init__(self, precision=F64, cache=None, mut=()):
        super().__init__(precision, cache)
        unknown = [m for m in mut if m not in MUTATIONS + FEATURE_MUTATIONS + FEATURE_REDUNDANT]
        assert not unknown, unknown
        self.mut = set(mut)
        self.states = {}
        self.uS = self.fS = self.aS = self.nS = self.lfS = None
        self.bufA = self.bufN = None          # what dAlpha / the nlZ terms physically hold
        self.z_ok = self.z_clobbered = False
        self.backsolve = 0                    # CtxState::Backsolve of the current factor
        self.events = []
        self.taint = set()
        self.failed_col = 0
        self.failS = None
        self.evals = 0
        self.memoise = False
        self.have_params = False
        self.stored = None                    # expans, bias, sn2, dist_mode as gpak_ctx keeps them
        self.stored_expans = None
        self.was_expans_only, self.was_white = True, 0.0
        self.dropped = []                     # (mutation, what it kept) each time a mutation changed the outcome

    # -- snapshots ----------------------------------------------------------------------------------------------
    def _cur(self):
        key = (self.tkey, self.kkey)
        self.states[key] = (self.X, self.y, self.kern)
        return key

    def _at(self, S):
        X, y, kern = self.states[S]
        m = ModelGpak(self.precision, self.cache)
        if X is not None:
            m.set_train(X, y)
        if kern is not None:
            m.set_kernel(kern["terms"], kern["bias"], kern["white"], kern["sn2"], kern["mode"])
        m.opts = dict(self.opts)
        return m

    def _invalidate(self):
        """CtxState::drop_factor: the rungs from the factor up and the factor's side facts"""
        self.fS = self.aS = self.nS = None
        self._drop_side_facts()

    def _drop_side_facts(self):
        self.z_ok = self.z_clobbered = False
        self.backsolve = 0
        if "f32 image kept" in self.mut and self.lfS is not None:
            self.dropped.append(("f32 image kept", self.lfS))
        else:
            self.lfS = None

    def flags(self):
        """(points, rung, z, backsolve, image, failed_col, factorisations) as tests/ctx_state_driver.cpp prints them.  A
        fact is held when its flag is up AND the buffer holds what the flag says: a mutation that writes into a buffer
        behind its flag's back (`predict leaks pooled mean`) shows here as the fact lost."""
        rung = 3 if self.nS is not None else 2 if self.aS is not None else 1 if self.fS is not None else 0
        return (int(self.uS is not None and "U" not in self.taint), rung, int(self.z_ok), self.backsolve,
                int(self.lfS is not None), self.failed_col, self.evals)

    # -- state --------------------------------------------------------------------------------------------------
    def set_option(self, opt, value):
        super().set_option(opt, value)
        if opt == OPT_MEMOISE:
            self.memoise = int(value) != 0
            self.events.append(f"set_memoise {int(self.memoise)}")

    def set_train(self, X, y):
        super().set_train(X, y)
        kept = (self.aS, self.nS)
        self.uS = self.lfS = None                         # release_train frees both; new_training_set:
        self._invalidate()
        if "set_train keeps alpha" in self.mut and kept[0] is not None:
            self.dropped.append(("set_train keeps alpha", kept[0]))
            self.aS, self.nS = kept
        self.evals = 0
        self.taint.discard("U")
        self.events.append("new_training_set")

    def set_params(self, expans, bias, sn2, dist_mode=DIST_DIRECT):
        e = tuple(float(v) for v in expans)
        new = (e, float(bias), float(sn2), int(dist_mode))
        same = self.have_params and self.stored == new
        if "memo ignores composition" not in self.mut:
            same = same and self.was_expans_only and self.was_white == 0.0
        elif same and self.memoise and not (self.was_expans_only and self.was_white == 0.0):
            self.dropped.append(("memo ignores composition", self.fS))
        super().set_params(expans, bias, sn2, dist_mode)
        self.stored, self.have_params = new, True
        self.was_expans_only, self.was_white = True, 0.0
        if not (same and self.memoise):
            self._invalidate()
            self.uS = None
        self.events.append("same_kernel" if same and self.memoise else "new_kernel")

    def set_kernel(self, terms, bias, white, sn2, dist_mode=DIST_DIRECT):
        super().set_kernel(terms, bias, white, sn2, dist_mode)
        e = self.stored[0] if self.stored else (0.0,) * 8
        for kd, p in self.kern["terms"]:
            if kd == xref.EXPANS:
                e = p
        self.stored, self.have_params = (e, float(bias), float(sn2), int(dist_mode)), True
        self.was_expans_only, self.was_white = self.expans_only, float(white)
        self._invalidate()
        if "set_kernel keeps U" in self.mut and self.uS is not None:
            self.dropped.append(("set_kernel keeps U", self.uS))
        else:
            self.uS = None
        self.events.append("new_kernel")

    # -- the ensure_* chain of api.hip -----------------------------------------------------------------------------
    def _ensure_U(self):
        if self.X is None or self.kern is None:
            return ESTATE
        if self.uS is None or self.uS[0] != self.tkey:          # U.n == N
            self.uS = self._cur()
            self.taint.discard("U")
            self.events.append("points_built")
        return OK

    def _ensure_factor(self):
        if self.fS is not None:
            return OK
        rc = self._ensure_U()
        if rc:
            return rc
        # factorisation_started.  The rungs are down already (no factor: nothing above it) and are left alone here, so that
        # a mutation that kept one of them up is still seen by what comes next, as it was when each fact was a flag of its own
        self._drop_side_facts()
        self.evals += 1
        self.events.append("factorisation_started")
        col = self._at(self.uS)._fit()["col"]
        self.taint.discard("factor")
        if col:
            self.failed_col = col
            self.failS = self.uS
            self.events.append(f"factorisation_failed {col}")
            return ENOTPD
        if "recovery keeps failed_column" in self.mut and self.failed_col:
            self.dropped.append(("recovery keeps failed_column", self.failed_col))
        else:
            self.failed_col = 0
        self.fS = self.uS
        if "U" in self.taint:
            self.taint.add("factor")
        self.z_ok = True                                  # the forward substitution of y / sn2 rides along
        # how the factor is substituted backwards is settled by the options it was built under (factorisation_succeeded)
        inv512, fused = self.opts.get(OPT_INV512, 1) != 0, self.opts.get(OPT_BWD_FUSED, 2)
        self.backsolve = 0 if not inv512 else {2: 3, 1: 2}.get(fused, 1)
        self.events.append(f"factorisation_succeeded 1 {int(inv512)} {fused}")
        return OK

    def _ensure_alpha(self):
        rc = self._ensure_factor()
        if rc == ENOTPD and "failed factor keeps alpha" in self.mut and self.bufA is not None:
            self.dropped.append(("failed factor keeps alpha", self.bufA))
            self.aS, self.nS = self.bufA, self.bufN
            return OK
        if rc:
            return rc
        if self.aS is not None:
            return OK
        self.taint.discard("alpha")
        if "factor" in self.taint or (self.z_ok and self.z_clobbered):
            self.taint.add("alpha")
        self.z_ok = self.z_clobbered = False              # the back substitution consumes L^-1 y / sn2
        self.aS = self.bufA = self.fS
        self.events += ["work_vectors_overwritten", "alpha_built"]
        return OK

    def _ensure_nlz(self):
        rc = self._ensure_alpha()
        if rc:
            return rc
        if self.nS is None:
            self.nS = self.bufN = self.aS
            self.events.append("nlz_built")
            self.taint.discard("nlz")
            if "alpha" in self.taint:
                self.taint.add("nlz")
        return OK

    def _answer(self, name, need, snaps, taints, *a, rc=None, **k):
        if rc is None:
            rc = {"U": self._ensure_U, "factor": self._ensure_factor, "alpha": self._ensure_alpha, "nlz": self._ensure_nlz}[need]()
        cur = self._cur()
        if rc == ENOTPD:
            S = self.failS
        elif rc:
            S = cur
        else:
            S = next((s for s in (getattr(self, n) for n in snaps) if s is not None and s != cur), cur)
        out = getattr(ModelGpak, name)(self._at(S), *a, **k)
        return _spoil(out) if rc == OK and self.taint & set(taints) else out

    # -- hot path ---------------------------------------------------------------------------------------------------
    def gram(self, want_d2=False):
        if self.X is not None and self.kern is not None:
            if "gram keeps factor" in self.mut and self.fS is not None:
                self.dropped.append(("gram keeps factor", self.fS))
                self.taint.add("factor")                  # dM holds K where the flag says L
            else:
                self._ensure_U()
                self._invalidate()
                self.events.append("matrix_overwritten")
        return self._answer("gram", "U", ("uS",), ("U",), want_d2)

    def factor(self):
        rc = self._ensure_factor()
        if rc == ESTATE:
            return ModelGpak.factor(self)                 # raises it
        return rc == OK

    def failed_column(self):
        return self.failed_col

    def chol_upper(self):
        return self._answer("chol_upper", "factor", ("fS",), ("factor",))

    def solve_alpha(self):
        return self._answer("solve_alpha", "alpha", ("aS",), ("alpha",))

    def solve_chol(self, X):
        out = self._answer("solve_chol", "factor", ("fS",), ("factor",), X)
        if self.fS is not None:
            if "solve_chol keeps z" in self.mut and self.z_ok:
                self.dropped.append(("solve_chol keeps z", self.fS))
                self.z_clobbered = True
            else:
                self.z_ok = False
                self.events.append("work_vectors_overwritten")
        return out

    def logLikelihood(self):
        return self._answer("logLikelihood", "nlz", ("nS",), ("nlz",))

    def nlz_terms(self):
        return self._answer("nlz_terms", "nlz", ("nS",), ("nlz",))

    def posteriorMeanVar(self, Xte, want_var=True, compat=0):
        snaps, rc = ["aS", "fS"], None
        if np.asarray(Xte).shape[1] == self.d:
            rc = self._ensure_nlz()
        if rc == OK:
            if self.precision == F32 and want_var:
                if self.lfS is None:
                    self.lfS = self.fS
                    self.events.append("image_built")
                snaps.append("lfS")
            if self.kern["mode"] == DIST_EXPANSION and "predict leaks pooled mean" in self.mut and self.uS is not None:
                self.dropped.append(("predict leaks pooled mean", self.uS))
                self.taint.add("U")                       # U re-centred on the train + test mean
        if rc is None:
            return ModelGpak.posteriorMeanVar(self, Xte, want_var, compat)     # refused before anything is brought up to date
        return self._answer("posteriorMeanVar", "nlz", snaps, ("alpha", "factor"), Xte, want_var, compat, rc=rc)

    def GradLL(self):
        if not self.expans_only:
            return ModelGpak.GradLL(self)                 # refused before anything is brought up to date
        return self._answer("GradLL", "nlz", ("aS", "fS"), ("alpha", "factor"))

    def GradLL_hyb(self, ng):
        return self._answer("GradLL_hyb", "nlz", ("aS", "fS"), ("alpha", "factor"), ng)

    def GradLL_exact(self, ng=10):
        return self._answer("GradLL_exact", "nlz", ("aS", "fS"), ("alpha", "factor"), ng)

    def loo(self):
        return self._answer("loo", "nlz", ("aS", "fS"), ("alpha", "factor"))

    def _blocks_ok(self, Xd):
        return self.X is not None and np.asarray(Xd).shape[1] == self.d

    def block_cross(self, Xd, nd):
        if not self._blocks_ok(Xd):
            return ModelGpak.block_cross(self, Xd, nd)
        return self._answer("block_cross", "nlz", (), (), Xd, nd)

    def predict_block(self, Xd, nd, want_var=True, latent=False):
        if not self._blocks_ok(Xd):
            return ModelGpak.predict_block(self, Xd, nd, want_var, latent)
        return self._answer("predict_block", "nlz", ("aS", "fS"), ("alpha", "factor"), Xd, nd, want_var, latent)

    def predict_joint(self, Xd, nd, want_cov=True, latent=False, prior=False):
        if not self._blocks_ok(Xd):
            return ModelGpak.predict_joint(self, Xd, nd, want_cov, latent, prior)
        return self._answer("predict_joint", "nlz", ("aS", "fS"), ("alpha", "factor"), Xd, nd, want_cov, latent, prior)

    def sample_joint(self, Xd, nd, xi, nugget=0.0, latent=False):
        if not self._blocks_ok(Xd):
            return ModelGpak.sample_joint(self, Xd, nd, xi, nugget, latent)
        return self._answer("sample_joint", "nlz", ("aS", "fS"), ("alpha", "factor"), Xd, nd, xi, nugget, latent)

    # -- the feature calls: csrc/api.hip refuses from the current state alone (single_gpu_call, the layout of the gradient, the
    # labels, the columns), then ensure_nlz, then the _impl, which reads the factor, alpha and the training points and raises no
    # event -- but gpak_condition_impl, whose solve runs through dWork (work_vectors_overwritten, csrc/condition.hip) ---------
    def _feature(self, name, *a, **k):
        probe = getattr(ModelGpak, name)(self._at(self._cur()), *a, **k)      # a refusal raises here, before anything is built
        mutation = f"{name} answers from the factor as it stands"
        if mutation in self.mut and self.nS is None:
            # no ensure_nlz: the _impl reads dM / dAlpha as the last call that built them left them
            self.dropped.append((mutation, self.bufA))
            if self.bufA is None or self.states[self.bufA][0] is None or self.states[self.bufA][0].shape != self.X.shape:
                return _spoil(probe)              # nothing there, or of another size: not the right numbers
            return getattr(ModelGpak, name)(self._at(self.bufA), *a, **k)
        rc = self._ensure_nlz()
        out = self._answer(name, "nlz", ("aS", "fS"), ("alpha", "factor"), *a, rc=rc, **k)
        if rc == OK and self.kern["mode"] == DIST_EXPANSION and f"{name} leaks pooled mean" in self.mut and self.uS is not None:
            self.dropped.append((f"{name} leaks pooled mean", self.uS))
            self.taint.add("U")                   # U re-centred on the mean pooled with the call's own points
        if rc == OK and name in ("condition", "sample_path"):
            if "condition keeps z" in self.mut:
                self.dropped.append(("condition keeps z", self.fS))
                self.z_clobbered = self.z_ok      # alpha is built first and has consumed z: z_ok is down already
            else:
                self.z_ok = False
                self.events.append("work_vectors_overwritten")
        return out

    def loo_grad(self, ng=10):
        return self._feature("loo_grad", ng)

    def cv_groups(self, labels):
        return self._feature("cv_groups", labels)

    def cv_groups_grad(self, labels, ng=10):
        return self._feature("cv_groups_grad", labels, ng)

    def cv_folds(self, labels, no_batch=False):
        return self._feature("cv_folds", labels, no_batch)

    def cv_folds_grad(self, labels, ng=10, no_batch=False):
        return self._feature("cv_folds_grad", labels, ng, no_batch)

    def design(self, Xt, nd, Xc, holes, weights=None, pick=0, want_reduction=False):
        return self._feature("design", Xt, nd, Xc, holes, weights, pick, want_reduction)

    def condition(self, Xd, nd, Ysim, Fsim=None, unfused=False):
        return self._feature("condition", Xd, nd, Ysim, Fsim, unfused)

    def sample_path(self, Xd, nd, feat_term, omega, ab, b0, E, unfused=False):
        return self._feature("sample_path", Xd, nd, feat_term, omega, ab, b0, E, unfused)

    def timing(self):
        return {"evaluations": self.evals}


# Each name drops the bring-up-to-date (ensure_nlz) of ONE factor-dependent feature call, or lets a call that pools a mean with
# its own points write the re-centred training points into U (EXPANSION form).  FEATURE_REDUNDANT: gpak_condition's
# work_vectors_overwritten comes after ensure_nlz, whose back substitution has consumed z already: dropping it changes nothing.
FEATURE_FACTOR_CALLS = ("cv_groups", "cv_groups_grad", "cv_folds", "cv_folds_grad", "design", "condition", "sample_path")
FEATURE_MUTATIONS = tuple(f"{m} answers from the factor as it stands" for m in FEATURE_FACTOR_CALLS) + \
    ("design leaks pooled mean", "condition leaks pooled mean")
FEATURE_REDUNDANT = ("condition keeps z",)


# -------------------------------------------------------------------------------------------------------------------------
# Each name drops ONE invalidation or reset of the group's three layers (csrc/multi.hip, RankCore::have_result of
# csrc/dist.hip, the replica contexts).  GROUP_MUTATIONS change an answer, a status or the count of evaluations;
# GROUP_REDUNDANT name resets that another reset covers (replica_train_ok = 0 makes ensure_replica clear replica_params_ok,
# and that clears replica_factor_ok), so dropping one of them alone changes nothing that can be observed.
GROUP_MUTATIONS = ("set_train keeps factor_current", "set_train keeps count", "set_params keeps factor_current",
                   "set_params keeps have_result", "set_train keeps replica train", "set_params keeps replica params",
                   "gram keeps replica factor", "set_params keeps general_kernel", "recovery keeps failed_column",
                   "import keeps f32 image")
GROUP_REDUNDANT = ("set_train keeps replica factor", "set_params keeps replica factor")


class _Replica:
    """What multi.hip knows about the gpak_ctx of one rank (train_ok, params_ok, factor_ok) and what that context holds:
    the training set and kernel it was last given (tS, kS: keys), the state its matrix buffer's factor was built from (fS;
    None: no factor), the state of its fp32 image (lfS), and whether the matrix buffer holds K where the group believes L."""

    def __init__(self):
        self.train_ok = self.params_ok = self.factor_ok = False
        self.tS = self.kS = self.fS = self.lfS = None
        self.N = 0
        self.holds_K = False


class GroupCaching(ModelGpak):
    """The validity logic of a group: gpak_multi (factor_current, failed_col, evaluations, general_kernel), the ranks'
    have_result / have_params, and per rank the replica flags with the replica's own factor state.  Answers come from
    ModelGpak at the snapshot the flags point at; a replica that holds something else than the flags say spoils them."""

    def __init__(self, precision=F64, cache=None, ranks=2, mut=()):
        super().__init__(precision, cache, ranks)
        unknown = [m for m in mut if m not in GROUP_MUTATIONS + GROUP_REDUNDANT]
        assert not unknown and ranks >= 2, (unknown, ranks)
        self.mut = set(mut)
        self.states = {}
        self.rep = [_Replica() for _ in range(ranks)]
        self.rS = None                        # RankCore::have_result, as the state the ranks' result was built from
        self.rank_failed = 0                  # RankCore::failed_col
        self.failS = None
        self.factor_current = False
        self.general = False
        self.have_params = False
        self.failed_col = 0
        self.evals = 0
        self.dropped = []

    _cur, _at = CachingModel._cur, CachingModel._at

    def _keeps(self, name, what=True):
        if name in self.mut and what:
            self.dropped.append((name, what))
            return True
        return False

    # -- state --------------------------------------------------------------------------------------------------------
    def set_option(self, opt, value):
        pass                                  # gpak_set_option on a group: nothing to set, GPAK_OK

    def set_train(self, X, y):
        super().set_train(X, y)               # refused (columns) before anything is stored
        for r in self.rep:
            if not self._keeps("set_train keeps replica train", r.train_ok):
                r.train_ok = False
            if not self._keeps("set_train keeps replica factor", r.factor_ok):
                r.factor_ok = False
        if not self._keeps("set_train keeps count", self.evals):
            self.evals = 0
        self.failed_col = 0
        if not self._keeps("set_train keeps factor_current", self.factor_current):
            self.factor_current = False
        self.rS = None                        # release_problem: the ranks' buffers are gone

    def _new_kernel(self, general):
        if not (self.general and not general and self._keeps("set_params keeps general_kernel")):
            self.general = general
        self.have_params = True
        for r in self.rep:
            if not self._keeps("set_params keeps replica params", r.params_ok):
                r.params_ok = False
            if not self._keeps("set_params keeps replica factor", r.factor_ok):
                r.factor_ok = False
        if not self._keeps("set_params keeps factor_current", self.factor_current):
            self.factor_current = False
        if not self._keeps("set_params keeps have_result", self.rS):
            self.rS = None

    def set_params(self, expans, bias, sn2, dist_mode=DIST_DIRECT):
        super().set_params(expans, bias, sn2, dist_mode)
        self._new_kernel(False)

    def set_kernel(self, terms, bias, white, sn2, dist_mode=DIST_DIRECT):
        super().set_kernel(terms, bias, white, sn2, dist_mode)
        self._new_kernel(True)

    # -- gpak_multi_nlz ---------------------------------------------------------------------------------------------------
    def _nlz(self):
        if self.X is None or self.kern is None:
            return ESTATE                     # the group / every rank refuses: nothing is factored, nothing counted
        fresh = not self.factor_current
        rc = OK
        if self.rS is None:
            S = self._cur()
            self.rank_failed = self._at(S)._fit()["col"]
            if self.rank_failed:
                self.failS, rc = S, ENOTPD
            else:
                self.rS = S
        if not (rc == OK and self._keeps("recovery keeps failed_column", self.failed_col)):
            self.failed_col = self.rank_failed
        if fresh:
            self.evals += 1                   # a failed factorisation is an evaluation too
        if rc == OK:
            self.factor_current = True
        return rc

    def _ask(self, name, rc, S, *a, spoil=False, **k):
        if rc == ENOTPD:
            S = self.failS
        elif rc:
            S = self._cur()                   # ModelGpak raises the same status there
        out = getattr(ModelGpak, name)(self._at(S), *a, **k)
        return _spoil(out) if spoil and rc == OK else out

    # -- the replicas (ensure_replica / replica_with_factor of multi.hip) -------------------------------------------------
    def _ensure_replica(self, r):
        p = self.rep[r]
        if not p.train_ok:
            p.tS, p.N, p.fS, p.lfS, p.holds_K = self.tkey, self.N, None, None, False     # gpak_set_train on the replica
            p.train_ok, p.params_ok = True, False
        if not p.params_ok:
            if not self.have_params:
                raise ModelError(ESTATE, "no parameters")
            p.kS, p.fS = self.kkey, None
            p.params_ok, p.factor_ok = True, False

    def _with_factor(self, r, factors_itself=False):
        """Bring replica r up to the ranks' factor as multi.hip does; returns whether the replica then holds what the group
        believes it holds.  factors_itself: the call goes through the replica's own ensure_factor (solve_chol, the factor
        copy, the gradient), which factors from what the replica holds when its matrix buffer has no factor; the sharded
        prediction reads the buffer as it is."""
        self._ensure_replica(r)
        p = self.rep[r]
        if not p.factor_ok:
            if p.N != self.N:
                raise ModelError(ESTATE, "gpak_import_factor: the context does not hold the group's training set")
            p.fS, p.holds_K, p.factor_ok = self.rS, False, True
            if not self._keeps("import keeps f32 image", p.lfS):
                p.lfS = None
        if factors_itself and p.fS is None:
            p.fS, p.holds_K = "own", False
        held = (p.tS, p.kS) == self.rS
        return held and p.fS in (self.rS, "own") and not p.holds_K

    def _on_replica0(self, name, wants_factor, *a, **k):
        if wants_factor:
            rc = self._nlz()
            if rc:
                return self._ask(name, rc, None, *a, **k)
            return self._ask(name, OK, self.rS, *a, spoil=not self._with_factor(0, True), **k)
        if self.X is None:
            raise ModelError(ESTATE, "no training set")
        self._ensure_replica(0)
        p = self.rep[0]
        return self._ask(name, OK, self._cur(), *a, spoil=(p.tS, p.kS) != (self.tkey, self.kkey), **k)


    # -- hot path ------------------------------------------------------------------------------------------------------------
    def gram(self, want_d2=False):
        out = self._on_replica0("gram", False, want_d2)
        p = self.rep[0]
        p.fS = None                           # gpak_gram on the replica: its matrix buffer holds K
        if self._keeps("gram keeps replica factor", p.factor_ok):
            p.holds_K = True
        else:
            p.factor_ok = False
        return out

    def compute_k(self, X1, X2, want_d2=False):
        out = self._on_replica0("compute_k", False, X1, X2, want_d2)
        self.rep[0].factor_ok = False         # not needed (the call leaves the matrix alone): costs one import
        return out

    def factor(self):
        rc = self._nlz()
        if rc == ESTATE:
            return ModelGpak.factor(self)
        return rc == OK

    def failed_column(self):
        return self.failed_col

    def chol_upper(self):
        return self._on_replica0("chol_upper", True)

    def solve_chol(self, X):
        return self._on_replica0("solve_chol", True, X)

    def solve_alpha(self):
        return self._ask("solve_alpha", self._nlz(), self.rS)

    def logLikelihood(self):
        return self._ask("logLikelihood", self._nlz(), self.rS)

    def nlz_terms(self):
        return self._ask("nlz_terms", self._nlz(), self.rS)

    def posteriorMeanVar(self, Xte, want_var=True, compat=0):
        Xte = np.asarray(Xte)
        if self.X is None or Xte.shape[1] != self.d:
            return ModelGpak.posteriorMeanVar(self, Xte, want_var, compat)      # GPAK_ESTATE, then GPAK_EINVAL
        rc = self._nlz()
        if rc:
            return self._ask("posteriorMeanVar", rc, None, Xte, want_var, compat)
        M = Xte.shape[0]
        per = -(-(-(-M // self.ranks)) // 256) * 256          # ceil(M / P) rounded up to 256: the slices of gpak_multi_predict
        good = True
        for r in range(self.ranks):
            if min(M, r * per) >= min(M, (r + 1) * per):
                continue                      # no slice: the replica is not even built
            good &= self._with_factor(r)
            p = self.rep[r]
            if self.precision == F32 and want_var:
                if p.lfS is None:
                    p.lfS = p.fS
                good &= p.lfS == self.rS
        return self._ask("posteriorMeanVar", OK, self.rS, Xte, want_var, compat, spoil=not good)

    def GradLL(self):
        if self.general:
            raise ModelError(ENOTIMPL, "gpak_grad handles the ExpAns(+Bias) composition only")
        return self._ask("GradLL", self._nlz(), self.rS)

    def GradLL_hyb(self, ng):
        if not self.general:
            if int(ng) != 10:
                raise ModelError(EINVAL, "the ExpAns(+Bias) composition has 10 gradient entries")
            return self._ask("GradLL_hyb", self._nlz(), self.rS, ng)
        return self._on_replica0("GradLL_hyb", True, ng)

    def timing(self):
        return {"evaluations": self.evals}
