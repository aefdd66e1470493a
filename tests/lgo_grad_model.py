"""gpak_cv_groups_grad on a long-lived context: the call sequence, the models it is held to and how a step is judged.  TEST
INFRASTRUCTURE, in the manner of tests/loo_grad_model.py and built on it, on tests/ctx_model.py and on
tests/ctx_sequences.py (their data, their classes, their bounds) without changing them: the call is outside their
vocabulary, so this file carries what they would.

  GroupGradModel     loo_grad_model.LooGradModel + cv_groups_grad: stateless, every answer from the current training set,
                     kernel and labels alone;
  GroupGradCaching   loo_grad_model.LooGradCaching + cv_groups_grad: the validity logic of csrc/api.hip;
  SEQUENCE           (method, arguments by key, status due) on one context;
  run                drives it on any object with Gpak's method names; errors judges a cv_groups_grad answer against the
                     model's.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_model as cm  # noqa: E402
import ctx_sequences as cs  # noqa: E402
import cvg_ref  # noqa: E402
import lgo_grad_ref  # noqa: E402
import loo_grad_model as lgm  # noqa: E402

OK, ENOTPD, EINVAL, ESTATE, ENOTIMPL = cm.OK, cm.ENOTPD, cm.EINVAL, cm.ESTATE, cm.ENOTIMPL
GROUP_MAX = 128
SUMMARY = ("mse", "mssr", "msmd", "log_pl")

# key -> labels of n samples
GROUPS = {
    "holes100": lambda n: cvg_ref.holes(n, 100),
    "random": cvg_ref.random_groups,
    "mixed": cvg_ref.mixed_sizes,
    "big": lambda n: cvg_ref.holes(n, GROUP_MAX + 1),     # refused: a group above the limit
}


def labels_of(key, n):
    return np.asarray(GROUPS[key](int(n)), dtype=np.int64)


class GroupGradModel(lgm.LooGradModel):
    def _group_grad(self, labels):
        """(gradient, 1/2 sum |W|, summary values): lgo_grad_ref and cvg_ref on the direct-form Gram matrix"""
        def build():
            k = self.kern
            g, W = lgo_grad_ref.grad_lgo(self.X, self.y, self._terms(), k["bias"], k["sn2"], labels, want_w=True)
            s = cvg_ref.summary(self.y, *cvg_ref.cv_groups(self._fit()["K"], self.y, k["sn2"], labels))
            return g, 0.5 * float(np.abs(W).sum()), s
        return self._cached(("cv_groups_grad", cm._digest(labels)), build)

    def cv_groups_grad(self, labels, ng=10):
        """What the header promises: the refusals first (no factorisation) -- the context, the composition, the labels --
        then GPAK_ENOTPD with NaN, then the numbers"""
        self._single_only("gpak_cv_groups_grad")
        self._need()
        self._grad_checks(ng)
        labels = np.asarray(labels)
        if labels.size != self.N:
            raise ValueError("one label per training sample")
        values, group = np.unique(labels, return_inverse=True)
        sizes = np.bincount(group)
        if sizes.max() > GROUP_MAX:
            raise cm.ModelError(EINVAL, "a group has more than 128 samples")
        nan = float("nan")
        if self._fit()["col"]:
            return np.full(int(ng), nan), dict(mse=nan, mssr=nan, msmd=nan, log_pl=nan, ms=0.0, groups=int(sizes.size), max_size=0,
                                               status=ENOTPD, labels=values)
        g, _, s = self._group_grad(group)
        return g.copy(), dict(s, ms=0.0, groups=int(sizes.size), max_size=int(sizes.max()), status=OK, labels=values)


class GroupGradCaching(lgm.LooGradCaching):
    def _at(self, S):
        m = super()._at(S)
        m.__class__ = GroupGradModel
        return m

    def cv_groups_grad(self, labels, ng=10):
        """As LooGradCaching.loo_grad: the refusals read the current composition and the labels alone, then ensure_nlz, then
        the answer from the snapshot alpha and the factor were built at"""
        cm.ModelGpak._need(self)
        self._grad_checks(ng)
        if np.bincount(np.unique(np.asarray(labels), return_inverse=True)[1]).max() > GROUP_MAX:
            raise cm.ModelError(EINVAL, "a group has more than 128 samples")
        rc = self._ensure_nlz()
        cur = self._cur()
        if rc == ENOTPD:
            S = self.failS
        elif rc:
            S = cur
        else:
            S = next((s for s in (self.aS, self.fS) if s is not None and s != cur), cur)
        out = GroupGradModel.cv_groups_grad(self._at(S), labels, ng)
        return cm._spoil(out) if rc == OK and self.taint & {"alpha", "factor"} else out


# gpak_cv_groups_grad leaves H and W in dG / dBinv and its lists in the scratch buffer: the gradients, gpak_loo and
# gpak_loo_grad that use those buffers next rebuild them, and it rebuilds them after any of those; as the first call after
# new parameters or a new training set it brings the factor up to date itself; refused (before a training set, wrong length,
# a group above the limit, White child -- also at parameters that cannot be factored) or failed (not positive definite) it
# leaves the context usable.
SEQUENCE = [
    ("cv_groups_grad", dict(ng=10, groups="random"), ESTATE), ("set_params", dict(kern="E"), OK),
    ("cv_groups_grad", dict(ng=10, groups="random"), ESTATE),
    ("set_train", dict(train="T300"), OK), ("cv_groups_grad", dict(ng=10, groups="holes100"), OK), ("loo", {}, OK),
    ("GradLL_exact", dict(ng=10), OK), ("cv_groups_grad", dict(ng=10, groups="random"), OK), ("GradLL", {}, OK),
    ("cv_groups_grad", dict(ng=10, groups="holes100"), OK), ("loo_grad", dict(ng=10), OK),
    ("cv_groups_grad", dict(ng=10, groups="mixed"), OK), ("logLikelihood", {}, OK), ("solve_alpha", {}, OK), ("timing", {}, OK),
    ("set_params", dict(kern="T2"), OK), ("cv_groups_grad", dict(ng=10, groups="random"), OK),
    ("posteriorMeanVar", dict(X="P5"), OK), ("loo", {}, OK),
    ("set_kernel", dict(kern="EXR"), OK), ("cv_groups_grad", dict(ng=15, groups="holes100"), OK), ("GradLL_hyb", dict(ng=15), OK),
    ("cv_groups_grad", dict(ng=10, groups="holes100"), EINVAL), ("cv_groups_grad", dict(ng=15, groups="big"), EINVAL),
    ("cv_groups_grad", dict(ng=15, groups="random"), OK),
    ("set_kernel", dict(kern="EW"), OK), ("cv_groups_grad", dict(ng=10, groups="random"), ENOTIMPL), ("loo", {}, OK),
    ("set_params", dict(kern="BAD"), OK), ("cv_groups_grad", dict(ng=11, groups="random"), EINVAL),
    ("cv_groups_grad", dict(ng=10, groups="big"), EINVAL), ("timing", {}, OK),
    ("cv_groups_grad", dict(ng=10, groups="random"), ENOTPD), ("logLikelihood", {}, OK),
    ("cv_groups_grad", dict(ng=10, groups="random"), ENOTPD), ("timing", {}, OK),
    ("set_params", dict(kern="E13"), OK), ("cv_groups_grad", dict(ng=10, groups="mixed"), OK), ("GradLL_exact", dict(ng=10), OK),
    ("set_train", dict(train="T700"), OK), ("cv_groups_grad", dict(ng=10, groups="random"), OK), ("loo", {}, OK),
    ("cv_groups_grad", dict(ng=10, groups="random"), OK), ("timing", {}, OK),
]


def ask(g, method, kw, n_train):
    """(status, [arrays]) as cs.invoke returns them; cv_groups_grad is in neither cs.invoke's vocabulary nor lgm.ask's.
    Before a training set the labels are made for 300 samples: the call is refused before it reads them."""
    if method != "cv_groups_grad":
        return lgm.ask(g, method, kw, n_train)
    n = n_train or 300
    try:
        if not n_train and hasattr(g, "_h"):
            g.N = n                           # the binding sizes its label check by N; the library has no training set
        grad, s = g.cv_groups_grad(labels_of(kw["groups"], n), kw["ng"])
    except Exception as e:
        if getattr(e, "status", None) not in cs.API_STATUSES:   # a HIP failure: no answer, nothing more is asked of the device
            cs.DEVICE_ERROR.append(f"{method} {kw}: {e}")
            raise
        return int(e.status), []
    finally:
        if not n_train and hasattr(g, "_h"):
            g.N = 0
    return int(s["status"]), [grad, np.array([s[k] for k in SUMMARY]), np.array([s["groups"], s["max_size"]], dtype=float)]


def run(make, fresh_make=None):
    """Drive SEQUENCE on make(); one record per step: index, method, kw, train and kernel keys, result and -- with
    fresh_make, for every step that answers -- the result of a context that received only set_train, the current kernel
    call and that one method.  The object is closed unless a call failed in a way that is no answer."""
    g = make()
    train = kern = None
    fresh = {}
    out = []
    try:
        for i, (method, kw, _due) in enumerate(SEQUENCE):
            n = cs.TRAIN[train][0] if train else 0
            res = ask(g, method, kw, n)
            fr = None
            if method in cs.SETTERS:
                cs.must(res, "group gradient", i, method, kw)
                train, kern = (kw["train"], kern) if method == "set_train" else (train, (method, kw["kern"]))
            elif fresh_make is not None and method != "timing":
                key = (train, kern, method, cs.arg_key(kw))
                if key not in fresh:
                    f = fresh_make()
                    try:
                        if train:
                            cs.must(ask(f, "set_train", dict(train=train), 0), "set_train", train)
                        if kern:
                            cs.must(ask(f, kern[0], dict(kern=kern[1]), n), *kern)
                        fresh[key] = ask(f, method, kw, n)
                    finally:
                        if not cs.DEVICE_ERROR:
                            f.close()
                fr = fresh[key]
            out.append(dict(i=i, method=method, kw=kw, train=train, kern=kern, res=res, fresh=fr))
    finally:
        if not cs.DEVICE_ERROR:
            g.close()
    return out


def model_at(rec, cache):
    m = GroupGradModel(cm.F64, cache)
    if rec["train"]:
        m.set_train(*cs.train(rec["train"]))
    if rec["kern"]:
        ask(m, rec["kern"][0], dict(kern=rec["kern"][1]), 0)
    return m


def errors(rec, got, want, cache):
    """[(label, error, bound)] of a step's answer against the model's.  cv_groups_grad: the bounds of
    test_group_gradient_matches_numpy_restatement (per block; the bias entry, 1/2 sum W, also on the condition of its own
    sum), 1e-8 relative for the summary's values, the counts equal; every other method: loo_grad_model.errors."""
    if rec["method"] != "cv_groups_grad":
        return lgm.errors(rec, got, want, cache)
    if got[0] != want[0]:
        return [("status", float("inf"), 1.0)]
    g, w = got[1], want[1]
    if len(g) != len(w) or any(x.shape != y.shape for x, y in zip(g, w)):
        return [("shape", float("inf"), 1.0)]
    if not w:
        return []
    if any(np.isnan(y).any() for y in w):
        return [("nan", 0.0 if all(np.array_equal(np.isnan(x), np.isnan(y)) for x, y in zip(g, w)) else float("inf"), 1.0)]
    m = model_at(rec, cache)
    n = cs.TRAIN[rec["train"]][0]
    group = np.unique(labels_of(rec["kw"]["groups"], n), return_inverse=True)[1]
    nk = len(w[0]) - 2
    return [("kernel block", float(np.abs(g[0][:nk] - w[0][:nk]).max() / np.abs(w[0][:nk]).max()), 1e-8),
            ("bias", abs(g[0][nk] - w[0][nk]), 1e-8 * abs(w[0][nk]) + 1e-15 * m._group_grad(group)[1]),
            ("sn2", abs(g[0][nk + 1] - w[0][nk + 1]) / abs(w[0][nk + 1]), 1e-8),
            ("summary", float((np.abs(g[1] - w[1]) / np.abs(w[1])).max()), 1e-8),
            ("counts", 0.0 if np.array_equal(g[2], w[2]) else float("inf"), 1.0)]
