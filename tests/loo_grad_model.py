"""gpak_loo_grad on a long-lived context: the call sequence, the models it is held to and how a step is judged.  TEST
INFRASTRUCTURE, built on tests/ctx_model.py and tests/ctx_sequences.py (their data, their classes, their bounds) without
changing them: the call is outside their vocabulary, so this file carries what they would.

  LooGradModel     ctx_model.ModelGpak + loo_grad: stateless, every answer from the current training set and kernel alone;
  LooGradCaching   ctx_model.CachingModel + loo_grad: the validity logic of csrc/api.hip, with its single mutations;
  SEQUENCE         (method, arguments by key, status due) on one context;
  run              drives it on any object with Gpak's method names; errors judges a loo_grad answer against the model's.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_model as cm  # noqa: E402
import ctx_sequences as cs  # noqa: E402
import loo_grad_ref  # noqa: E402

OK, ENOTPD, EINVAL, ESTATE, ENOTIMPL = cm.OK, cm.ENOTPD, cm.EINVAL, cm.ESTATE, cm.ENOTIMPL


class LooGradModel(cm.ModelGpak):
    def _loo_grad(self):
        """(gradient, 1/2 sum |W|): loo_grad_ref on the direct-form Gram matrix, as GradLL_exact's reference"""
        def build():
            k = self.kern
            g, W = loo_grad_ref.grad_loo(self.X, self.y, self._terms(), k["bias"], k["sn2"], want_w=True)
            return g, 0.5 * float(np.abs(W).sum())
        return self._cached("loo_grad", build)

    def loo_grad(self, ng=10):
        """What the header promises: the refusals first (no factorisation), then GPAK_ENOTPD with NaN, then the numbers"""
        self._need()
        self._grad_checks(ng)
        nan = float("nan")
        if self._fit()["col"]:
            return np.full(int(ng), nan), dict(mse=nan, mssr=nan, log_pl=nan, ms=0.0, passes=0, status=ENOTPD)
        return self._loo_grad()[0].copy(), self.loo()[2]


class LooGradCaching(cm.CachingModel):
    def _at(self, S):
        m = super()._at(S)
        m.__class__ = LooGradModel
        return m

    def loo_grad(self, ng=10):
        """CachingModel._answer("loo_grad", "nlz", ("aS", "fS"), ("alpha", "factor"), ng) after the refusals, which read
        the current composition alone"""
        cm.ModelGpak._need(self)
        self._grad_checks(ng)
        rc = self._ensure_nlz()
        cur = self._cur()
        if rc == ENOTPD:
            S = self.failS
        elif rc:
            S = cur
        else:
            S = next((s for s in (self.aS, self.fS) if s is not None and s != cur), cur)
        out = LooGradModel.loo_grad(self._at(S), ng)
        return cm._spoil(out) if rc == OK and self.taint & {"alpha", "factor"} else out


# gpak_loo_grad leaves H and W in dG / dBinv: the gradients and gpak_loo that read those workspaces next rebuild them, and it
# rebuilds them after any of those; as the first call after new parameters or a new training set it brings the factor up to
# date itself; refused (before a training set, wrong length, White child -- also at parameters that cannot be factored) or
# failed (not positive definite) it leaves the context usable.
SEQUENCE = [
    ("loo_grad", dict(ng=10), ESTATE), ("set_params", dict(kern="E"), OK), ("loo_grad", dict(ng=10), ESTATE),
    ("set_train", dict(train="T300"), OK), ("loo_grad", dict(ng=10), OK), ("loo", {}, OK),
    ("GradLL_exact", dict(ng=10), OK), ("loo_grad", dict(ng=10), OK), ("GradLL", {}, OK), ("loo_grad", dict(ng=10), OK),
    ("logLikelihood", {}, OK), ("solve_alpha", {}, OK), ("timing", {}, OK),
    ("set_params", dict(kern="T2"), OK), ("loo_grad", dict(ng=10), OK), ("posteriorMeanVar", dict(X="P5"), OK), ("loo", {}, OK),
    ("set_kernel", dict(kern="EXR"), OK), ("loo_grad", dict(ng=15), OK), ("GradLL_hyb", dict(ng=15), OK),
    ("loo_grad", dict(ng=10), EINVAL), ("loo_grad", dict(ng=15), OK),
    ("set_kernel", dict(kern="EW"), OK), ("loo_grad", dict(ng=10), ENOTIMPL), ("loo", {}, OK),
    ("set_params", dict(kern="BAD"), OK), ("loo_grad", dict(ng=11), EINVAL), ("timing", {}, OK), ("loo_grad", dict(ng=10), ENOTPD),
    ("logLikelihood", {}, OK), ("loo_grad", dict(ng=10), ENOTPD), ("timing", {}, OK),
    ("set_params", dict(kern="E13"), OK), ("loo_grad", dict(ng=10), OK), ("GradLL_exact", dict(ng=10), OK),
    ("set_train", dict(train="T700"), OK), ("loo_grad", dict(ng=10), OK), ("loo", {}, OK), ("loo_grad", dict(ng=10), OK),
    ("timing", {}, OK),
]


def ask(g, method, kw, n_train):
    """(status, [arrays]) as cs.invoke returns them; loo_grad is not in its vocabulary."""
    if method != "loo_grad":
        return cs.invoke(g, method, kw, n_train)
    try:
        grad, s = g.loo_grad(kw["ng"])
    except Exception as e:
        if getattr(e, "status", None) not in cs.API_STATUSES:   # a HIP failure: no answer, nothing more is asked of the device
            cs.DEVICE_ERROR.append(f"{method} {kw}: {e}")
            raise
        return int(e.status), []
    return int(s["status"]), [grad, np.array([s[k] for k in ("mse", "mssr", "log_pl")])]


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
                cs.must(res, "loo gradient", i, method, kw)
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
    m = LooGradModel(cm.F64, cache)
    if rec["train"]:
        m.set_train(*cs.train(rec["train"]))
    if rec["kern"]:
        ask(m, rec["kern"][0], dict(kern=rec["kern"][1]), 0)
    return m


def errors(rec, got, want, cache):
    """[(label, error, bound)] of a step's answer against the model's.  loo_grad: the bounds of
    test_loo_gradient_matches_numpy_restatement (per group; the bias entry, 1/2 sum W, also on the condition of its own sum)
    and test_loo_matches_numpy_restatement's for the summary; every other method: cs.model_errors."""
    m = model_at(rec, cache)
    if rec["method"] != "loo_grad":
        return cs.model_errors(rec["method"], rec["kw"], got, want, m)
    if got[0] != want[0]:
        return [("status", float("inf"), 1.0)]
    g, w = got[1], want[1]
    if len(g) != len(w) or any(x.shape != y.shape for x, y in zip(g, w)):
        return [("shape", float("inf"), 1.0)]
    if not w:
        return []
    if any(np.isnan(y).any() for y in w):
        return [("nan", 0.0 if all(np.array_equal(np.isnan(x), np.isnan(y)) for x, y in zip(g, w)) else float("inf"), 1.0)]
    nk = len(w[0]) - 2
    return [("kernel block", float(np.abs(g[0][:nk] - w[0][:nk]).max() / np.abs(w[0][:nk]).max()), 1e-8),
            ("bias", abs(g[0][nk] - w[0][nk]), 1e-8 * abs(w[0][nk]) + 1e-15 * m._loo_grad()[1]),
            ("sn2", abs(g[0][nk + 1] - w[0][nk + 1]) / abs(w[0][nk + 1]), 1e-8),
            ("summary", float((np.abs(g[1] - w[1]) / np.abs(w[1])).max()), 1e-8)]
