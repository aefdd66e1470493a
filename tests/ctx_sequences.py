"""Call sequences on one long-lived context (include/gpak.h) and how a step's answer is judged.  TEST INFRASTRUCTURE.

A step is (context index, method of gp_ss_ak_amd.gpak.Gpak, arguments BY KEY); the keys name the small fixed data
below.  The same steps run on tests/ctx_model.py (CPU) and, through tests/ctx_seq_worker.py, on libgpak_hip.so, where
every step that returns numbers is compared

  (a) bit for bit with a FRESH context of the same precision that received only the current options, set_train, the
      current kernel call and that one method, and
  (b) with ModelGpak, under the bound the method's own GPU test uses (model_errors below names the test).

Training sets (synth.drillholes / drillholes4), N chosen to cross what the state depends on and no larger:
  129 -> Np 256 (the second tile almost all padding), 300 -> 384, 700 -> 768 (a second, partial 512-column block of the
  back substitution), 1100 -> 1152 (Np >= 1024: leading-dimension pad 32, two column splits of the row-sum kernels).

Seeded random sequences: RANDOM_COUNT = 4 sequences of RANDOM_LENGTH = 36 steps, seed RANDOM_SEED + k, drawn from the
same vocabulary at N in {129, 300}; the generator keeps the preconditions (a gradient length matching the composition, no
gradient with a White child, points with the training set's columns).

A setter a sequence means to be REFUSED is a step made with no(...): run() requires exactly that status (refused, beside
must) and Track does not hear of it, so every later answer is compared with a context that never saw the call.

GROUP_SEQUENCES (further down) are the sequences on a multi-GPU context: `ranks` per context, make(precision, ranks), a
fresh answer from a fresh group of the same rank count; engine_sequence cuts them down to what a group over caller-supplied
engines answers, for the run of the group's host code on the CPU.

FEATURE_SEQUENCES (last part) bring the calls of the ten feature headers (gpak_loo_grad.h, gpak_cv_groups(_grad).h,
gpak_cv_folds(_grad).h, gpak_design.h, gpak_condition.h, gpak_local.h, gpak_local_ok.h, gpak_local_search.h) into the same
vocabulary: FEATURE_INVOKE, feature_errors, lists of their own beside SEQUENCES.  They run at T129 and T300 (the long-double
references of the design, the simulation and the local calls are cubic in N); T700 and T1100 appear in `cv workspace` alone,
for the second 512-column block and the leading-dimension change T1100 -> T300, where the float64 restatements suffice.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_model as cm  # noqa: E402
import failcol_ref  # noqa: E402
from gp_ss_ak_amd import synth  # noqa: E402

OK, ENOTPD, EINVAL, ESTATE, ENOTIMPL = cm.OK, cm.ENOTPD, cm.EINVAL, cm.ESTATE, cm.ENOTIMPL
F64, F32 = cm.F64, cm.F32
EXPANSION, DIRECT = cm.DIST_EXPANSION, cm.DIST_DIRECT
COMPAT_VARCLAMP, COMPAT_SN2SKIP = 1, 2
OPTS = {"MEMOISE": 1, "INV512": 9, "PRED_BATCH": 11, "BWD_FUSED": 12, "LOO_ROWS": 14}
EXPANS, EXP, RBF = 0, 1, 2
U = 2.0 ** -53
FILL_TOL = {DIRECT: 1e-13, EXPANSION: 2e-7}      # tests/dev_ops_cases.py FILL_TOL = test_gram_matches_oracle

# ---- the data the keys name -------------------------------------------------------------------------------------------
TRAIN = {"T129": (129, 3), "T300": (300, 3), "T700": (700, 3), "T1100": (1100, 3), "T1100d4": (1100, 4)}
E = list(synth.DEFAULT_EXPANS)
E13 = list(E)
E13[1] *= 1.3
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
# name -> (terms, bias, white, sn2)
KERN = {
    "E": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "E13": ([(EXPANS, E13)], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "Esn": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.0, 0.05),
    "T2": ([(EXPANS, THETA2)], 0.35, 0.0, 0.05),
    "ER": ([(EXPANS, E), (RBF, [0.5, 0.9, 0.5])], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "EXR": ([(EXPANS, E), (EXP, [0.5, 0.9]), (RBF, [0.5, 0.9, 0.5])], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2),
    "EW": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.05, synth.DEFAULT_SN2),
    "BAD": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.0, -0.5),          # B = I + K / sn2 is indefinite
    # ... from a CHOSEN column past the first 128-tile of T300 on (tests/failcol_ref.py: sn2 between the largest eigenvalues of
    # the leading 199- and 200-minors of K, the fixture rules asserted here, at import)
    "BAD200": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.0, failcol_ref.drill_case(300, 200)[0]),
}
BAD200_COLUMN = 200
NG = {name: sum(cm.NPARS[k] for k, _ in v[0]) + 2 for name, v in KERN.items()}
POINTS = {"P5": (5, 3), "P300": (300, 3), "P700": (700, 3), "Q5": (5, 4), "Q300": (300, 4)}
BLOCKS = {"B12x8": (12, 8, 3), "B40x8": (40, 8, 3), "B40x1": (40, 1, 3), "B300x1": (300, 1, 3), "C12x8": (12, 8, 4), "C40x1": (40, 1, 4)}
DISC = {1: (1, 1, 1), 8: (2, 2, 2)}
# what a setter must REFUSE (cs.refused): a training set of five columns, a composition with a kind that does not exist; the
# third is gpak_set_params with BAD_MODE as its distance form
BAD_TRAIN = {"T129x5": (129, 5)}
BAD_KERN = {"UNK": ([(EXPANS, E), (9, [0.5, 0.9, 0.5])], synth.DEFAULT_BIAS, 0.0, synth.DEFAULT_SN2)}
BAD_MODE = 7
TRANSPORTS = ("none", "in-process peer copies", "rccl")      # gpak_transport, as the number the sequences compare


@functools.lru_cache(maxsize=None)
def train(key):
    if key in BAD_TRAIN:
        n, d = BAD_TRAIN[key]
        X, y = synth.drillholes4(n)
        return np.asfortranarray(np.hstack([X, X[:, :d - 4]])), y
    n, d = TRAIN[key]
    X, y = synth.drillholes4(n) if d == 4 else synth.drillholes(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def points(key):
    if key.startswith("X:"):
        return train(key[2:])[0]
    m, d = POINTS[key]
    P = synth.test_points4(m) if d == 4 else synth.test_points(m)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def blocks(key):
    from gp_ss_ak_amd import gpak
    m, nd, d = BLOCKS[key]
    rng = np.random.default_rng(7000 + 100 * m + 10 * nd + d)
    c = rng.uniform(-0.9, 0.9, (m, d))
    if d == 4:
        c[:, 3] = rng.integers(0, 4, m) * (2.0 / 3.0) - 1.0
    Xd, n = gpak.block_points(c, (0.1, 0.1, 0.05), DISC[nd])
    assert n == nd
    Xd.setflags(write=False)
    return Xd, nd


@functools.lru_cache(maxsize=None)
def rhs(n, k):
    return np.asfortranarray(np.random.default_rng(31 * n + k).standard_normal((n, k)))


# ---- steps ------------------------------------------------------------------------------------------------------------
class Track:
    """What a fresh context must be given to stand where context c stands: options, training set, kernel call."""

    def __init__(self, precision, ranks=1):
        self.precision, self.ranks, self.opts, self.train, self.kern = precision, ranks, {}, None, None

    def note(self, method, kw):
        if method == "set_option":
            self.opts[kw["opt"]] = kw["value"]
        elif method == "set_train":
            self.train = kw["train"]
        elif method in ("set_params", "set_kernel"):
            self.kern = (method, kw["kern"], kw.get("mode", DIRECT))

    def key(self):
        return (self.precision, tuple(sorted(self.opts.items())), self.train, self.kern) + ((self.ranks,) if self.ranks > 1 else ())

    def state(self):
        """The state in the sense of the separation condition: training set and kernel VALUES (not the distance form,
        not the options: they change how an answer is computed, not what it is)."""
        k = self.kern
        return (self.train, None if k is None else kern_values(k[0], k[1]))


def kern_values(method, name):
    terms, bias, white, sn2 = KERN[name]
    if method == "set_params":            # gpak_set_params takes the ExpAns child alone and has no White
        terms, white = [t for t in terms if t[0] == EXPANS][:1], 0.0
    return (tuple((k, tuple(p)) for k, p in terms), bias, white, sn2)


SETTERS = ("set_option", "set_train", "set_params", "set_kernel")
API_STATUSES = (ENOTPD, EINVAL, ESTATE, ENOTIMPL)    # what the header promises as answers to a question
DEVICE_ERROR = []         # set by the first call that failed in any other way: contexts are then left unclosed ...
LEAKED = []               # ... and kept referenced here, so that no destructor calls into the library either


def invoke(obj, method, kw, n_train):
    """Call obj.method with the data the keys name; returns (status, [arrays or None])."""
    status = None
    try:
        if method in FEATURE_INVOKE:
            status, out = FEATURE_INVOKE[method](obj, kw, n_train)
        elif method == "set_option":
            out = obj.set_option(OPTS[kw["opt"]], kw["value"])
        elif method == "set_train":
            out = obj.set_train(*train(kw["train"]))
        elif method == "set_params":
            terms, bias, white, sn2 = kern_values("set_params", kw["kern"])
            out = obj.set_params(np.array(terms[0][1]), bias, sn2, kw.get("mode", DIRECT))
        elif method == "set_kernel":
            terms, bias, white, sn2 = (BAD_KERN if kw["kern"] in BAD_KERN else KERN)[kw["kern"]]
            out = obj.set_kernel(terms, bias, white, sn2, kw.get("mode", DIRECT))
        elif method == "gram":
            out = obj.gram(want_d2=kw.get("want_d2", False))
        elif method == "compute_k":
            out = obj.compute_k(points(kw["X1"]), points(kw["X2"]), want_d2=kw.get("want_d2", False))
        elif method == "solve_chol":
            out = obj.solve_chol(rhs(n_train, kw["k"]))
        elif method == "posteriorMeanVar":
            out = obj.posteriorMeanVar(points(kw["X"]), want_var=kw.get("want_var", True), compat=kw.get("compat", 0))
        elif method in ("GradLL_hyb", "GradLL_exact"):
            out = getattr(obj, method)(kw["ng"])
        elif method == "transport":
            name = obj.transport()
            out = np.array([[name.startswith(t) for t in TRANSPORTS].index(True)])
        elif method == "block_cross":
            out = obj.block_cross(*blocks(kw["blocks"]))
        elif method == "predict_block":
            out = obj.predict_block(*blocks(kw["blocks"]), want_var=kw.get("want_var", True), latent=kw.get("latent", False))
        elif method == "predict_joint":
            out = obj.predict_joint(*blocks(kw["blocks"]), want_cov=kw.get("want_cov", True), latent=kw.get("latent", False))
        elif method == "sample_joint":
            Xd, nd = blocks(kw["blocks"])
            out = obj.sample_joint(Xd, nd, np.eye(Xd.shape[0] // nd), nugget=kw.get("nugget", 0.0), latent=kw.get("latent", False))
        elif method == "timing":
            t = obj.timing()
            out = None if t is None else np.array([t["evaluations"]])
        else:
            out = getattr(obj, method)()
    except Exception as e:    # GpakError and ModelError both carry the status of include/gpak.h
        if getattr(e, "status", None) not in API_STATUSES:
            # GPAK_EHIP (a HIP failure: the device may have faulted), GPAK_ENOMEM, anything else: not an answer.  The run
            # ends here with the library's message, and nothing more is asked of the device, not even to close a context.
            DEVICE_ERROR.append(f"{method} {kw}: {e}")
            raise
        return int(e.status), []
    status = OK if status is None else int(status)
    if method == "loo":
        status = int(out[2]["status"])
        out = (out[0], out[1], np.array([out[2][k] for k in ("mse", "mssr", "log_pl")]))
    if not isinstance(out, tuple):
        out = (out,)
    return status, [None if o is None else np.atleast_1d(np.asarray(o, dtype=float)) for o in out]


def same_bits(a, b):
    """Status and every array equal bit for bit, NaN equal to NaN."""
    if a[0] != b[0] or len(a[1]) != len(b[1]):
        return False
    for x, y in zip(a[1], b[1]):
        if (x is None) != (y is None):
            return False
        if x is not None and not (x.shape == y.shape and np.array_equal(x, y, equal_nan=True)):
            return False
    return True


def make_one(make, precision, ranks):
    """make(precision) for a single context, make(precision, ranks) for a group of `ranks` ranks."""
    return make(precision) if ranks == 1 else make(precision, ranks)


def fresh_answer(make, track, method, kw, n_train):
    """The same question to a context (a group of the same rank count) that has done nothing else.  failed_column reports
    the last factorisation: the fresh context factors first."""
    g = make_one(make, track.precision, track.ranks)
    try:
        for opt, value in track.opts.items():
            must(invoke(g, "set_option", dict(opt=opt, value=value), n_train), "set_option", opt)
        if track.train:
            must(invoke(g, "set_train", dict(train=track.train), n_train), "set_train", track.train)
        if track.kern:
            must(invoke(g, track.kern[0], dict(kern=track.kern[1], mode=track.kern[2]), n_train), *track.kern)
        if method == "failed_column":
            invoke(g, "factor", {}, n_train)
        return invoke(g, method, kw, n_train)
    finally:
        if DEVICE_ERROR:
            LEAKED.append(g)
        else:
            g.close()


def must(res, *what):
    """A setter of the sequences' own vocabulary answers GPAK_OK."""
    if res[0] != OK:
        DEVICE_ERROR.append(f"{what}: status {res[0]}")
        raise RuntimeError(f"{what}: status {res[0]} where GPAK_OK was due")
    return res


def refused(res, status, *what):
    """A setter the sequence means to be REFUSED answers exactly that status; the context must then stand where it stood
    (every later step is compared with a fresh context that never saw the call)."""
    if res[0] != status:
        DEVICE_ERROR.append(f"{what}: status {res[0]} where {status} was due")
        raise RuntimeError(f"{what}: status {res[0]} where the refusal {status} was due")
    return res


def ranks_of(seq, c):
    r = seq.get("ranks", 1)
    return r[c] if isinstance(r, (tuple, list)) else r


def arg_key(kw):
    return tuple(sorted(kw.items()))


def run(seq, make, fresh_make=None, fresh_cache=None):
    """Drive the sequence; yields one record per step: index, ctx, method, kw, track key, state, result, fresh result
    (None without fresh_make, and for the setters and timing)."""
    ctxs, tracks = {}, {}
    try:
        for i, (c, method, kw) in enumerate(seq["steps"]):
            if c not in ctxs:
                ctxs[c] = make_one(make, seq["precision"], ranks_of(seq, c))
                tracks[c] = Track(seq["precision"], ranks_of(seq, c))
            tr = tracks[c]
            n_train = TRAIN[tr.train][0] if tr.train else 0
            kw = dict(kw)
            refuse = kw.pop("refuse", None)
            res = invoke(ctxs[c], method, kw, n_train)
            if method in SETTERS and refuse is not None:
                refused(res, refuse, seq["name"], i, method, kw)           # Track.note does not hear of it
            elif method in SETTERS:
                must(res, seq["name"], i, method, kw)
                tr.note(method, kw)
            fr = None
            if fresh_make is not None and method not in SETTERS and method != "timing":
                fk = (tr.key(), method, arg_key(kw))
                if fresh_cache is None or fk not in fresh_cache:
                    ans = fresh_answer(fresh_make, tr, method, kw, n_train)
                    if fresh_cache is None:
                        fr = ans
                    else:
                        fresh_cache[fk] = ans
                if fresh_cache is not None:
                    fr = fresh_cache[fk]
            yield dict(i=i, ctx=c, method=method, kw=kw, track=tr.key(), state=tr.state(), mode=tr.kern[2] if tr.kern else DIRECT,
                       train=tr.train, kern=tr.kern, ranks=tr.ranks, tracker=tr, n_train=n_train, res=res, fresh=fr)
    finally:
        if DEVICE_ERROR:
            LEAKED.extend(ctxs.values())
        else:
            for g in ctxs.values():
                g.close()


def model_at(rec, cache, precision=F64):
    """ModelGpak standing where the record's context stood."""
    m = cm.ModelGpak(precision, cache, rec.get("ranks", 1))
    if rec["train"]:
        m.set_train(*train(rec["train"]))
    if rec["kern"]:
        invoke(m, rec["kern"][0], dict(kern=rec["kern"][1], mode=rec["kern"][2]), 0)
    return m


# ---- (b): the bound each method's own GPU test uses -----------------------------------------------------------------
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def model_errors(method, kw, got, want, m, precision=F64):
    """[(label, error, bound)] of a result against the model's, both as invoke returns them.  m: the ModelGpak of the state
    (scales: max|y|, the prior variance).  An empty list: nothing numeric to compare (statuses are compared apart).
    Shapes that differ count as an infinite error."""
    if got[0] != want[0]:
        return [("status", float("inf"), 1.0)]
    g, w = got[1], want[1]
    if len(g) != len(w) or any((x is None) != (y is None) or (x is not None and x.shape != y.shape) for x, y in zip(g, w)):
        return [("shape", float("inf"), 1.0)]
    if not g or all(x is None for x in g):
        return []
    if any(np.isnan(y).any() for y in w if y is not None):      # quiet NaN where the header promises it: NaN for NaN
        ok = all(np.array_equal(np.isnan(x), np.isnan(y)) for x, y in zip(g, w) if y is not None)
        return [("nan", 0.0 if ok else float("inf"), 1.0)]
    mode = m.kern["mode"] if m.kern else DIRECT
    direct = mode == DIRECT
    # 1e-8 DIRECT / 1e-5 EXPANSION: test_predict_matches_oracle, test_reference_style_gradient_matches_oracle.  The tests of
    # loo, predict_block, predict_joint, sample_joint and GradLL_exact named below hold those methods to 1e-8 in the DIRECT form
    # and run nothing downstream of the factor in the EXPANSION form, and their references (loo_ref, block_ref, joint_ref,
    # exact_grad_ref) are direct-form: in the EXPANSION form these methods BORROW the prediction's 1e-5 (they inherit the same
    # cancellation noise of the Gram matrix through alpha and the factor); no existing test sets a bound of their own there.
    t8 = 1e-8 if direct else 1e-5
    plain = m.expans_only and m.d == 3
    if method in ("gram", "compute_k"):               # test_gram_matches_oracle; 1e-12 on D2: test_other_kernel_compositions, test_four_column_inputs
        out = [("K", rel(g[0], w[0]), 1e-13 if direct else 2e-7)]
        if len(g) > 1 and g[1] is not None:
            out.append(("D2", float(np.abs(g[1] - w[1]).max()), (1e-14 if direct else 1e-13) if plain else 1e-12))
        return out
    if method in FEATURE_INVOKE:
        return feature_errors(method, kw, g, w, m, t8, direct)
    if method in ("factor", "n_gpus", "transport"):   # yes / no, a count, a name: equal or not
        return [(method, float(g[0][0] != w[0][0]), 0.5)]
    if method == "failed_column":                     # the column itself: an integer, equal or not (tests/failcol_ref.py)
        return [("failed_column", float(g[0][0] != w[0][0]), 0.5)]
    if method == "chol_upper":                        # test_factor_alpha_nlz_match_oracle (direct form)
        assert direct
        return [("R", rel(g[0], w[0]), 1e-11)]
    if method in ("solve_alpha", "solve_chol"):       # test_factor_alpha_nlz_match_oracle, test_other_kernel_compositions
        return [("x", rel(g[0], w[0]), t8)]
    if method == "logLikelihood":                     # 1e-9 direct, 1e-6 expansion: test_other_kernel_compositions
        return [("nlz", abs(g[0][0] - w[0][0]) / abs(w[0][0]), 1e-9 if direct else 1e-6)]
    if method == "nlz_terms":                         # test_factor_alpha_nlz_match_oracle
        b = [1e-9, 1e-9, 1e-11] if direct else [1e-6] * 3
        return [(n, abs(g[k][0] - w[k][0]) / abs(w[k][0]), b[k]) for k, n in enumerate(("quad", "sumlp", "logdet"))]
    if method == "posteriorMeanVar":                  # test_predict_matches_oracle; fp32: test_fp32_prediction_context
        out = [("mean", rel(g[0], w[0]), 1e-8 if precision == F32 else t8)]
        if g[1] is not None:
            out.append(("var", rel(g[1], w[1]), 2e-4 if precision == F32 else t8))
        return out
    if method in ("GradLL", "GradLL_hyb"):
        return [("g", float(np.abs(g[0] - w[0]).max() / np.abs(w[0]).max()), t8)]
    if method == "GradLL_exact":                      # test_exact_gradient_matches_numpy_restatement: per group
        nk = len(w[0]) - 2
        return [("kernel block", float(np.abs(g[0][:nk] - w[0][:nk]).max() / np.abs(w[0][:nk]).max()), t8),
                ("bias", abs(g[0][nk] - w[0][nk]) / abs(w[0][nk]), t8), ("sn2", abs(g[0][nk + 1] - w[0][nk + 1]) / abs(w[0][nk + 1]), t8)]
    ymax, pv = float(np.abs(m.y).max()), m.prior_variance()
    if method == "loo":                               # test_loo_matches_numpy_restatement (DIRECT; EXPANSION: borrowed, see t8)
        return [("mean", float(np.abs(g[0] - w[0]).max() / ymax), t8), ("var", float((np.abs(g[1] - w[1]) / w[1]).max()), t8),
                ("summary", float((np.abs(g[2] - w[2]) / np.abs(w[2])).max()), t8)]
    if method == "block_cross":                       # test_block_cross_against_long_double / _in_the_expansion_form
        nd = BLOCKS[kw["blocks"]][1]
        wl = np.abs(w[0])
        bound = FILL_TOL[mode] * float(wl.max()) + (nd + 2) * U * wl
        return [("kbar", float((np.abs(g[0] - w[0]) / bound).max()), 1.0)]
    if method == "predict_block":                     # test_predict_block_matches_numpy_reference (DIRECT; EXPANSION: borrowed, see t8)
        out = [("mean", float(np.abs(g[0] - w[0]).max() / ymax), t8)]
        if g[1] is not None:
            out.append(("var", float(np.abs(g[1] - w[1]).max() / pv), t8))
        return out
    if method == "predict_joint":                     # test_predict_joint_matches_numpy_reference (DIRECT; EXPANSION: borrowed, see t8)
        out = [("mean", float(np.abs(g[0] - w[0]).max() / ymax), t8)]
        if g[1] is not None:
            out.append(("cov", float(np.abs(g[1] - w[1]).max() / pv), t8))
        return out
    if method == "sample_joint":
        # The normals are the identity, so Z - mean 1' is the factor Lc itself (test_identity_normals_return_the_factor).
        # Lc Lc' against the MODEL's covariance + nugget I: the covariance's own bound t8 * prior variance
        # (test_predict_joint_matches_numpy_reference) plus the backward error of the factorisation, 8 (M + 1) u max diag
        # (test_identity_normals_return_the_factor), plus the rounding of Z = mean + Lc taken away again:
        # |d_ij| <= u (|mean_i| + |Lc_ij|), which moves (Lc Lc')_ij by at most 2 u (max|mean| + sqrt(max diag)) sqrt(M max diag)
        # (Cauchy-Schwarz on a row of Lc).  A factor's conditioning does not enter: the product is compared, not Lc.
        Xd, nd = blocks(kw["blocks"])
        M = Xd.shape[0] // nd
        _, cov = m.predict_joint(Xd, nd, latent=kw.get("latent", False))
        A = cov + kw.get("nugget", 0.0) * np.eye(M)
        Lc = g[0].astype(np.longdouble) - g[1].astype(np.longdouble)[:, None]
        dmax = float(np.diag(A).max())
        bound = t8 * pv + 8 * (M + 1) * U * dmax + 2 * U * (float(np.abs(g[1]).max()) + dmax ** 0.5) * (M * dmax) ** 0.5
        return [("mean", float(np.abs(g[1] - w[1]).max() / ymax), t8),
                ("Lc Lc'", float(np.abs((Lc @ Lc.T).astype(float) - A).max()), bound),
                ("above the diagonal", float(np.abs(np.triu(Lc.astype(float), 1)).max()), 4 * U * float(np.abs(g[1]).max()) + 1e-300)]
    raise AssertionError(method)


def worst(errs):
    return max([0.0] + [e / b for _, e, b in errs])


# ---- the named sequences -------------------------------------------------------------------------------------------------
def S(method, ctx=0, **kw):
    return (ctx, method, kw)


def opt(name, value, ctx=0):
    return S("set_option", ctx, opt=name, value=value)


def everything(pts, b8, b1, ng=10, hyb=False, ctx=0):
    """predict with variance, predict_block, predict_joint, sample_joint, loo and the gradients of the composition"""
    out = [S("posteriorMeanVar", ctx, X=pts), S("predict_block", ctx, blocks=b8), S("predict_joint", ctx, blocks=b1),
           S("sample_joint", ctx, blocks=b1), S("loo", ctx)]
    out += [S("GradLL_hyb", ctx, ng=ng)] if hyb else [S("GradLL", ctx)]
    return out + [S("GradLL_exact", ctx, ng=ng)]


def seq_memo():
    """GPAK_OPT_MEMOISE: gpak_set_params after a composition whose ExpAns child, bias, sn2 and distance form are the
    values it is given (an extra child; a White child), and the reverse; identical values rebuild nothing (the count of
    factorisations stands still); the distance form alone, sn2 alone rebuild."""
    s = [opt("MEMOISE", 1), S("set_train", train="T300")]
    for comp in ("ER", "EW"):
        s += [S("set_kernel", kern=comp), S("logLikelihood"), S("timing"),
              S("set_params", kern="E"), S("logLikelihood"), S("timing"), S("solve_alpha"), S("posteriorMeanVar", X="P5"), S("loo"),
              S("GradLL"), S("nlz_terms"),
              S("set_params", kern="E"), S("logLikelihood"), S("timing"), S("solve_alpha")]          # identical: nothing rebuilt
    s += [S("set_kernel", kern="ER"), S("logLikelihood"), S("timing"), S("set_kernel", kern="EW"), S("logLikelihood"), S("loo"),
          S("set_kernel", kern="EW"), S("logLikelihood"), S("timing"),                                 # set_kernel always rebuilds
          S("set_params", kern="E"), S("logLikelihood"), S("timing"),
          S("set_params", kern="E", mode=EXPANSION), S("logLikelihood"), S("timing"), S("nlz_terms"),
          S("set_params", kern="E", mode=EXPANSION), S("logLikelihood"), S("timing"),
          S("set_params", kern="Esn", mode=EXPANSION), S("logLikelihood"), S("timing"), S("nlz_terms"),
          opt("MEMOISE", 0), S("set_params", kern="Esn", mode=EXPANSION), S("logLikelihood"), S("timing")]
    return s


def seq_gram_between(mode):
    """gpak_gram reuses the matrix buffer: whatever factor it held is gone, alpha and nlZ with it.  In the expansion form
    a prediction centres ITS copy of the training points on the train + test mean: the Gram matrices after it must still
    be centred on the training mean."""
    s = [S("set_train", train="T300"), S("set_params", kern="T2", mode=mode), S("logLikelihood"),
         S("set_params", kern="E", mode=mode), S("logLikelihood"), S("gram", want_d2=True), S("solve_alpha"),
         S("posteriorMeanVar", X="P300"), S("loo"), S("compute_k", X1="X:T300", X2="P5", want_d2=True), S("gram"),
         S("posteriorMeanVar", X="P5", compat=COMPAT_VARCLAMP | COMPAT_SN2SKIP), S("predict_block", blocks="B12x8"), S("gram"),
         S("logLikelihood"), S("nlz_terms")]
    if mode == DIRECT:
        s += [S("gram"), S("chol_upper")]
    return s


def seq_size_walk():
    """N 300 -> 1100 -> 129 -> 1100 with 3 -> 4 -> 3 -> 3 input columns: buffers grown at the large size are used at the
    small one and the other way round; the kernel is set once per column count and survives gpak_set_train."""
    s = [S("set_train", train="T300"), S("set_params", kern="E")] + everything("P300", "B12x8", "B40x1")
    s += [S("set_train", train="T1100d4"), S("set_params", kern="T2")] + everything("Q300", "C12x8", "C40x1")
    s += [S("set_train", train="T129")] + everything("P300", "B12x8", "B40x1")
    s += [S("set_train", train="T1100")] + everything("P300", "B12x8", "B40x1")
    return s


def seq_prediction_buffers(mode, ctx=0):
    """dWt / dPart / dPv / dXte / Upred / Tq are shared by the point, block and joint paths, dXblk / dTblk / dC by the
    block and joint ones; M = 700 under GPAK_OPT_PRED_BATCH = 256 is three batches with a ragged last one."""
    c = dict(ctx=ctx)
    return [S("set_train", train="T700", **c), S("set_params", kern="E", mode=mode, **c), opt("PRED_BATCH", 256, ctx),
            S("posteriorMeanVar", X="P700", **c), S("predict_block", blocks="B40x8", **c), S("predict_joint", blocks="B300x1", **c),
            S("sample_joint", blocks="B300x1", **c), opt("PRED_BATCH", 0, ctx), S("posteriorMeanVar", X="P5", **c),
            S("block_cross", blocks="B40x8", **c), opt("PRED_BATCH", 256, ctx), S("posteriorMeanVar", X="P700", want_var=False, **c),
            S("set_params", kern="T2", mode=mode, **c), S("posteriorMeanVar", X="P700", **c), S("predict_block", blocks="B40x8", latent=True, **c),
            S("predict_joint", blocks="B40x8", latent=True, **c), opt("PRED_BATCH", 0, ctx), S("posteriorMeanVar", X="P300", **c),
            S("gram", **c), S("logLikelihood", **c)]


def seq_solve_scratch():
    """dWork: L^-1 y / sn2 from the factorisation, the right-hand sides of gpak_solve_chol, the back substitution's
    scratch.  GPAK_OPT_INV512 / GPAK_OPT_BWD_FUSED change between calls without a gpak_set_params, then with one."""
    return [S("set_train", train="T700"), S("set_params", kern="E"), S("factor"), S("solve_chol", k=3), S("solve_alpha"),
            S("logLikelihood"), S("solve_chol", k=1), S("GradLL"), S("solve_alpha"), S("chol_upper"),
            opt("INV512", 0), S("solve_chol", k=3), S("solve_alpha"), opt("BWD_FUSED", 0), opt("INV512", 1), S("solve_chol", k=1),
            S("logLikelihood"),
            S("set_params", kern="E13"), S("solve_chol", k=3), S("solve_alpha"), S("logLikelihood"),
            opt("BWD_FUSED", 1), S("set_params", kern="E"), S("solve_alpha"), S("solve_chol", k=1),
            opt("INV512", 0), S("set_params", kern="E13"), S("solve_chol", k=3), S("solve_alpha"), S("nlz_terms"),
            opt("INV512", 1), opt("BWD_FUSED", 2), S("set_params", kern="E"), S("solve_alpha"), S("chol_upper")]


def seq_fail_and_recover():
    """sn2 = -0.5: the factorisation fails.  NaN / GPAK_ENOTPD where the header promises them, the same failing values
    again under memoisation still fail, and good parameters afterwards answer as a fresh context does."""
    al = [S("logLikelihood"), S("failed_column"), S("solve_alpha")] + everything("P5", "B12x8", "B40x1")
    bad = [S("logLikelihood"), S("failed_column"), S("loo"), S("predict_block", blocks="B12x8"), S("predict_joint", blocks="B40x1"),
           S("sample_joint", blocks="B40x1"), S("block_cross", blocks="B12x8"), S("GradLL"), S("GradLL_exact", ng=10),
           S("posteriorMeanVar", X="P5"), S("solve_alpha"), S("nlz_terms"), S("factor"), S("failed_column")]
    return ([S("set_train", train="T300"), S("set_params", kern="E")] + al + [S("set_params", kern="BAD")] + bad +
            [opt("MEMOISE", 1), S("set_params", kern="BAD"), S("logLikelihood"), S("timing"), S("failed_column"), S("loo"),
             S("set_params", kern="BAD200"), S("logLikelihood"), S("failed_column"),      # ... and at column 200, not 1
             S("set_params", kern="E13")] + al + [S("chol_upper"), S("timing")])


def seq_gradients(ctx=0):
    """dG / dGpart are shared by the three gradients and gpak_loo; a refused gradient leaves the context as it was."""
    c = dict(ctx=ctx)
    return [S("set_train", train="T300", **c), S("set_params", kern="E", **c), S("GradLL", **c), S("loo", **c), S("GradLL_exact", ng=10, **c),
            S("set_params", kern="E13", **c), S("loo", **c), S("GradLL", **c),
            S("set_kernel", kern="ER", **c), S("GradLL_hyb", ng=13, **c), S("GradLL_exact", ng=13, **c), S("GradLL", **c),
            S("logLikelihood", **c), S("solve_alpha", **c), S("GradLL_exact", ng=10, **c),
            S("set_kernel", kern="EXR", **c), S("GradLL_hyb", ng=15, **c), S("loo", **c), S("GradLL_exact", ng=15, **c),
            S("set_kernel", kern="EW", **c), S("GradLL_exact", ng=10, **c), S("loo", **c), S("logLikelihood", **c),
            S("set_params", kern="T2", **c), S("GradLL_exact", ng=10, **c), S("GradLL", **c)]


def seq_f32():
    """GPAK_F32: the fp32 image of the factor follows new parameters and a new training set; loo, predict_block and
    predict_joint in between are fp64 per the header."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("posteriorMeanVar", X="P300"), S("loo"),
            S("set_params", kern="T2"), S("posteriorMeanVar", X="P300"), S("predict_block", blocks="B12x8"),
            S("set_train", train="T1100"), S("posteriorMeanVar", X="P300"), S("predict_joint", blocks="B40x1"),
            S("set_params", kern="E"), S("loo"), S("posteriorMeanVar", X="P300"), S("posteriorMeanVar", X="P5", want_var=False),
            S("set_train", train="T129"), S("posteriorMeanVar", X="P300")]


def seq_two_contexts():
    """Two live contexts of different N advanced alternately, step by step."""
    a, b = seq_prediction_buffers(DIRECT, 0), seq_gradients(1)
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


def seq_out_of_order():
    """Calls before gpak_set_train and before any parameters return GPAK_ESTATE and leave the context usable;
    gpak_set_params before gpak_set_train; gpak_set_train twice."""
    early = ["logLikelihood", "nlz_terms", "solve_alpha", "gram", "factor", "loo", "GradLL"]
    s = [S(m) for m in early] + [S("GradLL_exact", ng=10), S("posteriorMeanVar", X="P5"), S("predict_block", blocks="B12x8"),
                                 S("predict_joint", blocks="B40x1"), S("sample_joint", blocks="B40x1"), S("failed_column")]
    s += [S("set_params", kern="E")] + [S(m) for m in early] + [S("posteriorMeanVar", X="P5"), S("predict_block", blocks="B12x8"),
                                                                 S("compute_k", X1="P300", X2="P5")]
    s += [S("set_train", train="T129"), S("logLikelihood"), S("solve_alpha"), S("posteriorMeanVar", X="P5")]
    s += [S("set_train", ctx=1, train="T129")] + [S(m, ctx=1) for m in early] + [S("predict_block", ctx=1, blocks="B12x8"),
                                                                                  S("posteriorMeanVar", ctx=1, X="P5"),
                                                                                  S("posteriorMeanVar", ctx=1, X="Q5")]
    s += [S("set_params", ctx=1, kern="E13"), S("logLikelihood", ctx=1), S("loo", ctx=1)]
    s += [S("set_train", train="T300"), S("set_train", train="T129"), S("logLikelihood"), S("solve_alpha"), S("loo"),
          S("posteriorMeanVar", X="Q5"), S("logLikelihood")]
    return s


RANDOM_SEED, RANDOM_COUNT, RANDOM_LENGTH = 20171027, 4, 36


def seq_random(k):
    rng = np.random.default_rng(RANDOM_SEED + k)
    pick = lambda a: a[int(rng.integers(len(a)))]   # noqa: E731
    cur = dict(train=None, kern=None)

    def set_train():
        cur["train"] = pick(["T129", "T300"])
        return S("set_train", train=cur["train"])

    def set_kern():
        cur["kern"] = pick(["E", "E13", "T2", "Esn", "ER", "EXR", "EW"])
        if cur["kern"] in ("ER", "EXR", "EW"):
            return S("set_kernel", kern=cur["kern"])
        return S("set_params", kern=cur["kern"])

    steps = [set_train(), set_kern()]
    plain = lambda: cur["kern"] in ("E", "E13", "T2", "Esn")   # noqa: E731
    while len(steps) < RANDOM_LENGTH:
        r = rng.random()
        if r < 0.08:
            steps.append(set_train())
        elif r < 0.25:
            steps.append(set_kern())
        elif r < 0.33:
            steps.append(opt(*pick([("PRED_BATCH", 256), ("PRED_BATCH", 0), ("LOO_ROWS", 128), ("LOO_ROWS", 0), ("MEMOISE", 1), ("MEMOISE", 0)])))
        else:
            m = pick(["gram", "factor", "solve_alpha", "solve_chol", "logLikelihood", "nlz_terms", "posteriorMeanVar", "grad", "exact", "loo",
                      "block_cross", "predict_block", "predict_joint", "sample_joint", "compute_k", "chol_upper"])
            ng = NG[cur["kern"]]
            if m == "grad":
                if cur["kern"] == "EW":
                    continue
                steps.append(S("GradLL") if plain() else S("GradLL_hyb", ng=ng))
            elif m == "exact":
                if cur["kern"] == "EW":
                    continue
                steps.append(S("GradLL_exact", ng=ng))
            elif m == "solve_chol":
                steps.append(S("solve_chol", k=int(rng.integers(1, 4))))
            elif m == "posteriorMeanVar":
                steps.append(S("posteriorMeanVar", X=pick(["P5", "P300"]), want_var=bool(rng.integers(2))))
            elif m == "compute_k":
                steps.append(S("compute_k", X1="P300", X2="P5"))
            elif m in ("block_cross", "predict_block"):
                steps.append(S(m, blocks=pick(["B12x8", "B40x1"])))
            elif m in ("predict_joint", "sample_joint"):
                steps.append(S(m, blocks=pick(["B12x8", "B40x1"])))
            else:
                steps.append(S(m))
    return steps


def _seq(name, group, steps, precision=F64, doc=""):
    return dict(name=name, group=group, steps=steps, precision=precision, doc=doc)


SEQUENCES = [
    _seq("memo", "memo", seq_memo()),
    _seq("gram between [direct]", "gram", seq_gram_between(DIRECT)),
    _seq("gram between [expansion]", "gram", seq_gram_between(EXPANSION)),
    _seq("size walk", "walk", seq_size_walk()),
    _seq("prediction buffers [direct]", "pred", seq_prediction_buffers(DIRECT)),
    _seq("prediction buffers [expansion]", "pred", seq_prediction_buffers(EXPANSION)),
    _seq("solve scratch", "solve", seq_solve_scratch()),
    _seq("fail and recover", "fail", seq_fail_and_recover()),
    _seq("gradients", "grad", seq_gradients()),
    _seq("f32", "f32", seq_f32(), F32),
    _seq("two contexts", "two", seq_two_contexts()),
    _seq("out of order", "order", seq_out_of_order()),
] + [_seq(f"random {k}", "random", seq_random(k)) for k in range(RANDOM_COUNT)]
GROUPS = []
for _s in SEQUENCES:
    if _s["group"] not in GROUPS:
        GROUPS.append(_s["group"])
BY_NAME = {s["name"]: s for s in SEQUENCES}

# which function of include/gpak.h a step reaches (gpak_create / gpak_destroy / gpak_last_error: every context made, closed,
# every status turned into GpakError)
ENTRY = {"set_option": "gpak_set_option", "set_train": "gpak_set_train", "set_params": "gpak_set_params", "set_kernel": "gpak_set_kernel",
         "gram": "gpak_gram", "compute_k": "gpak_compute_k", "factor": "gpak_factor", "failed_column": "gpak_failed_column",
         "chol_upper": "gpak_get_chol_upper", "solve_alpha": "gpak_solve_alpha", "solve_chol": "gpak_solve_chol", "logLikelihood": "gpak_nlz",
         "nlz_terms": "gpak_nlz_terms", "posteriorMeanVar": "gpak_predict", "GradLL": "gpak_grad", "GradLL_hyb": "gpak_grad_hyb",
         "GradLL_exact": "gpak_grad_exact", "loo": "gpak_loo", "block_cross": "gpak_block_cross", "predict_block": "gpak_predict_block",
         "predict_joint": "gpak_predict_joint", "sample_joint": "gpak_sample_joint", "timing": "gpak_timing"}
ALWAYS = {"gpak_create", "gpak_destroy", "gpak_last_error"}


# ---- refused setters: the context stands where it stood -------------------------------------------------------------------
def no(method, status, ctx=0, **kw):
    """A setter call that must be refused with `status` (run: cs.refused)."""
    return (ctx, method, dict(kw, refuse=status))


def seq_refused_setters():
    """A refused gpak_set_train (five columns), gpak_set_params (a distance form that does not exist) and gpak_set_kernel (an
    unknown kind) change nothing: the sizes the binding allocates by, the parameters, the composition and what is cached."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"),
            no("set_train", ENOTIMPL, train="T129x5"), S("solve_alpha"), S("logLikelihood"), S("posteriorMeanVar", X="P5"), S("timing"),
            no("set_params", EINVAL, kern="E13", mode=BAD_MODE), S("logLikelihood"), S("GradLL"), S("timing"),
            no("set_kernel", EINVAL, kern="UNK"), S("logLikelihood"), S("GradLL"), S("timing"),
            S("set_params", kern="T2"), S("logLikelihood"), no("set_train", ENOTIMPL, train="T129x5"), S("solve_alpha"), S("loo"),
            S("set_train", train="T129"), no("set_kernel", EINVAL, kern="UNK"), S("solve_alpha"), S("gram"), S("timing")]


SEQUENCES.append(_seq("refused setters", "refused", seq_refused_setters()))
GROUPS.append("refused")
BY_NAME["refused setters"] = SEQUENCES[-1]
ENTRY.update(n_gpus="gpak_n_gpus", transport="gpak_transport", loo_grad="gpak_loo_grad")


# ---- sequences on a group (gpak_create_multi): DESIGN.md section 8, "Call sequences on a multi-GPU context" -----------------
# The group's block width is 512.  T129: Np 256, one block column (P = 2: rank 1 owns nothing).  T700: Np 768, columns
# 512 + 256 (P = 2: one each; P = 3: rank 2 owns nothing).  T1100 / T1100d4: Np 1152, 512 + 512 + 128, leading-dimension pad 32
# (P = 2: rank 0 owns two; P = 3: one each).  Prediction is sharded in slices of ceil(M / P) rounded up to 256: P5 -> rank 0
# alone (the other replicas are not even built); P300 at P = 2 -> 256 + 44; P700 -> 512 + 188 (P = 2), 256 + 256 + 188 (P = 3).
REFUSED_ON_A_GROUP = ("GradLL_exact", "loo", "loo_grad", "predict_block", "block_cross", "predict_joint", "sample_joint")


def g_all(pts, ctx=0, hyb=None):
    """what a group answers from one factorisation: sharded prediction, the calls on replica 0, the distributed ones"""
    c = dict(ctx=ctx)
    return [S("posteriorMeanVar", X=pts, **c), S("solve_chol", k=2, **c), S("logLikelihood", **c), S("nlz_terms", **c), S("solve_alpha", **c),
            S("GradLL_hyb", ng=hyb, **c) if hyb else S("GradLL", **c), S("timing", **c)]


def seq_g_count():
    """gpak_set_train while the parameters stay: evaluations and the accumulated times restart at the new set's FIRST
    factorisation; gpak_set_params before gpak_set_train; gpak_set_train twice; the same values set again factor again."""
    return [S("set_params", kern="E"), S("set_train", train="T300"), S("logLikelihood"), S("timing"), S("logLikelihood"), S("timing"),
            S("set_train", train="T129"), S("logLikelihood"), S("timing"), S("solve_alpha"), S("timing"),
            S("set_params", kern="E13"), S("GradLL"), S("timing"), S("nlz_terms"), S("timing"),
            S("set_train", train="T300"), S("set_train", train="T129"), S("timing"), S("factor"), S("timing"),
            S("set_params", kern="E13"), S("logLikelihood"), S("timing"), S("posteriorMeanVar", X="P5"), S("timing"),
            S("set_params", kern="E"), S("solve_alpha"), S("timing")]


def seq_g_late(ctx=0):
    """A replica first used late: P5 is rank 0's alone, then new parameters, then P700 builds replicas 1 .. P-1, which must
    take the CURRENT training set, kernel and factor; then a new training set and P300."""
    c = dict(ctx=ctx)
    return [S("set_train", train="T700", **c), S("set_params", kern="E", **c), S("posteriorMeanVar", X="P5", **c),
            S("set_params", kern="T2", **c), S("posteriorMeanVar", X="P700", **c), S("timing", **c),
            S("set_train", train="T1100", **c), S("posteriorMeanVar", X="P300", **c), S("solve_chol", k=2, **c), S("timing", **c),
            S("set_params", kern="E13", **c), S("posteriorMeanVar", X="P700", want_var=False, **c), S("posteriorMeanVar", X="P5", **c),
            S("timing", **c)]


def seq_g_gram(mode, ctx=0):
    """gpak_gram / gpak_compute_k run on replica 0 and overwrite its matrix: the prediction, solve_chol and the factor copy
    after them import the ranks' factor again, and nothing is factored again (evaluations stand still).  In the EXPANSION
    form the sharded prediction centres on the pooled mean of ALL test points."""
    c = dict(ctx=ctx)
    s = [S("set_train", train="T300", **c), S("set_params", kern="T2", mode=mode, **c), S("logLikelihood", **c),
         S("set_params", kern="E", mode=mode, **c), S("logLikelihood", **c), S("timing", **c), S("gram", want_d2=True, **c),
         S("posteriorMeanVar", X="P300", **c), S("compute_k", X1="X:T300", X2="P5", want_d2=True, **c), S("solve_chol", k=3, **c),
         S("gram", **c), S("solve_chol", k=1, **c), S("solve_alpha", **c), S("gram", **c), S("posteriorMeanVar", X="P700", **c),
         S("timing", **c)]
    if mode == DIRECT:
        s += [S("gram", **c), S("chol_upper", **c)]
    return s + [S("nlz_terms", **c), S("timing", **c)]


def seq_g_compositions():
    """gpak_set_kernel <-> gpak_set_params: gpak_grad on a composition is refused and leaves the group usable; gpak_grad_hyb
    with the composition's length runs on replica 0 from the distributed factor; a wrong length is GPAK_EINVAL; a White child."""
    return [S("set_train", train="T300"), S("set_kernel", kern="ER"), S("GradLL"), S("logLikelihood"), S("GradLL_hyb", ng=13),
            S("posteriorMeanVar", X="P300"), S("timing"),
            S("set_params", kern="E"), S("GradLL"), S("GradLL_hyb", ng=13), S("GradLL_hyb", ng=10), S("posteriorMeanVar", X="P300"),
            S("set_kernel", kern="EW"), S("logLikelihood"), S("GradLL_hyb", ng=10), S("GradLL"), S("posteriorMeanVar", X="P5"),
            S("solve_chol", k=1),
            S("set_kernel", kern="EXR"), S("GradLL_hyb", ng=15), S("GradLL_hyb", ng=13), S("solve_alpha"),
            S("set_params", kern="T2"), S("GradLL"), S("timing")]


def seq_g_fail():
    """sn2 = -0.5: NaN and GPAK_ENOTPD as the header promises, every ask of failing values factors (and counts) again, the
    calls on the replicas import nothing; good parameters afterwards answer as a fresh group does."""
    bad = [S("logLikelihood"), S("failed_column"), S("timing"), S("logLikelihood"), S("timing"), S("factor"), S("solve_alpha"),
           S("nlz_terms"), S("GradLL"), S("posteriorMeanVar", X="P5"), S("solve_chol", k=1), S("chol_upper"), S("timing")]
    return ([S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"), S("failed_column"),
             S("set_params", kern="BAD")] + bad + [S("set_params", kern="BAD"), S("logLikelihood"), S("failed_column"), S("timing"),
                                                   S("set_params", kern="BAD200"), S("logLikelihood"), S("failed_column"), S("timing"),
                                                   S("set_params", kern="E13"), S("logLikelihood"), S("failed_column"),
                                                   S("posteriorMeanVar", X="P5"), S("solve_chol", k=1), S("chol_upper"), S("timing")])


def seq_g_walk():
    """N 300 -> 1100 (four columns) -> 129 -> 1100: one, three, one, three block columns; the ranks' and the replicas' buffers
    follow; points with the wrong number of columns are refused and change nothing."""
    return ([S("set_train", train="T300"), S("set_params", kern="E")] + g_all("P300") + [S("posteriorMeanVar", X="Q5")] +
            [S("set_train", train="T1100d4"), S("set_params", kern="T2")] + g_all("Q300") + [S("posteriorMeanVar", X="P5")] +
            [S("set_train", train="T129")] + g_all("P300") + [S("set_train", train="T1100")] + g_all("P700"))


def seq_g_f32():
    """GPAK_F32 group: the replicas' fp32 image of the IMPORTED factor follows new parameters and a new training set."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("posteriorMeanVar", X="P300"),
            S("set_params", kern="T2"), S("posteriorMeanVar", X="P300"),
            S("set_train", train="T1100"), S("posteriorMeanVar", X="P700"),
            S("set_params", kern="E"), S("posteriorMeanVar", X="P300"), S("posteriorMeanVar", X="P5", want_var=False),
            S("set_train", train="T129"), S("posteriorMeanVar", X="P300")]


def refusals(ctx=0):
    c = dict(ctx=ctx)
    return [S("GradLL_exact", ng=10, **c), S("loo", **c), S("loo_grad", ng=10, **c), S("predict_block", blocks="B12x8", **c),
            S("block_cross", blocks="B12x8", **c), S("predict_joint", blocks="B40x1", **c), S("sample_joint", blocks="B40x1", **c)]


def seq_g_refusals():
    """The seven calls a group refuses (GPAK_ENOTIMPL), between questions: nothing changes, nothing is factored again."""
    return ([S("n_gpus"), S("transport"), S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"), S("timing")] +
            refusals() + [S("logLikelihood"), S("timing"), S("posteriorMeanVar", X="P5")] + refusals()[:3] +
            [S("solve_alpha"), S("solve_chol", k=1), S("timing"), S("n_gpus"), S("transport")])


def alternate(a, b):
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


def seq_g_order():
    """Questions before gpak_set_train and before any parameters: GPAK_ESTATE, nothing counted, the group usable afterwards."""
    def early(ctx, factor_reads):
        c = dict(ctx=ctx)
        s = [S("logLikelihood", **c), S("nlz_terms", **c), S("solve_alpha", **c), S("factor", **c), S("GradLL", **c),
             S("GradLL_hyb", ng=10, **c), S("gram", **c), S("posteriorMeanVar", X="P5", **c), S("failed_column", **c)]
        return s + ([S("solve_chol", k=1, **c), S("chol_upper", **c)] if factor_reads else []) + [S("n_gpus", **c), S("transport", **c)]
    s = early(0, False) + [S("set_params", kern="E")] + early(0, False)
    s += [S("set_train", train="T129"), S("logLikelihood"), S("solve_alpha"), S("posteriorMeanVar", X="P5"), S("timing")]
    s += [S("set_train", ctx=1, train="T129")] + early(1, True) + [S("posteriorMeanVar", ctx=1, X="Q5"), S("timing", ctx=1)]
    s += [S("set_params", ctx=1, kern="E13"), S("logLikelihood", ctx=1), S("timing", ctx=1)]
    s += [S("set_train", train="T300"), S("set_train", train="T129"), S("logLikelihood"), S("solve_alpha"),
          S("posteriorMeanVar", X="Q5"), S("logLikelihood"), S("timing")]
    return s


def seq_g_refused_setters():
    """seq_refused_setters on a group: the group's copy of the set, its composition flag and the ranks' stored composition too."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"),
            no("set_train", ENOTIMPL, train="T129x5"), S("solve_alpha"), S("posteriorMeanVar", X="P5"), S("timing"),
            no("set_params", EINVAL, kern="E13", mode=BAD_MODE), S("logLikelihood"), S("GradLL"), S("timing"),
            no("set_kernel", EINVAL, kern="UNK"), S("logLikelihood"), S("GradLL"), S("solve_chol", k=1), S("timing"),
            S("set_kernel", kern="ER"), S("logLikelihood"), no("set_kernel", EINVAL, kern="UNK"), S("logLikelihood"), S("GradLL_hyb", ng=13),
            S("solve_alpha"), no("set_train", ENOTIMPL, train="T129x5"), S("posteriorMeanVar", X="P300"), S("timing")]


GROUP_RANDOM = ((129, 2), (300, 3))        # (N, P) of the seeded random sequences
GROUP_RANDOM_LENGTH = 24


def seq_g_random(k):
    n, _ = GROUP_RANDOM[k]
    rng = np.random.default_rng(RANDOM_SEED + 100 + k)
    pick = lambda a: a[int(rng.integers(len(a)))]   # noqa: E731
    cur = dict(kern=None)

    def set_kern():
        cur["kern"] = pick(["E", "E13", "T2", "Esn", "ER", "EXR", "EW"])
        return S("set_kernel" if cur["kern"] in ("ER", "EXR", "EW") else "set_params", kern=cur["kern"])

    steps = [S("set_train", train=f"T{n}"), set_kern()]
    while len(steps) < GROUP_RANDOM_LENGTH:
        r = rng.random()
        if r < 0.08:
            steps.append(S("set_train", train=f"T{n}"))
        elif r < 0.25:
            steps.append(set_kern())
        else:
            m = pick(["gram", "factor", "solve_alpha", "solve_chol", "logLikelihood", "nlz_terms", "posteriorMeanVar", "grad", "compute_k",
                      "chol_upper", "timing", "failed_column", "refused", "n_gpus", "transport"])
            if m == "grad":
                if cur["kern"] == "EW":
                    continue
                plain = cur["kern"] in ("E", "E13", "T2", "Esn")
                steps.append(S("GradLL") if plain else S("GradLL_hyb", ng=NG[cur["kern"]]))
            elif m == "solve_chol":
                steps.append(S("solve_chol", k=int(rng.integers(1, 4))))
            elif m == "posteriorMeanVar":
                steps.append(S("posteriorMeanVar", X=pick(["P5", "P300", "P700"]), want_var=bool(rng.integers(2))))
            elif m == "compute_k":
                steps.append(S("compute_k", X1="P300", X2="P5"))
            elif m == "refused":
                steps.append(pick(refusals()))
            else:
                steps.append(S(m))
    return steps


def _gseq(name, wgroup, steps, ranks, precision=F64):
    return dict(name=name, group=wgroup, steps=steps, ranks=ranks, precision=precision)


# `group`: the worker process the sequence runs in on the device (tests/ctx_seq_worker.py --group NAME --ranks P, P the
# largest rank count of its sequences); split so that each stays near ten seconds (DESIGN.md has the measured figures)
GROUP_SEQUENCES = [
    _gseq("group count", "g-count", seq_g_count(), 2),
    _gseq("refusals (group)", "g-count", seq_g_refusals(), 2),
    _gseq("late replicas [P=2]", "g-late2", seq_g_late(), 2),
    _gseq("late replicas [P=3]", "g-late3", seq_g_late(), 3),
    _gseq("gram between (group) [direct]", "g-gram2", seq_g_gram(DIRECT), 2),
    _gseq("gram between (group) [expansion]", "g-gram3", seq_g_gram(EXPANSION), 3),
    _gseq("compositions (group)", "g-comp", seq_g_compositions(), 2),
    _gseq("fail and recover (group)", "g-fail", seq_g_fail(), 3),
    _gseq("size walk (group) [P=2]", "g-walk2", seq_g_walk(), 2),
    _gseq("size walk (group) [P=3]", "g-walk3", seq_g_walk(), 3),
    _gseq("f32 (group)", "g-f32", seq_g_f32(), 2, F32),
    _gseq("two groups", "g-two", alternate(seq_g_late(0), seq_g_gram(DIRECT, 1)), (2, 3)),
    _gseq("a group and a single context", "g-single", alternate(seq_g_gram(DIRECT, 0), seq_gradients(1)), (2, 1)),
    _gseq("out of order (group)", "g-order", seq_g_order(), (2, 2)),
    _gseq("refused setters (group)", "g-order", seq_g_refused_setters(), 2),
] + [_gseq(f"random (group) {k}", f"g-random{k}", seq_g_random(k), GROUP_RANDOM[k][1]) for k in range(len(GROUP_RANDOM))]
GROUP_BY_NAME = {s["name"]: s for s in GROUP_SEQUENCES}
WORKER_GROUPS = {}                         # worker group -> --ranks
for _s in GROUP_SEQUENCES:
    _r = _s["ranks"]
    WORKER_GROUPS[_s["group"]] = max(WORKER_GROUPS.get(_s["group"], 0), max(_r) if isinstance(_r, tuple) else _r)

# What a group over caller-supplied engines (gpak_create_multi_with_engines: the group's real host code on the CPU) answers
# without device replicas
ENGINE_VOCABULARY = SETTERS + ("logLikelihood", "nlz_terms", "solve_alpha", "GradLL", "GradLL_hyb", "factor", "failed_column", "timing",
                               "n_gpus", "transport") + REFUSED_ON_A_GROUP


def engine_sequence(seq, ranks):
    """The steps of a group sequence that an engine group answers (GradLL_hyb: while the kernel in force is ExpAns(+Bias),
    i.e. while the call is distributed), every group with `ranks` ranks; contexts that are no groups are left out; None
    where nothing is left to ask."""
    general, steps = {}, []
    for c, method, kw in seq["steps"]:
        if ranks_of(seq, c) == 1 or method not in ENGINE_VOCABULARY or seq["precision"] != F64:
            continue
        if method in ("set_params", "set_kernel") and "refuse" not in kw:
            general[c] = method == "set_kernel"
        if method == "GradLL_hyb" and general.get(c, False):
            continue
        steps.append((c, method, kw))
    if not any(m not in SETTERS + ("timing",) for _c, m, _kw in steps):
        return None
    return dict(seq, steps=steps, ranks=ranks)


# ======== the feature calls: DESIGN.md section 8, "Call sequences across the feature calls" ====================================
# gpak_loo_grad, gpak_cv_groups(_grad), gpak_cv_folds(_grad), gpak_design, gpak_condition, gpak_sample_path and the four local
# calls share dGpart, dG / dLoo, the prediction buffers, Upred and the dCond* buffers with each other and with the calls above.
# The data the keys name, built from what each feature's own tests use:
#   labels      cvg_ref.holes / mixed_sizes (1, 2, 127, 128) / singletons, cvf_cases.random_folds(3), and "big": contiguous folds
#               with one above 128 samples (129 + 171 at T300, 256 + 257 + 187 at T700, 129 + 971 at T1100, all of T129);
#               "over": groups of 129, which gpak_cv_groups(_grad) refuses;
#   designs     the two smallest 3-column entries of design_cases.CASES (T17 nd1 "six" weighted with 3 picks, T17 nd8 "twins"
#               with 2) and, as the large footprint in dGpart, "sizes" (T130 nd8, 344 candidates in holes of 1 .. 128);
#   draws       Ysim / Fsim as test_path_gpu.draws, S = 3 and S = 130 (one past the 128-realisation tile of gpak_kmm_f64);
#   priors      nfeat = 96 and 1100 (one past FEAT_CHUNK = 1024), frequencies as test_path_gpu.features, every feature on term 0
#               (valid under every composition), S = 3;
#   local       N300-M37-nd1-defaults and N513-M130-nd8-defaults of local_cases (lists of 1 .. 128 samples: every tier edge in
#               one call); the search over the same samples and centres with k = 17 and k = 128.
# The binding numbers labels by rank, so "a label out of range" cannot reach the library through it: the label refusal the
# sequences meet is the group above 128.  gpak_predict_local(_ok) are not asked at the failing parameters (sn2 < 0 makes every
# node's own matrix borderline; whether a pivot fails there is no property of the context).
import cvf_cases  # noqa: E402
import cvg_ref  # noqa: E402

# Compositions of the prediction-buffer sequences.  gpak_condition's own bound in the EXPANSION form is wide (2e-7 max|Kbar| sum_j
# |A_js|, and alpha grows as sn2 shrinks), so E / EXR / T2 at sn2 = 0.016 .. 0.05 lie only 100 to 1000 of those bounds apart; with a
# noise of 0.2 .. 0.4 and plainly different widths and amplitudes every pair is at least 1400 bounds apart (the separation test).
E2 = [E[0], 0.5 * E[1], E[2], 0.5 * E[3], E[4], 0.5 * E[5], 1.4, E[7]]
KERN.update({"En": ([(EXPANS, E)], synth.DEFAULT_BIAS, 0.0, 0.4), "E2n": ([(EXPANS, E2)], 0.05, 0.0, 0.3),
             "T2XRn": ([(EXPANS, THETA2), (EXP, [0.5, 0.9]), (RBF, [0.5, 0.9, 0.5])], 0.35, 0.0, 0.2)})
NG.update({name: sum(cm.NPARS[k] for k, _ in KERN[name][0]) + 2 for name in ("En", "E2n", "T2XRn")})
BIG_FOLDS = {129: (129,), 300: (129, 171), 700: (256, 257, 187), 1100: (129, 971)}
LABELS = {"holes": cvg_ref.holes, "mixed": cvg_ref.mixed_sizes, "singles": cvg_ref.singletons, "folds": cvf_cases.random_folds(3),
          "big": lambda n: cvf_cases.contiguous(*BIG_FOLDS[n])(n), "over": lambda n: cvg_ref.holes(n, 129)}
SMALL_GROUPS = ("holes", "mixed", "singles")          # no group above 128: what gpak_cv_groups takes
DESIGNS = {"six": ("N200-theta2-T17-nd1-six", True, 3), "twins8": ("N200-defaults-T17-nd8-twins", False, 2),
           "sizes": ("N513-defaults-T130-nd8-sizes", False, 1)}
PRIORS = {"F96": 96, "F1100": 1100}
PRIOR_S = 3
LOCAL = {"L37x1": "N300-M37-nd1-defaults", "L130x8": "N513-M130-nd8-defaults",
         "L37x8d4": "N300-M37-nd8-d4-defaults"}      # four columns: refused (GPAK_ENOTIMPL) by a context whose training set has three
CV_SUMMARY = ("mse", "mssr", "msmd", "log_pl")
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def labels(key, n):
    a = np.asarray(LABELS[key](int(n)), dtype=np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def design_args(key, bad_columns=False):
    """(Xt, nd, Xc, hole, weights, picks); bad_columns: a fourth column on both point sets (refused on a 3-column set)"""
    import design_cases as dc
    name, weighted, k = DESIGNS[key]
    T, nd = dc.CASES[name][2], dc.CASES[name][3]
    _X, _y, Xt, Xc, hole = dc.inputs(name)
    if bad_columns:
        Xt, Xc = np.asfortranarray(np.hstack([Xt, Xt[:, :1]])), np.asfortranarray(np.hstack([Xc, Xc[:, :1]]))
    return Xt, nd, Xc, hole, (dc.weights(T) if weighted else None), k


@functools.lru_cache(maxsize=None)
def draws(n, m, s):
    rng = np.random.default_rng(17 * n + m + s)
    return np.asfortranarray(0.7 * rng.standard_normal((n, s))), np.asfortranarray(1.3 * rng.standard_normal((m, s)))


@functools.lru_cache(maxsize=None)
def prior(key, n):
    """(feat_term, omega, ab, b0, E) of a spectral prior with PRIORS[key] features and PRIOR_S realisations"""
    nfeat = PRIORS[key]
    rng = np.random.default_rng(900 + nfeat + n)
    om = rng.standard_normal((nfeat, 4)) / np.abs(rng.standard_normal((nfeat, 1)))
    om[:, 3] = 0.0
    om[5] *= 1e4 / np.abs(om[5]).max()                # one frequency of order 1e4
    return (np.zeros(nfeat, dtype=np.int32), om, np.asfortranarray(rng.standard_normal((2 * nfeat, PRIOR_S))), rng.standard_normal(PRIOR_S),
            np.asfortranarray(rng.standard_normal((n, PRIOR_S))))


@functools.lru_cache(maxsize=None)
def local_inputs(key):
    """(Xs, ys, Xd, nd, nbr, centres) of a case of local_cases"""
    import local_cases as lc
    Xs, ys, Xd, nbr = lc.inputs(LOCAL[key])
    nd = lc.CASES[LOCAL[key]][2]
    return Xs, ys, Xd, nd, nbr, np.asfortranarray(lc.centres(Xd, nd))


class _sized:
    """The binding sizes its label and realisation checks by Gpak.N; before a training set the library refuses first, so
    the data is made for `n` samples and N says so for the length of the call."""

    def __init__(self, obj, n_train, n):
        self.obj, self.on = obj, (not n_train) and hasattr(obj, "_h")
        self.n = n

    def __enter__(self):
        if self.on:
            # only ever on a binding object that holds no training set; anything else would hide a stale size
            assert self.obj.N == 0, self.obj.N       # Gpak.__init__ sets N = 0 (and no d) until gpak_set_train is accepted
            self.obj.N = self.n

    def __exit__(self, *exc):
        if self.on:
            assert self.obj.N == self.n, (self.obj.N, self.n)        # the call itself must not have moved it
            self.obj.N = 0


def _cv_out(out):
    s = out[-1]
    return int(s["status"]), tuple(out[:-1]) + (np.array([s[k] for k in CV_SUMMARY]), np.array([s["groups"], s["max_size"]], dtype=float))


def _ask_cv(method):
    def ask(obj, kw, n_train):
        n = n_train or 300
        args = [labels(kw["labels"], n)] + ([kw["ng"]] if method.endswith("_grad") else [])
        opts = dict(no_batch=kw["no_batch"]) if "no_batch" in kw else {}
        with _sized(obj, n_train, n):
            return _cv_out(getattr(obj, method)(*args, **opts))
    return ask


def _ask_loo_grad(obj, kw, n_train):
    g, s = obj.loo_grad(kw["ng"])
    return int(s["status"]), (g, np.array([s[k] for k in ("mse", "mssr", "log_pl")]))


def _ask_design(obj, kw, n_train):
    Xt, nd, Xc, hole, wt, k = design_args(kw["design"], kw.get("bad_columns", False))
    gain, picked, pick_gain, ex = obj.design(Xt, nd, Xc, hole, wt, k, True)
    s = ex["summary"]
    return int(s["status"]), (gain, picked, pick_gain, ex["reduction"], ex["var"], ex["var_after"], np.array([s["var_before"], s["var_after"]]),
                              np.array([s["holes"], s["max_size"], s["picks"]], dtype=float))


def _ask_condition(obj, kw, n_train):
    Xd, nd = blocks(kw["blocks"])
    n = n_train or 300
    Y, F = draws(n, Xd.shape[0] // nd, kw["S"])
    with _sized(obj, n_train, n):
        Z, mean, s = obj.condition(Xd, nd, Y, F if kw.get("fsim", True) else None, unfused=kw.get("unfused", False))
    return int(s["status"]), (Z, mean, np.array([s["fused"]], dtype=float))


def _ask_sample_path(obj, kw, n_train):
    Xd, nd = blocks(kw["blocks"])
    n = n_train or 300
    with _sized(obj, n_train, n):
        Z, mean, s = obj.sample_path(Xd, nd, *prior(kw["prior"], n), unfused=kw.get("unfused", False))
    return int(s["status"]), (Z, mean, np.array([s["fused"]], dtype=float))


def _local_counts(s):
    return np.array([s[k] for k in ("nodes", "empty", "notpd", "max_used")], dtype=float)


def _ask_predict_local(obj, kw, n_train):
    Xs, ys, Xd, nd, nbr, _c = local_inputs(kw["local"])
    mean, var, s = obj.predict_local(Xs, ys, Xd, nd, nbr, latent=kw.get("latent", False))
    return OK, (mean, var, _local_counts(s))


def _ask_predict_local_ok(obj, kw, n_train):
    Xs, ys, Xd, nd, nbr, _c = local_inputs(kw["local"])
    mean, var, mu, s = obj.predict_local_ok(Xs, ys, Xd, nd, nbr, want_mu=True, latent=kw.get("latent", False))
    return OK, (mean, var, mu, _local_counts(s))


def _ask_search(obj, kw, n_train):
    Xs, _ys, _Xd, _nd, _nbr, centres = local_inputs(kw["local"])
    nbr, used, d2, _s = obj.local_neighbours_dev(Xs, centres, kw["k"], want_dist2=True)
    return OK, (nbr, used, d2)


FEATURE_INVOKE = {"loo_grad": _ask_loo_grad, "cv_groups": _ask_cv("cv_groups"), "cv_groups_grad": _ask_cv("cv_groups_grad"),
                  "cv_folds": _ask_cv("cv_folds"), "cv_folds_grad": _ask_cv("cv_folds_grad"), "design": _ask_design,
                  "condition": _ask_condition, "sample_path": _ask_sample_path,
                  "local_metric": lambda obj, kw, n_train: (OK, obj.local_metric(kw.get("term", 0))),
                  "predict_local": _ask_predict_local, "predict_local_ok": _ask_predict_local_ok, "local_neighbours_dev": _ask_search}
FEATURE_ENTRY = {"cv_groups": "gpak_cv_groups", "cv_groups_grad": "gpak_cv_groups_grad", "cv_folds": "gpak_cv_folds",
                 "cv_folds_grad": "gpak_cv_folds_grad", "design": "gpak_design", "condition": "gpak_condition",
                 "sample_path": "gpak_sample_path", "local_metric": "gpak_local_metric", "predict_local": "gpak_predict_local",
                 "predict_local_ok": "gpak_predict_local_ok", "local_neighbours_dev": "gpak_local_neighbours_dev"}
ENTRY.update(FEATURE_ENTRY)
FEATURE_HEADERS = ("gpak_cv_groups.h", "gpak_cv_groups_grad.h", "gpak_cv_folds.h", "gpak_cv_folds_grad.h", "gpak_design.h", "gpak_condition.h",
                   "gpak_local.h", "gpak_local_ok.h", "gpak_local_search.h", "gpak_loo_grad.h")


def _equal(label, a, b):
    return (label, 0.0 if np.array_equal(a, b) else float("inf"), 1.0)


def _gradient_errors(g, w, half, b):
    """test_group_gradient_matches_numpy_restatement / test_fold_gradient_matches_numpy_restatement / test_loo_gradient_...: per
    block; the bias entry (1/2 sum W) also on the condition of its own sum"""
    nk = len(w) - 2
    return [("kernel block", float(np.abs(g[:nk] - w[:nk]).max() / np.abs(w[:nk]).max()), b),
            ("bias", abs(g[nk] - w[nk]), b * abs(w[nk]) + 1e-15 * half), ("sn2", abs(g[nk + 1] - w[nk + 1]) / abs(w[nk + 1]), b)]


def feature_errors(method, kw, g, w, m, t8, direct):
    """model_errors for the feature calls.  b: 1e-8, the bound of every one of their GPU tests in the DIRECT form
    (cvf_cases.BOUND, test_cv_groups_gpu.BOUND, test_design_gpu.BOUND, test_path_gpu.BOUND, test_block_gpu.BOUND for the local
    calls).  In the EXPANSION form: gpak_design and gpak_condition have tests of their own there
    (test_design_in_the_expansion_form: the same bound; test_condition_in_the_expansion_form: the fill tolerance through
    sum_j |A_js|), the local calls use the direct distance whatever the form (test_predict_local_matches_...: the same bytes),
    and the cross-validation calls and gpak_loo_grad, whose tests run the DIRECT form only, BORROW the prediction's 1e-5 as loo
    and the block calls do above."""
    import path_ref
    b = 1e-8 if direct else t8
    if method == "local_neighbours_dev":              # test_local_search_gpu: bytes
        return [_equal("lists", g[0], w[0]), _equal("used", g[1], w[1]), _equal("dist2", g[2], w[2])]
    if method == "local_metric":
        # test_local_metric_is_the_distance_of_the_term: exp(-sqrt(D2)) var2 + bias within 1e-12 of its largest value, D2 from G.
        # Here with var2 = 1 and bias = 0 (they scale and shift both sides alike) on the first 64 points of P300.
        P = points("P300")[:64]

        def kernel(G):
            T = P @ G[:3, :3]
            return np.exp(-np.sqrt(((T[:, None, :] - T[None, :, :]) ** 2).sum(axis=2)))
        return [("exp(-|(x - x') G|)", float(np.abs(kernel(g[0]) - kernel(w[0])).max()), 1e-12)]
    pv = m.prior_variance()
    if method in ("predict_local", "predict_local_ok"):       # test_predict_local(_ok)_matches_the_long_double_reference
        ys = local_inputs(kw["local"])[1]
        smax = float(np.abs(ys).max())
        out = [("mean", float(np.abs(g[0] - w[0]).max() / smax), 1e-8), ("var", float(np.abs(g[1] - w[1]).max() / pv), 1e-8)]
        if method == "predict_local_ok":
            out.append(("mu", float(np.abs(g[2] - w[2]).max() / smax), 1e-8))
        return out + [_equal("counts", g[-1], w[-1])]
    ymax = float(np.abs(m.y).max())
    if method in ("cv_groups", "cv_folds"):           # test_cv_groups_matches_numpy_restatement, test_cv_folds_matches_numpy_restatement
        return [("mean", float(np.abs(g[0] - w[0]).max() / ymax), b), ("var", float((np.abs(g[1] - w[1]) / np.abs(w[1])).max()), b),
                ("logp", float((np.abs(g[2] - w[2]) / np.abs(w[2])).max()), b),
                ("summary", float((np.abs(g[3] - w[3]) / np.abs(w[3])).max()), b), _equal("counts", g[4], w[4])]
    if method == "loo_grad":                          # test_loo_gradient_matches_numpy_restatement; the summary: test_loo_matches_...
        return _gradient_errors(g[0], w[0], m._loo_grad()[1], b) + [("summary", float((np.abs(g[1] - w[1]) / np.abs(w[1])).max()), b)]
    if method in ("cv_groups_grad", "cv_folds_grad"):
        group = np.unique(labels(kw["labels"], m.N), return_inverse=True)[1].reshape(-1)
        return _gradient_errors(g[0], w[0], m._cv_grad_ref(group)[1], b) + \
            [("summary", float((np.abs(g[1] - w[1]) / np.abs(w[1])).max()), b), _equal("counts", g[2], w[2])]
    if method == "design":                            # test_design_matches_long_double, test_design_in_the_expansion_form
        Xt, nd, _Xc, _hole, wt, k = design_args(kw["design"])
        sw = float(Xt.shape[0] // nd if wt is None else wt.sum())
        out = [("gain", float(np.abs(g[0] - w[0]).max()), 1e-8 * pv * sw), _equal("picked", g[1], w[1]),
               ("reduction", float(np.abs(g[3] - w[3]).max()), 1e-8 * pv), ("var", float(np.abs(g[4] - w[4]).max()), 1e-8 * pv),
               ("var_after", float(np.abs(g[5] - w[5]).max()), 1e-8 * pv), ("sums", float(np.abs(g[6] - w[6]).max()), 1e-8 * pv * sw),
               _equal("counts", g[7], w[7])]
        return out + ([("pick_gain", float(np.abs(g[2] - w[2]).max()), 1e-8 * pv * sw)] if k else [])
    # gpak_condition / gpak_sample_path: test_condition_against_long_double, test_sample_path_is_the_reference_linear_map: 1e-8 of
    # max|y| + max|Ysim| + max|Fsim| (an absent Fsim adds nothing), the sampler also the rounding of theta,
    # 8 u sum_f |amp_f| (1 + sum_k |omega_fk u_k|).  EXPANSION (test_condition_in_the_expansion_form): per element also
    # 2e-7 max|Kbar| sum_j |A_js|, A = alpha 1' - Ky^-1 Ysim; the mean is the column A = alpha.  gpak_sample_path has no test in
    # that form and borrows gpak_condition's.
    Xd, nd = blocks(kw["blocks"])
    pm = m.path_model(Xd, nd)
    theta = 0.0
    if method == "condition":
        Y, F = draws(m.N, Xd.shape[0] // nd, kw["S"])
        F = F if kw.get("fsim", True) else None
    else:
        ft, om, ab, b0, E = prior(kw["prior"], m.N)
        F, Y = pm.prior_draw(ft, om, ab, b0, E)
        _, amp, arg = pm.features(pm.Xd, nd, ft, om)
        _, _, argx = pm.features(pm.X, 1, ft, om)
        theta = 8 * U * float((amp.astype(float) * (1 + np.maximum(arg, argx))).sum())
    scale = ymax + float(np.abs(Y).max()) + (float(np.abs(F).max()) if F is not None else 0.0)
    bz = bm = 1e-8 * scale + theta
    if not direct:
        A = pm.alpha[:, None] - path_ref.solve_ky(pm.L, np.asarray(Y, dtype=LD))
        kmax = float(np.abs(pm.Kbar).max())
        bz = bz + 2e-7 * kmax * np.abs(A).sum(axis=0).astype(float)[None, :]
        bm = bm + 2e-7 * kmax * float(np.abs(pm.alpha).sum())
    return [("Z", float((np.abs(g[0] - w[0]) / bz).max()), 1.0), ("mean", float(np.abs(g[1] - w[1]).max() / bm), 1.0), _equal("fused", g[2], w[2])]


# ---- the named feature sequences ---------------------------------------------------------------------------------------------
def cv_all(small, any_size, ng=10, ctx=0):
    c = dict(ctx=ctx)
    return [S("cv_groups", labels=small, **c), S("cv_groups_grad", labels=small, ng=ng, **c), S("cv_folds", labels=any_size, **c),
            S("cv_folds_grad", labels=any_size, ng=ng, **c)]


def seq_cv_workspace():
    """G = L^-T of the four cross-validation calls goes into dG when a gradient has allocated one, else into dLoo
    (csrc/cv_folds.hip, csrc/cv_groups.hip): each call before any gradient, then GradLL_exact and loo_grad (dG / dBinv exist from
    here on), then each again with loo, GradLL and GradLL_hyb between; then T1100 (leading-dimension pad 32) -> T300 -> T700 with
    one question of each after every change: every shared buffer holds the larger set's numbers at another leading dimension."""
    s = [S("set_train", train="T300"), S("set_params", kern="E")] + cv_all("mixed", "big")
    s += [S("GradLL_exact", ng=10), S("loo_grad", ng=10)]
    s += [S("cv_groups", labels="mixed"), S("loo"), S("cv_groups_grad", labels="holes", ng=10), S("GradLL"),
          S("cv_folds", labels="big", no_batch=True), S("GradLL_hyb", ng=10), S("cv_folds_grad", labels="folds", ng=10),
          S("cv_folds_grad", labels="big", ng=10, no_batch=True)]
    s += [S("timing"), S("set_train", train="T1100")] + cv_all("holes", "big")
    s += [S("timing"), S("set_train", train="T300")] + cv_all("holes", "big")
    s += [S("timing"), S("set_train", train="T700")] + cv_all("mixed", "big")
    return s + [S("timing")]


def seq_scratch():
    """dGpart: gpak_design carves four arrays out of it (csrc/design.hip), gpak_cv_groups five, gpak_cv_folds three, the
    gradients their partial sums.  The footprint grows and shrinks from call to call: the large design, then singletons, then
    the reverse, with the gradients between."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("design", design="sizes"), S("cv_groups", labels="singles"),
            S("cv_folds_grad", labels="big", ng=10), S("GradLL_exact", ng=10), S("loo_grad", ng=10), S("design", design="six"),
            S("cv_groups", labels="mixed"), S("timing"), S("set_params", kern="E13"), S("cv_groups", labels="singles"), S("design", design="sizes"),
            S("cv_folds_grad", labels="folds", ng=10), S("loo_grad", ng=10), S("GradLL_exact", ng=10), S("design", design="twins8"),
            S("cv_groups_grad", labels="singles", ng=10), S("timing")]


def seq_feature_prediction(mode):
    """dWt / dC / dTblk / dXblk / Upred serve the point, block and joint predictions, gpak_design and gpak_condition; dTblk is
    sized by the number of terms, gpak_design and gpak_condition transform the training points again into Upred under a mean
    pooled with their own points.  n_d = 1 and 8; M small, 300 in two batches, small; one term, three, one.  In the EXPANSION
    form every call that pools a mean is followed by logLikelihood and gram, which read the training points' own transform."""
    def pooled(step):
        return [step] + ([S("logLikelihood"), S("gram")] if mode == EXPANSION else [])
    s = [S("set_train", train="T300"), S("set_params", kern="En", mode=mode)]
    s += pooled(S("posteriorMeanVar", X="P5")) + [S("predict_block", blocks="B12x8")] + pooled(S("design", design="twins8"))
    s += pooled(S("condition", blocks="B40x1", S=3)) + [S("predict_joint", blocks="B40x1"), S("sample_joint", blocks="B12x8")]
    s += [opt("PRED_BATCH", 256)] + pooled(S("condition", blocks="B300x1", S=3)) + [S("predict_joint", blocks="B300x1")]
    s += pooled(S("posteriorMeanVar", X="P300")) + pooled(S("design", design="six")) + [opt("PRED_BATCH", 0)]
    s += pooled(S("condition", blocks="B12x8", S=3))
    s += [S("timing"), S("set_kernel", kern="T2XRn", mode=mode), S("predict_block", blocks="B12x8")] + pooled(S("condition", blocks="B40x8", S=3))
    s += pooled(S("design", design="six")) + [S("predict_joint", blocks="B40x1"), S("sample_joint", blocks="B40x1")]
    s += pooled(S("condition", blocks="B300x1", S=3))
    s += [S("set_params", kern="E2n", mode=mode)] + pooled(S("condition", blocks="B12x8", S=3)) + [S("predict_block", blocks="B40x8")]
    s += pooled(S("design", design="twins8")) + pooled(S("posteriorMeanVar", X="P5"))
    return s + [S("timing")]


def seq_simulation():
    """The dCond* buffers grow only: S = 130 (one past the 128-realisation tile) then S = 3, fused then unfused, 1100 features
    (one past FEAT_CHUNK) then 96; then T300 -> T129 -> T300: dCondY and dCondA take N rows per column of an N_p pitch, the rows
    N .. N_p keep the larger set's numbers.  gpak_condition solves through dWork: solve_chol, set_params and solve_alpha after each
    part.  No step follows a change of INV512 / BWD_FUSED."""
    after = lambda kern: [S("solve_chol", k=2), S("timing"), S("set_params", kern=kern), S("solve_alpha")]        # noqa: E731
    s = [S("set_train", train="T300"), S("set_params", kern="E"), S("condition", blocks="B40x8", S=130), S("condition", blocks="B40x8", S=3),
         S("condition", blocks="B40x8", S=3, unfused=True), S("condition", blocks="B40x8", S=130, fsim=False)] + after("E13")
    s += [S("sample_path", blocks="B40x1", prior="F1100"), S("sample_path", blocks="B40x1", prior="F96"),
          S("sample_path", blocks="B40x1", prior="F96", unfused=True)] + after("E")
    s += [S("set_train", train="T129"), S("condition", blocks="B40x8", S=130), S("sample_path", blocks="B40x1", prior="F96")] + after("E13")
    s += [S("set_train", train="T300"), S("condition", blocks="B40x8", S=3), S("condition", blocks="B40x8", S=130, unfused=True),
          S("sample_path", blocks="B12x8", prior="F96"), S("solve_alpha"), S("logLikelihood"), S("timing")]
    return s


def factor_calls(ctx=0):
    """every feature call that needs the factor, once"""
    c = dict(ctx=ctx)
    return cv_all("holes", "big", 10, ctx) + [S("loo_grad", ng=10, **c), S("design", design="six", **c), S("condition", blocks="B12x8", S=3, **c),
                                              S("sample_path", blocks="B12x8", prior="F96", **c)]


def factorless_calls(ctx=0):
    """the local calls that read neither the factor nor sn2"""
    c = dict(ctx=ctx)
    return [S("local_metric", **c), S("local_neighbours_dev", local="L37x1", k=17, **c)]


def local_calls(a="L37x1", b="L37x1", k=17, ctx=0):
    c = dict(ctx=ctx)
    return [S("local_metric", **c), S("predict_local", local=a, **c), S("predict_local_ok", local=b, **c),
            S("local_neighbours_dev", local=a, k=k, **c)]


def seq_feature_fail():
    """sn2 < 0 (from column 1, then from column 200): every feature call that needs the factor answers GPAK_ENOTPD with quiet
    NaN, the local calls that need none answer as before, and after good parameters everything has a fresh context's bits."""
    return ([S("set_train", train="T300"), S("set_params", kern="E"), S("cv_groups", labels="holes"), S("set_params", kern="BAD")] +
            factor_calls() + factorless_calls() + [S("failed_column"), S("timing"), S("set_params", kern="BAD200")] + factor_calls() +
            [S("failed_column"), S("timing"), S("set_params", kern="E13")] + factor_calls() + local_calls() + [S("failed_column"), S("timing")])


def seq_feature_f32():
    """GPAK_F32: the feature calls are fp64 whatever the context's precision; between fp32 predictions they must leave the fp32
    image of the factor alone and find the fp64 factor."""
    return [S("set_train", train="T300"), S("set_params", kern="E"), S("posteriorMeanVar", X="P300"), S("cv_groups", labels="holes"),
            S("posteriorMeanVar", X="P5"), S("design", design="six"), S("condition", blocks="B12x8", S=3), S("posteriorMeanVar", X="P300"),
            S("cv_folds_grad", labels="big", ng=10), S("loo_grad", ng=10), S("predict_local", local="L37x1"), S("posteriorMeanVar", X="P300"),
            S("set_params", kern="T2"), S("posteriorMeanVar", X="P300"), S("sample_path", blocks="B40x1", prior="F96"),
            S("cv_folds", labels="big"), S("cv_groups_grad", labels="mixed", ng=10), S("predict_local_ok", local="L37x1"),
            S("posteriorMeanVar", X="P5"), S("timing")]


def seq_feature_refused():
    """Each call's cheapest refusals (a group above 128, a gradient of the wrong length, a fourth column -- for the local
    predictions too: GPAK_ENOTIMPL --, k = 129 for the search, a White child for the gradients, no parameters, no training set) are
    results, and the answers after them are those of a context that never saw
    the call: nothing is factored for them (timing)."""
    early = cv_all("holes", "big", 10, 1) + [S("loo_grad", ctx=1, ng=10), S("design", ctx=1, design="six"),
                                             S("condition", ctx=1, blocks="B12x8", S=3), S("sample_path", ctx=1, blocks="B12x8", prior="F96")]
    return ([S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"), S("timing"),
             S("cv_groups", labels="over"), S("cv_groups_grad", labels="over", ng=10), S("logLikelihood"),
             S("cv_groups_grad", labels="holes", ng=11), S("cv_folds_grad", labels="big", ng=9), S("loo_grad", ng=13),
             S("design", design="six", bad_columns=True), S("condition", blocks="C12x8", S=3), S("sample_path", blocks="C12x8", prior="F96"),
             S("predict_local", local="L37x8d4"), S("predict_local_ok", local="L37x8d4"), S("local_neighbours_dev", local="L37x1", k=129),
             S("predict_local", local="L37x1"), S("solve_alpha"), S("GradLL"), S("timing"),
             S("set_kernel", kern="EW"), S("cv_groups_grad", labels="holes", ng=10), S("cv_folds_grad", labels="big", ng=10),
             S("loo_grad", ng=10), S("timing"), S("cv_groups", labels="holes"), S("logLikelihood"), S("timing")] +
            early + local_calls(ctx=1)[:3] + [S("local_neighbours_dev", ctx=1, local="L37x1", k=129),
                                              S("local_neighbours_dev", ctx=1, local="L37x1", k=17), S("set_params", ctx=1, kern="E")] + early +
            local_calls(ctx=1) +
            [S("set_train", ctx=1, train="T129"), S("cv_groups", ctx=1, labels="holes"), S("logLikelihood", ctx=1), S("timing", ctx=1)])


def seq_local_between():
    """The local calls need parameters only: before a training set, with one, between two gpak_condition calls (which share the
    block staging buffers), and after gpak_set_kernel to another composition."""
    cond = S("condition", blocks="B12x8", S=3)
    return ([S("set_params", kern="E")] + local_calls() + [S("set_train", train="T300")] + local_calls("L130x8", "L130x8", 128) +
            [cond, S("predict_local", local="L37x1"), S("predict_local_ok", local="L130x8", latent=True), cond, S("logLikelihood"),
             S("timing"), S("set_kernel", kern="EXR"), S("local_metric", term=2)] + local_calls("L37x1", "L130x8", 128) +
            [cond, S("solve_alpha"), S("timing")])


def seq_feature_two():
    """Two live contexts with different training sets and compositions, advanced alternately."""
    a = [S("set_train", train="T300"), S("set_params", kern="E"), S("cv_folds", labels="big"), S("design", design="six"),
         S("condition", blocks="B12x8", S=3), S("cv_groups_grad", labels="holes", ng=10), S("sample_path", blocks="B40x1", prior="F96"),
         S("predict_local", local="L37x1"), S("loo_grad", ng=10), S("timing")]
    b = [S("set_train", ctx=1, train="T129"), S("set_kernel", ctx=1, kern="EXR"), S("condition", ctx=1, blocks="B40x1", S=130),
         S("cv_groups", ctx=1, labels="mixed"), S("cv_folds_grad", ctx=1, labels="folds", ng=15), S("design", ctx=1, design="twins8"),
         S("loo_grad", ctx=1, ng=15), S("cv_folds", ctx=1, labels="holes"), S("predict_local_ok", ctx=1, local="L37x1"), S("timing", ctx=1)]
    return alternate(a, b)


FEATURE_RANDOM_COUNT, FEATURE_RANDOM_LENGTH = 3, 30


def seq_feature_random(k):
    """30 steps over the whole vocabulary, old and new, at N in {129, 300}; the generator keeps the preconditions: the gradient's
    length, no gradient with a White child, labels of the current N (no group above 128 for gpak_cv_groups), matching columns."""
    rng = np.random.default_rng(RANDOM_SEED + 200 + k)
    pick = lambda a: a[int(rng.integers(len(a)))]   # noqa: E731
    cur = dict(kern=None)

    def set_kern():
        cur["kern"] = pick(["E", "E13", "T2", "ER", "EXR", "EW"])
        return S("set_kernel" if cur["kern"] in ("ER", "EXR", "EW") else "set_params", kern=cur["kern"])

    steps = [S("set_train", train=pick(["T129", "T300"])), set_kern()]
    old = ["gram", "solve_alpha", "solve_chol", "logLikelihood", "nlz_terms", "posteriorMeanVar", "GradLL_exact", "loo", "predict_block",
           "predict_joint", "sample_joint", "chol_upper", "timing"]
    new = ["cv_groups", "cv_groups_grad", "cv_folds", "cv_folds_grad", "loo_grad", "design", "condition", "sample_path", "local_metric",
           "predict_local", "predict_local_ok", "local_neighbours_dev"]
    while len(steps) < FEATURE_RANDOM_LENGTH:
        r = rng.random()
        if r < 0.07:
            steps.append(S("set_train", train=pick(["T129", "T300"])))
        elif r < 0.2:
            steps.append(set_kern())
        elif r < 0.25:
            steps.append(opt(*pick([("PRED_BATCH", 256), ("PRED_BATCH", 0), ("LOO_ROWS", 128), ("LOO_ROWS", 0)])))
        else:
            m = pick(new) if r < 0.8 else pick(old)
            ng = NG[cur["kern"]]
            if m in ("GradLL_exact", "loo_grad", "cv_groups_grad", "cv_folds_grad") and cur["kern"] == "EW":
                continue
            if m in ("cv_groups", "cv_groups_grad"):
                steps.append(S(m, labels=pick(list(SMALL_GROUPS)), **(dict(ng=ng) if m.endswith("_grad") else {})))
            elif m in ("cv_folds", "cv_folds_grad"):
                steps.append(S(m, labels=pick(["big", "folds", "mixed"]), no_batch=bool(rng.integers(2)), **(dict(ng=ng) if m.endswith("_grad") else {})))
            elif m in ("GradLL_exact", "loo_grad"):
                steps.append(S(m, ng=ng))
            elif m == "design":
                steps.append(S(m, design=pick(["six", "twins8"])))
            elif m == "condition":
                steps.append(S(m, blocks=pick(["B12x8", "B40x1"]), S=pick([3, 130]), fsim=bool(rng.integers(2)), unfused=bool(rng.integers(2))))
            elif m == "sample_path":
                steps.append(S(m, blocks=pick(["B12x8", "B40x1"]), prior="F96"))
            elif m in ("predict_local", "predict_local_ok"):
                steps.append(S(m, local="L37x1", latent=bool(rng.integers(2))))
            elif m == "local_neighbours_dev":
                steps.append(S(m, local="L37x1", k=pick([17, 128])))
            elif m == "solve_chol":
                steps.append(S(m, k=int(rng.integers(1, 4))))
            elif m == "posteriorMeanVar":
                steps.append(S(m, X=pick(["P5", "P300"])))
            elif m in ("predict_block", "predict_joint", "sample_joint"):
                steps.append(S(m, blocks=pick(["B12x8", "B40x1"])))
            else:
                steps.append(S(m))
    return steps


# `group`: one worker process each (tests/ctx_seq_worker.py --group NAME: the worker finds the list by the group's name)
FEATURE_SEQUENCES = [
    _seq("cv workspace", "f-cv", seq_cv_workspace()),
    _seq("scratch", "f-scratch", seq_scratch()),
    _seq("feature prediction buffers [direct]", "f-pred-direct", seq_feature_prediction(DIRECT)),
    _seq("feature prediction buffers [expansion]", "f-pred-expansion", seq_feature_prediction(EXPANSION)),
    _seq("simulation", "f-sim", seq_simulation()),
    _seq("feature fail and recover", "f-fail", seq_feature_fail()),
    _seq("feature f32", "f-f32", seq_feature_f32(), F32),
    _seq("feature refused", "f-refused", seq_feature_refused()),
    _seq("local between", "f-local", seq_local_between()),
    _seq("feature two contexts", "f-two", seq_feature_two()),
] + [_seq(f"feature random {k}", f"f-random{k}", seq_feature_random(k)) for k in range(FEATURE_RANDOM_COUNT)]
FEATURE_GROUPS = []
for _s in FEATURE_SEQUENCES:
    if _s["group"] not in FEATURE_GROUPS:
        FEATURE_GROUPS.append(_s["group"])
FEATURE_BY_NAME = {s["name"]: s for s in FEATURE_SEQUENCES}


# ---- the feature calls on a group: every one of them is built for the single-GPU context (all ten headers: GPAK_ENOTIMPL) ------
def feature_refusals(ctx=0):
    c = dict(ctx=ctx)
    return [S("cv_groups", labels="holes", **c), S("cv_groups_grad", labels="holes", ng=10, **c), S("cv_folds", labels="big", **c),
            S("cv_folds_grad", labels="big", ng=10, **c), S("design", design="six", **c), S("condition", blocks="B12x8", S=3, **c),
            S("sample_path", blocks="B12x8", prior="F96", **c), S("local_metric", **c), S("predict_local", local="L37x1", **c),
            S("predict_local_ok", local="L37x1", **c), S("local_neighbours_dev", local="L37x1", k=17, **c)]


def seq_g_feature_refusals():
    """Between logLikelihood, solve_alpha and a sharded prediction (P300 at P = 2: 256 + 44) each feature call is asked of a group
    and refused; nothing changes and nothing is factored again."""
    r = feature_refusals()
    return ([S("set_train", train="T300"), S("set_params", kern="E"), S("logLikelihood"), S("timing")] + r[:4] +
            [S("logLikelihood"), S("solve_alpha")] + r[4:7] + [S("posteriorMeanVar", X="P300"), S("timing")] + r[7:] +
            [S("solve_alpha"), S("posteriorMeanVar", X="P300"), S("logLikelihood"), S("timing")])


GROUP_SEQUENCES.append(_gseq("g feature refusals", "g-feature", seq_g_feature_refusals(), 2))
GROUP_BY_NAME["g feature refusals"] = GROUP_SEQUENCES[-1]
WORKER_GROUPS["g-feature"] = 2
