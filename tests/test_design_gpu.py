"""GPU tests (-m gpu) of infill drilling design: gpak_design, gpak_dev_design_score alone and `gp_ss_ak design`.

Cases, data and the reference are those of tests/design_cases.py: the long-double route of tests/design_ref.py, which
tests/test_design.py pins against refits and whose every pick it shows to be decided by at least 1e-6 of the gain.
Bounds: gain, reduction, var, var_after and pick_gain within the project's GPU bound, 1e-8 of the prior variance (BOUND of
tests/test_joint_gpu.py), times sum(wt) for the weighted sums; picked equal.  The refit through the
library alone is held to twice that (two quantities, each held to 1e-8).  The score kernel alone has a derived bound of
its own (tests/design_worker.py).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import gpak, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_cases as dc  # noqa: E402
import design_worker  # noqa: E402
import test_block_gpu as tb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")
pytestmark = pytest.mark.gpu

BOUND = 1e-8
BIG = "N513-defaults-T130-nd8-sizes"
SMALL = "N200-theta2-T17-nd1-six"
WHITE = "N200-white-T257-nd8-six"


def design(g, name, weighted=False, k=None, mode=gpak.DIST_DIRECT, want_reduction=True, hole=None):
    N, comp, T, nd, layout, kk = dc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, labels = dc.inputs(name)
    g.set_train(X, y)
    tb.set_composition(g, terms, bias, sn2, white, mode)
    try:
        return g.design(Xt, nd, Xc, labels if hole is None else hole, dc.weights(T) if weighted else None,
                        kk if k is None else k, want_reduction)
    finally:
        tb.set_defaults(g)


def errors(name, weighted, got):
    """each output's largest error over its bound, against the long-double restatement"""
    N, comp, T, nd, layout, k = dc.CASES[name]
    gain, picked, pick_gain, ex = got
    ref = dc.reference(name, weighted)
    pv = tb.prior_variance(comp)
    sw = float(dc.weights(T).sum()) if weighted else float(T)
    f = lambda a: np.asarray(a).astype(float)   # noqa: E731
    out = {"gain": np.abs(gain - f(ref["gain"])).max() / (BOUND * pv * sw),
           "reduction": np.abs(ex["reduction"] - f(ref["reduction"])).max() / (BOUND * pv),
           "var": np.abs(ex["var"] - f(ref["var"])).max() / (BOUND * pv),
           "var_after": np.abs(ex["var_after"] - f(ref["var_after"])).max() / (BOUND * pv),
           "var_before_sum": abs(ex["summary"]["var_before"] - float(ref["var_before"])) / (BOUND * pv * sw),
           "var_after_sum": abs(ex["summary"]["var_after"] - float(ref["var_after_sum"])) / (BOUND * pv * sw)}
    if k:
        out["pick_gain"] = np.abs(pick_gain - f(ref["pick_gain"])).max() / (BOUND * pv * sw)
    return out, ref


# ---- 1. the library against the long-double restatement ---------------------------------------------------------------
AGAINST = [(name, w) for name in dc.CASES for w in (False, True)]


@pytest.mark.parametrize("name,weighted", AGAINST, ids=[f"{n}-{'weighted' if w else 'ones'}" for n, w in AGAINST])
def test_design_matches_long_double(gp, name, weighted):
    N, comp, T, nd, layout, k = dc.CASES[name]
    got = design(gp, name, weighted)
    errs, ref = errors(name, weighted, got)
    s = got[3]["summary"]
    print(f"\n{name} weighted={weighted}: worst value over its bound " + ", ".join(f"{key} {v:.3g}" for key, v in errs.items()) +
          f"; picks {list(got[1])}; {s['ms']:.2f} ms")
    assert s["status"] == gpak.OK and s["holes"] == int(dc.inputs(name)[4].max()) + 1 and s["picks"] == k
    assert s["max_size"] == int(np.bincount(dc.inputs(name)[4]).max())
    assert list(got[1]) == ref["picked"]
    assert max(errs.values()) <= 1.0


def test_design_in_the_expansion_form(gp):
    """GPAK_DIST_EXPANSION (the pooled mean over the training set, the targets' points and the candidates): the same
    reference, the same bound."""
    for name in (SMALL, "N200-d4-T1-nd8-six"):
        got = design(gp, name, True, mode=gpak.DIST_EXPANSION)
        errs, ref = errors(name, True, got)
        print(f"\n{name} expansion form: worst value over its bound " + ", ".join(f"{key} {v:.3g}" for key, v in errs.items()))
        assert list(got[1]) == ref["picked"] and max(errs.values()) <= 1.0


# ---- 2. one refit through the library alone ---------------------------------------------------------------------------
def test_var_after_is_the_refit_variance(gp):
    name = SMALL
    N, comp, T, nd, layout, k = dc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = dc.inputs(name)
    gain, picked, pick_gain, ex = design(gp, name)
    assert len(picked) == k == 3 and np.all(ex["var_after"] > 0.0)       # the block path clamps at 0: nothing to clamp here
    extra = Xc[np.isin(hole, picked)]
    gp.set_train(np.vstack([X, extra]), np.concatenate([y, np.zeros(len(extra))]))
    tb.set_composition(gp, terms, bias, sn2, white)
    try:
        _, lat = gp.predict_block(Xt, nd, latent=True)
    finally:
        tb.set_defaults(gp)
    err = np.abs(lat - ex["var_after"]).max() / tb.prior_variance(comp)
    print(f"\n{name}: var_after against predict_block on training + picked holes: {err / (2 * BOUND):.3g} of its bound")
    assert err <= 2 * BOUND
    assert np.all(ex["var_after"] < ex["var"])


# ---- 3. the score kernel alone ----------------------------------------------------------------------------------------
_SCORE = {}


def score_records():
    if not _SCORE:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "design_worker.py")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        _SCORE["rc"], _SCORE["err"] = r.returncode, r.stderr.decode()[-2000:]
        for line in r.stdout.decode().splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                _SCORE[rec["name"]] = rec
    return _SCORE


@pytest.mark.parametrize("shape", design_worker.SHAPES, ids=[s[0] for s in design_worker.SHAPES])
def test_score_kernel_alone(shape):
    """gpak_dev_design_score on caller-owned buffers (tests/design_worker.py, where the bound is derived): every column norm
    and every gain within its backward-error bound of the long-double values; the read-only operands, the outputs of holes
    that are not live, the guard bands and the skew rows bit-identical; the same bytes from a second call; the refusals;
    a zero weight ignored exactly.  And the check bites."""
    recs = score_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs[shape[0]]
    print(f"\n{rec}")
    assert rec["T"] == shape[1] and rec["kappa"] <= design_worker.KAPPA
    assert rec["ratio_reduction"] <= 1.0 and rec["ratio_gain"] <= 1.0
    for key in ("rc", "others_untouched", "guards", "P_untouched", "lists_untouched", "info", "repeatable"):
        assert rec[key] is True, (key, rec)
    assert rec["bites"] > 1e6
    if shape[2] and shape[1] > 2:
        assert rec["zero_weight_exact"] is True


def test_score_kernel_reports_a_failing_hole():
    recs = score_records()
    assert recs["rc"] == 0, recs["err"]
    rec = recs["failing"]
    print(f"\n{rec}")
    assert rec["rc"] and rec["info"] == 2 and rec["nan"] and rec["hole0_finite"]


# ---- 4. invariants ----------------------------------------------------------------------------------------------------
def same(a, b):
    """the same bytes"""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_invariants_of_the_call(gp):
    name = SMALL
    N, comp, T, nd, layout, k = dc.CASES[name]
    X, y, Xt, Xc, hole = dc.inputs(name)
    H = int(hole.max()) + 1
    g0, p0, pg0, e0 = design(gp, name, True, k=0)
    g3, p3, pg3, e3 = design(gp, name, True)
    g3b, p3b, pg3b, e3b = design(gp, name, True)
    assert p0.size == 0 and pg0.size == 0 and e0["summary"]["picks"] == 0
    assert same(e0["var"], e0["var_after"]) and e0["summary"]["var_before"] == e0["summary"]["var_after"]
    # the first round does not depend on the plan; two calls return the same bytes
    assert same(g0, g3) and same(e0["reduction"], e3["reduction"]) and same(e0["var"], e3["var"])
    for a, b in ((g3, g3b), (pg3, pg3b), (e3["reduction"], e3b["reduction"]), (e3["var"], e3b["var"]),
                 (e3["var_after"], e3b["var_after"])):
        assert same(a, b)
    assert list(p3) == list(p3b)
    # reduction is optional and changes nothing else
    g3n, p3n, pg3n, e3n = design(gp, name, True, want_reduction=False)
    assert e3n["reduction"] is None and same(g3, g3n) and same(pg3, pg3n) and same(e3["var_after"], e3n["var_after"])
    # another numbering of the same holes permutes the outputs
    perm = np.array([3, 0, 5, 1, 4, 2], dtype=np.int32)         # old label -> new label
    gq, pq, pgq, eq = design(gp, name, True, hole=perm[hole])
    assert same(gq[perm], g3) and same(eq["reduction"][:, perm], e3["reduction"]) and list(pq) == list(perm[p3])
    assert same(pgq, pg3) and same(eq["var_after"], e3["var_after"])
    # gain is the chain over b ascending of wt_b * reduction[b, h]: a zero weight is ignored exactly
    w = dc.weights(T)
    assert np.count_nonzero(w == 0.0) >= 3
    chain = np.zeros(H)
    for b in range(T):
        if w[b] != 0.0:
            chain = chain + w[b] * e3["reduction"][b, :]
    assert same(chain, g3)
    # wt = NULL is all ones, bit for bit
    g1, p1, pg1, e1 = design(gp, name, False)
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    gp.set_train(X, y)
    tb.set_composition(gp, terms, bias, sn2, white)
    try:
        g1w, p1w, pg1w, e1w = gp.design(Xt, nd, Xc, hole, np.ones(T), k, True)
    finally:
        tb.set_defaults(gp)
    assert same(g1, g1w) and same(pg1, pg1w) and list(p1) == list(p1w) and same(e1["var_after"], e1w["var_after"])
    assert e1["summary"]["var_before"] == e1w["summary"]["var_before"]


def test_f32_context_returns_the_same_bytes(gp):
    name = WHITE
    a = design(gp, name, True)
    g32 = gpak.Gpak(0, precision=gpak.F32)
    try:
        b = design(g32, name, True)
    finally:
        g32.close()
    assert same(a[0], b[0]) and list(a[1]) == list(b[1]) and same(a[2], b[2])
    for key in ("reduction", "var", "var_after"):
        assert same(a[3][key], b[3][key])


def test_the_call_only_reads_the_context(gp):
    """factor, alpha and nlZ stand after the call: nlZ, alpha and a prediction afterwards equal a fresh context's, and no
    factorisation was added."""
    name = BIG
    N, comp, T, nd, layout, k = dc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = dc.inputs(name)
    Xte = synth.test_points(40)
    fresh = gpak.Gpak(0)
    try:
        fresh.set_train(X, y)
        tb.set_composition(fresh, terms, bias, sn2, white)
        want = (fresh.logLikelihood(), fresh.solve_alpha(), fresh.posteriorMeanVar(Xte), fresh.predict_joint(Xt, nd))
    finally:
        fresh.close()
    gp.set_train(X, y)
    tb.set_composition(gp, terms, bias, sn2, white)
    try:
        nlz = gp.logLikelihood()
        n0 = gp.timing()["evaluations"]
        gp.design(Xt, nd, Xc, hole, None, 2, True)
        got = (gp.logLikelihood(), gp.solve_alpha(), gp.posteriorMeanVar(Xte), gp.predict_joint(Xt, nd))
        assert gp.timing()["evaluations"] == n0 and got[0] == nlz == want[0]
    finally:
        tb.set_defaults(gp)
    assert same(got[1], want[1])
    for a, b in zip(got[2] + got[3], want[2] + want[3]):
        assert same(a, b)


# ---- 5. statuses ------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_factorisation(gp):
    name = SMALL
    N, comp, T, nd, layout, k = dc.CASES[name]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    X, y, Xt, Xc, hole = dc.inputs(name)
    H, Mc = int(hole.max()) + 1, len(hole)
    lib, h = gp._lib, gp._h
    ip = lambda a: None if a is None else a.ctypes.data_as(gpak.C.POINTER(gpak.C.c_int))   # noqa: E731
    p = gpak._p
    gain, picked, pick_gain = np.zeros(H), np.zeros(H, dtype=np.int32), np.zeros(H)
    Xtf, Xcf = np.asfortranarray(Xt), np.asfortranarray(Xc)

    def call(**kw):
        a = dict(Xt=p(Xtf), T=T, nd=nd, Xc=p(Xcf), Mc=Mc, d=3, hole=ip(hole), H=H, wt=None, k=1, gain=p(gain), red=None, var=None,
                 picked=ip(picked), pick_gain=p(pick_gain), var_after=None, summary=None)
        a.update(kw)
        rc = lib.gpak_design(h, *a.values())
        return rc, gp.last_error()

    gp.set_train(X, y)
    tb.set_composition(gp, terms, bias, sn2, white)
    try:
        n0 = gp.timing()["evaluations"]
        big = hole.copy()
        big[:] = 0
        unused = np.where(hole == 2, 1, hole).astype(np.int32)
        outside = hole.copy()
        outside[4] = H
        many = np.zeros(129, dtype=np.int32)
        X129 = np.asfortranarray(np.tile(Xc[:1], (129, 1)) + 0.001 * np.arange(129)[:, None])
        wneg, wnan = np.ones(T), np.ones(T)
        wneg[3], wnan[5] = -1.0, np.nan
        cases = [
            (dict(T=0), "must all be positive"), (dict(nd=0), "must all be positive"), (dict(Mc=0), "must all be positive"),
            (dict(d=4), "as many columns as the training set"),
            (dict(Xt=None), "Xt is NULL"), (dict(Xc=None), "Xc is NULL"), (dict(hole=None), "hole is NULL"),
            (dict(gain=None), "gain is NULL"),
            (dict(H=0), "H = 0 is outside [1, Mc = 57]"), (dict(H=Mc + 1), "is outside [1, Mc = 57]"),
            (dict(hole=ip(outside)), f"point 4 has label {H}, outside [0, {H})"),
            (dict(hole=ip(unused)), "label 2 is not used"),
            (dict(hole=ip(many), H=1, Mc=129, Xc=p(X129)), "hole 0 has more than 128 points (point 128 is one too many)"),
            (dict(wt=p(wneg)), "weight 3 is negative or not finite"), (dict(wt=p(wnan)), "weight 5 is negative or not finite"),
            (dict(k=-1), "k = -1 is outside [0, H = 6]"), (dict(k=H + 1), "k = 7 is outside [0, H = 6]"),
            (dict(picked=None), "picked is NULL with k > 0"), (dict(pick_gain=None), "pick_gain is NULL with k > 0"),
            (dict(T=1 << 23, nd=64), "1 GiB point budget"),
        ]
        assert Mc == 57
        for kw, text in cases:
            rc, err = call(**kw)
            assert rc == gpak.EINVAL and text in err and err.startswith("gpak_design: "), (kw.keys(), rc, err)
        assert gp.timing()["evaluations"] == n0                  # nothing was factored for any of them
        rc, err = call()
        assert rc == gpak.OK and 0 <= picked[0] < H and pick_gain[0] == gain[picked[0]]
        picked[:], pick_gain[:] = -7, -7.0                       # k = 0 leaves both untouched, NULL or not
        assert call(k=0)[0] == gpak.OK and call(k=0, picked=None, pick_gain=None)[0] == gpak.OK
        assert np.all(picked == -7) and np.all(pick_gain == -7.0)
    finally:
        tb.set_defaults(gp)
    # ESTATE: no training set; no parameters
    g2 = gpak.Gpak(0)
    try:
        rc = g2._lib.gpak_design(g2._h, p(Xtf), T, nd, p(Xcf), Mc, 3, ip(hole), H, None, 0, p(gain), None, None, None, None, None, None)
        assert rc == gpak.ESTATE and "no training set" in g2.last_error()
        g2.set_train(X, y)
        rc = g2._lib.gpak_design(g2._h, p(Xtf), T, nd, p(Xcf), Mc, 3, ip(hole), H, None, 0, p(gain), None, None, None, None, None, None)
        assert rc == gpak.ESTATE and "no parameters" in g2.last_error()
    finally:
        g2.close()


def test_multi_gpu_context_is_refused():
    name = SMALL
    N, comp, T, nd, layout, k = dc.CASES[name]
    X, y, Xt, Xc, hole = dc.inputs(name)
    X, y = tb.data(513, 3)
    g = gpak.Gpak(devices=[0, 0])
    try:
        g.set_train(X[:256], y[:256])
        g.set_params(np.array(tb.THETA2), 0.35, 0.05)
        with pytest.raises(gpak.GpakError) as ei:
            g.design(Xt, nd, Xc, hole)
        assert ei.value.status == gpak.ENOTIMPL and "single-GPU context" in str(ei.value)
    finally:
        g.close()


def test_failed_training_factor_gives_nan(gp):
    name = SMALL
    N, comp, T, nd, layout, k = dc.CASES[name]
    X, y, Xt, Xc, hole = dc.inputs(name)
    gp.set_train(X, y)
    gp.set_params(np.array(tb.THETA2), 0.35, -1.0)               # a negative sn2: B is not positive definite
    try:
        gain, picked, pick_gain, ex = gp.design(Xt, nd, Xc, hole, None, 2, True)
        err = gp.last_error()
    finally:
        tb.set_defaults(gp)
    assert ex["summary"]["status"] == gpak.ENOTPD and "training factor" in err
    for a in (gain, pick_gain, ex["reduction"], ex["var"], ex["var_after"]):
        assert np.all(np.isnan(a))
    assert np.isnan(ex["summary"]["var_before"]) and np.isnan(ex["summary"]["var_after"])


# ---- 6. the command line ----------------------------------------------------------------------------------------------
def test_cli_design_after_train(gp, tmp_path):
    """train on N = 512 (two iterations), then design on 20 target blocks at 2 x 2 x 2 and five candidate holes under
    labels that are neither sorted nor dense.  The standardisation of this set is the identity, so the file's gains are
    those of Gpak.design with the trained parameters, at the file's six digits; --pick 3 marks three holes."""
    import make_golden_lbfgs
    tb.build()
    N, T = 512, 20
    Xs, ys = make_golden_lbfgs.prepared(N)
    tb.write_csv(tmp_path / "train.txt", Xs, ys)
    rng = np.random.default_rng(60)
    centres = rng.uniform(Xs.min(axis=0) + 0.05, Xs.max(axis=0) - 0.05, (T, 3))
    tb.write_csv(tmp_path / "targets.txt", centres, np.zeros(T))
    sizes, names = [6, 9, 4, 12, 7], [40, -3, 17, 5, 8]
    pts, lab = [], []
    for m, nm in zip(sizes, names):
        q = np.tile(rng.uniform(0.8 * Xs.min(axis=0), 0.8 * Xs.max(axis=0)), (m, 1))
        q[:, 2] = 0.8 * Xs[:, 2].max() - 0.02 * np.arange(m)
        pts.append(q)
        lab += [nm] * m
    Xc = np.vstack(pts)
    tb.write_csv(tmp_path / "cand.txt", Xc, np.zeros(len(Xc)))
    with open(tmp_path / "holes.txt", "w") as f:
        f.write("# hole of each candidate point\n" + "\n".join(str(v) for v in lab) + "\n")
    w = 0.5 + np.arange(T) % 3
    np.savetxt(tmp_path / "w.txt", w)
    exe, model = os.path.join(HOST, "gp_ss_ak"), str(tmp_path / "model")
    env = dict(os.environ, GPAK_MAX_ITERS="2")
    env.pop("GPAK_OPT", None)
    subprocess.run([exe, "-v", "1", "-np", "train", "-k", "ExpAns", "-kn", "1", "-o", "LBFGS", str(tmp_path / "train.txt"), model],
                   env=env, cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    stats = np.loadtxt(model + "_Statistics.txt", delimiter=",")
    assert np.all(stats[:, 0] == 0.0) and np.all(stats[:, 1] == 1.0)
    r = subprocess.run([exe, "-v", "1", "--block-size", "0.08,0.06,0.04", "--block-disc", "2,2,2", "--pick", "3", "--weights",
                        str(tmp_path / "w.txt"), "design", "--candidates", str(tmp_path / "cand.txt"), "--holes",
                        str(tmp_path / "holes.txt"), str(tmp_path / "targets.txt"), model, str(tmp_path / "train.txt")],
                       cwd=tmp_path, input=b"", stdout=subprocess.PIPE, check=True)
    text = r.stdout.decode()
    lines = open(model + "_design.txt").read().splitlines()
    assert lines[0] == "# Hole, Samples, Gain, Share, Pick"
    rows = [line.split() for line in lines[1:]]
    assert [int(v[0]) for v in rows] == sorted(names)                    # ascending label
    assert [int(v[1]) for v in rows] == [sizes[names.index(nm)] for nm in sorted(names)]

    body = open(model).read().splitlines()[1:]
    values = [line.split() for line in body if "=" not in line and line.strip()]
    e, bias = [float(v) for v in values[0]], float(values[1][0])
    sn2 = float([line for line in body if line.startswith("Hyperparams_likelihood=")][0].split("=")[1])
    Xd, nd = gpak.block_points(centres, (0.08, 0.06, 0.04), (2, 2, 2))
    gp.set_train(Xs, ys)
    gp.set_params(np.array(e), bias, sn2, gpak.DIST_DIRECT)
    try:
        gain, picked, pick_gain, ex = gp.design(Xd, nd, Xc, np.array(lab), w, 3)
    finally:
        tb.set_defaults(gp)

    def close(a, b):
        return np.all(np.abs(np.asarray(a, dtype=float) - b) <= 1e-5 * np.abs(b))

    s = ex["summary"]
    assert list(s["labels"]) == sorted(names)
    assert close([v[2] for v in rows], gain) and close([v[3] for v in rows], gain / s["var_before"])
    marks = [int(v[4]) for v in rows]
    assert sorted(marks) == [0, 0, 1, 2, 3] and [marks.index(j + 1) for j in range(3)] == list(picked)
    for j in range(3):
        assert len(rows[picked[j]]) == 6 and close([rows[picked[j]][5]], pick_gain[j:j + 1])
    assert all(len(v) == 5 for v, m in zip(rows, marks) if m == 0)
    assert "var_before" in text and "var_after" in text and "device time" in text
    for j in range(3):
        assert f"pick {j + 1}: hole {s['labels'][picked[j]]} " in text
