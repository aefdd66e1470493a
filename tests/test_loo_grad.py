"""CPU tests (-m "not gpu") of the leave-one-out gradient feature:

1. tests/loo_grad_ref.py (the NumPy restatement gpak_loo_grad is compared with on the GPU) against central differences
   of -log_pl of tests/loo_ref.py;
2. the same restatement against a second float64 route to the weight matrix (np.linalg.inv for the Cholesky inverse);
3. the `--objective` option of the command line: what it accepts and what it refuses, before any device is opened;
4. include/gpak_loo_grad.h against the binding and the library, as tests/test_abi.py holds include/gpak.h;
5. the call sequence of tests/loo_grad_model.py on the stateless model and on the restatement of api.hip's validity logic,
   as tests/test_ctx_sequences.py holds the calls of its vocabulary.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gp_ss_ak_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_grad_ref as xref  # noqa: E402
import ctx_sequences as cs  # noqa: E402
import loo_grad_model as lgm  # noqa: E402
import loo_grad_ref as lref  # noqa: E402
from test_abi import header_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gp_ss_ak_amd", "host")

E = list(synth.DEFAULT_EXPANS)
THETA2 = [0.3, 1.7, -0.4, 1.1, 0.8, 0.6, 1.2, 0.9]
PARAMS = {"defaults": (E, synth.DEFAULT_BIAS, synth.DEFAULT_SN2), "theta2": (THETA2, 0.35, 0.05)}
# (N, input columns)
SIZES = [(64, 3), (200, 3), (513, 3), (512, 4)]
CASES = [(N, cols, name) for N, cols in SIZES for name in ("defaults", "theta2")]


def build():
    subprocess.check_call(["make", "-s", "-C", HOST])


def data(N, cols):
    return synth.drillholes4(N) if cols == 4 else synth.drillholes(N)


_GRAD = {}


def restatement(N, cols, name):
    """(gradient, W) of the Cholesky route, computed once per case."""
    key = (N, cols, name)
    if key not in _GRAD:
        X, y = data(N, cols)
        e, bias, sn2 = PARAMS[name]
        _GRAD[key] = lref.grad_loo(X, y, [(xref.EXPANS, e)], bias, sn2, want_w=True)
    return _GRAD[key]


@pytest.mark.parametrize("N,cols,name", CASES)
def test_restatement_matches_central_differences(N, cols, name):
    """One inverse width (lam_x, entry 1) and Sigma (entry 6) with h = 1e-5, the bias (entry 8) with h = 1e-5, sn2
    (entry 9) with h = 1e-6; with four columns InversewidthR (entry 7) as well.  Bound 1e-7 of |g|inf: the truncation
    of a central difference is h^2 f''' / 6 and its rounding eps |F| / h ~ 1e-9 on entries >= 1."""
    X, y = data(N, cols)
    e, bias, sn2 = PARAMS[name]
    g, _ = restatement(N, cols, name)
    x0 = np.array(list(e) + [bias, sn2])

    def F(x):
        return lref.objective(X, y, [(xref.EXPANS, x[:8])], float(x[8]), float(x[9]))

    worst = 0.0
    for k, h in [(1, 1e-5), (6, 1e-5), (8, 1e-5), (9, 1e-6)] + ([(7, 1e-5)] if cols == 4 else []):
        d = np.zeros(10)
        d[k] = h
        fd = (F(x0 + d) - F(x0 - d)) / (2 * h)
        err = abs(g[k] - fd) / np.abs(g).max()
        worst = max(worst, err)
        print(f"\nN={N} d={cols} {name} entry {k}: restatement {g[k]:.12g}, differences {fd:.12g}, |err| / |g|inf = {err:.3g}")
    assert worst <= 1e-7
    if cols == 3:
        assert g[7] == 0.0


@pytest.mark.parametrize("N,cols,name", CASES)
def test_restatement_matches_a_second_float64_route(N, cols, name):
    """np.linalg.inv in place of the Cholesky inverse.  Kernel block <= 1e-10 of its largest entry, the sn2 entry <=
    1e-10 of itself.  The bias entry, 1/2 sum W, cancels by about 10^8: the two routes differ by up to 2.6e-10 of it, which
    is 5e-18 of 1/2 sum |W| -- printed here in both units, bounded on the device (tests/test_loo_grad_gpu.py)."""
    X, y = data(N, cols)
    e, bias, sn2 = PARAMS[name]
    g, W = restatement(N, cols, name)
    g2 = lref.grad_loo(X, y, [(xref.EXPANS, e)], bias, sn2, route="inv")
    ek = np.abs(g2[:8] - g[:8]).max() / np.abs(g[:8]).max()
    es = abs(g2[9] - g[9]) / abs(g[9])
    eb = abs(g2[8] - g[8])
    print(f"\nN={N} d={cols} {name}: kernel block {ek:.3g}, sn2 {es:.3g} relative; bias entry {g[8]:.6g}: "
          f"{eb / abs(g[8]):.3g} of itself, {eb / (0.5 * np.abs(W).sum()):.3g} of 1/2 sum|W| = {0.5 * np.abs(W).sum():.6g}")
    assert ek <= 1e-10 and es <= 1e-10


@pytest.mark.parametrize("args,msg", [
    (["--objective", "bogus", "train", "x.txt"], "--objective takes nlz or loo"),
    (["--objective", "loo", "--gradient", "reference", "train", "x.txt"], "drop --gradient reference"),
    (["--gradient", "reference", "--objective", "loo", "train", "x.txt"], "drop --gradient reference"),
    (["--objective", "loo", "--gpus", "2", "train", "x.txt"], "one GPU only"),
    (["--gpus", "2", "--objective", "loo", "train", "x.txt"], "one GPU only"),
    (["-g", "2", "--gradient", "exact", "--objective", "loo", "train", "x.txt"], "one GPU only"),
])
def test_cli_refuses_bad_objective_options(args, msg):
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert msg in r.stderr.decode()


@pytest.mark.parametrize("args", [
    ["--objective", "loo", "train"],
    ["--objective", "nlz", "train"],
    ["--objective", "loo", "--gradient", "exact", "train"],
    ["--gradient", "exact", "--objective", "loo", "train"],
    ["--objective", "nlz", "--gradient", "reference", "train"],
    ["--objective", "nlz", "--gpus", "2", "train"],
])
def test_cli_accepts_the_objective_option(args):
    """The option and its combinations pass the parser: `train` without a data file then stops at its own check, before
    any device is opened."""
    build()
    r = subprocess.run([os.path.join(HOST, "gp_ss_ak"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0
    assert "There are not enough input parameters." in r.stderr.decode()


def test_header_binding_and_library_list_the_same_symbols():
    import ctypes
    declared = header_functions("gpak_loo_grad.h")
    assert declared == sorted(_lib.LOO_GRAD_SYMBOLS) == ["gpak_loo_grad"]
    assert not set(declared) & set(header_functions())               # declared once
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gpak_loo_grad.h"\n'
                   'int main(void){gpak_loo_summary s; (void)s; return gpak_loo_grad(0, 0, 0, 0) == GPAK_EINVAL ? GPAK_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


# ---- the call sequence on the models ------------------------------------------------------------------------------------
CACHE = {}
_RUNS = {}


def expected():
    if "want" not in _RUNS:
        _RUNS["want"] = lgm.run(lambda: lgm.LooGradModel(lgm.cm.F64, CACHE))
    return _RUNS["want"]


def test_sequence_on_the_models():
    """The stateless model and the unmutated restatement of api.hip agree step for step, and every step answers with the
    status the header promises."""
    want = expected()
    caching = lgm.run(lambda: lgm.LooGradCaching(lgm.cm.F64, CACHE))
    asked = 0
    for w, c, (method, kw, due) in zip(want, caching, lgm.SEQUENCE):
        if method == "timing":
            continue
        assert w["res"][0] == due and cs.same_bits(w["res"], c["res"]), (w["i"], method, kw, w["res"][0], c["res"][0])
        asked += method == "loo_grad"
    assert len(want) == len(caching) == len(lgm.SEQUENCE) and asked >= 12
    assert {w["res"][0] for w in want if w["method"] == "loo_grad"} == {lgm.OK, lgm.ENOTPD, lgm.EINVAL, lgm.ESTATE, lgm.ENOTIMPL}
    # a refused call factors nothing; a failed factorisation is tried again at every question
    evals = [int(c["res"][1][0][0]) for c in caching if c["method"] == "timing"]
    assert evals[0] == 1 and evals[2] == evals[1] + 3 and evals[3] == 1, evals


# mutation of ctx_model.CachingModel (one dropped invalidation of api.hip) -> index of the first step off the model: the
# first gpak_loo_grad after the call whose invalidation was dropped
CAUGHT_AT = {"set_kernel keeps U": 18, "failed factor keeps alpha": 28, "set_train keeps alpha": 36}


@pytest.mark.parametrize("mutation", sorted(CAUGHT_AT))
def test_a_dropped_invalidation_is_caught_by_the_next_loo_gradient(mutation):
    want = expected()
    made = []

    def make():
        made.append(lgm.LooGradCaching(lgm.cm.F64, CACHE, [mutation]))
        return made[-1]

    first = None
    for w, rec in zip(want, lgm.run(make)):
        if rec["method"] in cs.SETTERS or rec["method"] == "timing":
            continue
        ratio = cs.worst(lgm.errors(w, rec["res"], w["res"], CACHE))
        if ratio > 1.0:
            first = (rec["i"], rec["method"], ratio)
            break
    assert first is not None, f"{mutation}: the sequence runs on the mutated model without a difference"
    print(f"\n{mutation}: step {first[0]} ({first[1]}) is {first[2]:.3g} bounds off the model")
    assert made[0].dropped and all(d[0] == mutation for d in made[0].dropped)
    assert first[:2] == (CAUGHT_AT[mutation], "loo_grad")


def test_distinct_states_are_a_thousand_bounds_apart():
    """The model's gradient in every OTHER state of the sequence with a gradient of the same length is at least 1000 bounds
    away from the step's own: an answer served from a stale state cannot pass."""
    want = expected()
    states = {}
    for w in want:
        if w["train"] and w["kern"]:
            states.setdefault((w["train"], cs.kern_values(*w["kern"])), w)
    pairs, closest = 0, float("inf")
    for w in want:
        if w["method"] != "loo_grad" or w["res"][0] != lgm.OK:
            continue
        for st, other in states.items():
            if st == (w["train"], cs.kern_values(*w["kern"])):
                continue
            stale = lgm.ask(lgm.model_at(other, CACHE), "loo_grad", w["kw"], 0)
            if stale[0] != lgm.OK:
                continue                      # another status: caught as such
            ratio = cs.worst(lgm.errors(w, stale, w["res"], CACHE))
            pairs, closest = pairs + 1, min(closest, ratio)
            assert ratio >= 1000.0, (w["i"], w["kw"], "against", st[0], other["kern"])
    print(f"\n{len(states)} states, {pairs} (step, other state) pairs, the closest {closest:.3g} bounds apart")
    assert len(states) >= 5 and pairs >= 10
