"""One long-lived context against fresh ones across call orders (tests/ctx_sequences.py, tests/ctx_model.py).

CPU (-m "not gpu"): every sequence runs on ModelGpak and, step for step equal, on the unmutated CachingModel; each named
mutation of the context's validity logic is caught by a named sequence; any two distinct states of a sequence give model
answers at least 1000 bounds apart, so that an answer from the wrong state cannot hide inside a bound; every function
include/gpak.h declares is called somewhere.

GPU (-m gpu): one fresh process per group (tests/ctx_seq_worker.py).  Every step of the long-lived context is (a)
bit-equal to a fresh context's answer (four steps excepted: MODEL_ONLY says why) and (b) within the method's existing bound of
the model; the count of factorisations (gpak_timing) is that of the unmutated CachingModel.  Figures per group:
DESIGN.md section 8, "Call sequences on one context".
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_model as cm  # noqa: E402
import ctx_sequences as cs  # noqa: E402
from test_abi import header_functions  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CACHE = {}          # ModelGpak's results, shared by every test of this module
SEPARATION = 1000.0
# declared in include/gpak.h and out of this module's scope: the multi-GPU surface (its own state, its own issue), the
# calibration microbenchmarks, the process-wide tuning reload, the error text before a context exists
EXCLUDED = {"gpak_create_multi", "gpak_n_gpus", "gpak_transport", "gpak_calibrate", "gpak_reload_tuning", "gpak_global_error"}
# Steps held to the model alone, (sequence, step) -> why their bits legitimately depend on earlier calls.
# How a context substitutes backwards is settled when it FACTORS (api.hip ensure_factor: the explicit 512-block inverses and
# the [R ; T] stacks are built beside the factorisation's forward substitution only), so GPAK_OPT_INV512 / GPAK_OPT_BWD_FUSED
# changed afterwards take effect at the next factorisation.  Until then the long-lived context keeps the back substitution
# of the options it factored under while a fresh context, given the current options, uses another: the same alpha and
# solve_chol in another summation order (measured: they differ in the last bits, and are equal again after gpak_set_params).
_BACKSOLVE = "options of the back substitution changed since the factorisation"
MODEL_ONLY = {("solve scratch", 11): _BACKSOLVE, ("solve scratch", 12): _BACKSOLVE, ("solve scratch", 15): _BACKSOLVE,
              ("solve scratch", 16): _BACKSOLVE}


def model_run(seq, mut=None):
    make = (lambda p: cm.ModelGpak(p, CACHE)) if mut is None else (lambda p: cm.CachingModel(p, CACHE, mut))
    return list(cs.run(seq, make))


_MODEL_RUNS = {}


def expected(seq):
    if seq["name"] not in _MODEL_RUNS:
        _MODEL_RUNS[seq["name"]] = model_run(seq)
    return _MODEL_RUNS[seq["name"]]


def judge(seq, rec, want, got=None):
    """(worst error / bound, [(label, error, bound)]) of a step's result against the model's."""
    m = cs.model_at(want, CACHE, seq["precision"])
    errs = cs.model_errors(rec["method"], rec["kw"], rec["res"] if got is None else got, want["res"], m, seq["precision"])
    return cs.worst(errs), errs


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s["name"] for s in cs.SEQUENCES])
def test_sequence_on_the_models(name):
    seq = cs.BY_NAME[name]
    want = expected(seq)
    caching = model_run(seq, mut=())
    counted = 0
    for w, c in zip(want, caching):
        if w["method"] == "timing":
            assert w["res"][1] == [None] and c["res"][1][0].shape == (1,)
            continue
        assert cs.same_bits(w["res"], c["res"]), (name, w["i"], w["method"], w["kw"], w["res"][0], c["res"][0])
        counted += w["method"] not in cs.SETTERS
    assert len(want) == len(caching) == len(seq["steps"]) and counted > 0
    statuses = {w["res"][0] for w in want}
    print(f"{name}: {len(want)} steps, {counted} compared, statuses {sorted(statuses)}")


def test_the_sequences_meet_the_statuses_the_header_promises():
    seen = {}
    for seq in cs.SEQUENCES:
        for w in expected(seq):
            seen.setdefault(w["res"][0], set()).add((seq["name"], w["method"]))
    assert ("out of order", "logLikelihood") in seen[cs.ESTATE] and ("out of order", "predict_block") in seen[cs.ESTATE]
    assert ("gradients", "GradLL") in seen[cs.ENOTIMPL] and ("gradients", "GradLL_exact") in seen[cs.ENOTIMPL]
    assert ("fail and recover", "GradLL") in seen[cs.ENOTPD] and ("fail and recover", "posteriorMeanVar") in seen[cs.ENOTPD]
    assert ("fail and recover", "loo") in seen[cs.ENOTPD]
    assert cs.EINVAL in seen
    fail = expected(cs.BY_NAME["fail and recover"])
    nan_steps = [w["method"] for w in fail if w["res"][1] and all(v is not None and np.isnan(v).all() for v in w["res"][1])]
    assert {"logLikelihood", "loo", "predict_block", "predict_joint", "sample_joint"} <= set(nan_steps)
    cols = [int(w["res"][1][0][0]) for w in fail if w["method"] == "failed_column"]
    assert cols[0] == 0 and all(c >= 1 for c in cols[1:-1]) and cols[-1] == 0 and len(cols) >= 4


# mutation -> (the named sequence that catches it, index and method of its first step off the model).  That step is the
# first one after the call whose invalidation was dropped that reads what the call should have invalidated: the very next
# step everywhere but for `gram keeps factor` (gram at 5; solve_alpha at 6 returns the alpha the context still rightly holds;
# the variance at 7 reads the matrix buffer), `predict leaks pooled mean` (prediction at 7; loo and compute_k do not read the
# training points' transformed copy, the Gram matrix at 10 does) and `recovery keeps failed_column` (good parameters at 33,
# the factorisation at 34, the question at 35).
CAUGHT_BY = {
    "memo ignores composition": ("memo", 6, "logLikelihood"),
    "gram keeps factor": ("gram between [direct]", 7, "posteriorMeanVar"),
    "set_train keeps alpha": ("size walk", 19, "posteriorMeanVar"),
    "set_kernel keeps U": ("gradients", 9, "GradLL_hyb"),
    "failed factor keeps alpha": ("fail and recover", 13, "logLikelihood"),
    "solve_chol keeps z": ("solve scratch", 4, "solve_alpha"),
    "predict leaks pooled mean": ("gram between [expansion]", 10, "gram"),
    "f32 image kept": ("f32", 5, "posteriorMeanVar"),
    "recovery keeps failed_column": ("fail and recover", 35, "failed_column"),
}


def first_divergence(seq, mut):
    want = expected(seq)
    made = []

    def make(p):
        made.append(cm.CachingModel(p, CACHE, mut))
        return made[-1]

    it = cs.run(seq, make)
    for w, rec in zip(want, it):
        if rec["method"] in cs.SETTERS or rec["method"] == "timing":
            continue
        ratio, errs = judge(seq, rec, w)
        if ratio > 1.0:
            it.close()
            return rec, ratio, [d for g in made for d in g.dropped]
    return None, 0.0, [d for g in made for d in g.dropped]


@pytest.mark.parametrize("mutation", cm.MUTATIONS)
def test_each_mutation_is_caught(mutation):
    """The first step off the model comes after the call whose invalidation was dropped, and is the first later step that
    reads what that call should have invalidated."""
    name, index, method = CAUGHT_BY[mutation]
    seq = cs.BY_NAME[name]
    rec, ratio, dropped = first_divergence(seq, [mutation])
    assert rec is not None, f"{mutation}: the sequence '{name}' runs on the mutated model without a difference"
    print(f"{mutation}: '{name}' step {rec['i']} ({rec['method']} {rec['kw']}) is {ratio:.3g} bounds off the model")
    assert dropped and all(d[0] == mutation for d in dropped)
    assert rec["method"] == method and (index is None or rec["i"] == index), (rec["i"], rec["method"])
    # the step before it in the same context changed or kept the state (one after the dropped invalidation) or, where the
    # kept quantity is read later only, every compared step in between agreed with the model (first_divergence)
    assert rec["i"] > 0


def test_the_steps_held_to_the_model_alone_are_what_their_reason_says():
    for (name, i), why in MODEL_ONLY.items():
        steps = cs.BY_NAME[name]["steps"]
        assert steps[i][1] in ("solve_chol", "solve_alpha", "logLikelihood")
        back = [k for k in range(i) if steps[k][1] in ("set_params", "set_kernel", "set_train", "gram")][-1]
        changed = [k for k in range(back, i) if steps[k][1] == "set_option" and steps[k][2]["opt"] in ("INV512", "BWD_FUSED")]
        assert changed and why == _BACKSOLVE


def test_the_mutations_table_is_the_models():
    assert set(CAUGHT_BY) == set(cm.MUTATIONS) and len(cm.MUTATIONS) == 9
    assert {v[0] for v in CAUGHT_BY.values()} <= {s["name"] for s in cs.SEQUENCES if s["group"] != "random"}


@pytest.mark.parametrize("name", [s["name"] for s in cs.SEQUENCES])
def test_distinct_states_are_a_thousand_bounds_apart(name):
    """For every compared step: the model's answer to the same question in every OTHER state the sequence's context of
    the same precision goes through (same number of input columns; a gradient of the same length) is at least 1000 bounds
    away -- an answer served from a stale state cannot pass (b).  Where the model's two answers are the same bytes the
    question does not read what differs between the states (gram, compute_k, block_cross: sn2; compute_k: the training set).
    `factor` and `failed_column` answer yes / no and are left out; `timing` is no function of the state.  States that differ in the distance form or in the
    options alone are one state here: those change how an answer is computed, not what it is."""
    seq = cs.BY_NAME[name]
    want = expected(seq)
    states = {}
    for w in want:
        if w["train"] and w["kern"]:
            states.setdefault(w["state"], w)
    closest = (float("inf"), None)
    pairs = 0
    for w in want:
        if w["method"] in cs.SETTERS + ("timing", "factor", "failed_column") or w["res"][0] != cs.OK or not w["train"]:
            continue
        if any(v is not None and np.isnan(v).any() for v in w["res"][1]):
            continue
        for st, other in states.items():
            if st == w["state"] or cs.TRAIN[other["train"]][1] != cs.TRAIN[w["train"]][1]:
                continue
            m = cs.model_at(dict(other, kern=(other["kern"][0], other["kern"][1], w["mode"])), CACHE, seq["precision"])
            stale = cs.invoke(m, w["method"], w["kw"], cs.TRAIN[other["train"]][0])
            if stale[0] != cs.OK or any(v is not None and np.isnan(v).any() for v in stale[1]):
                continue                      # another status: caught as such
            if cs.same_bits(stale, w["res"]):
                continue                      # the question does not read what differs (block_cross and sn2)
            ratio, errs = judge(seq, w, w, got=stale)
            pairs += 1
            if ratio < closest[0]:
                closest = (ratio, (w["i"], w["method"], w["kw"], st[0], errs))
            assert ratio >= SEPARATION, (name, w["i"], w["method"], w["kw"], "against", other["train"], other["kern"], errs)
    print(f"{name}: {len(states)} states, {pairs} (step, other state) pairs, the closest {closest[0]:.3g} bounds apart: {closest[1]}")
    if name not in ("out of order",):
        assert len(states) >= 2 and pairs > 0


@pytest.mark.parametrize("status", [-1, cm.ENOMEM])
def test_a_failure_that_is_no_answer_ends_the_run(status):
    """GPAK_EHIP (a HIP failure: the device may have faulted) and GPAK_ENOMEM are not turned into results: the call raises with
    the library's message, no later step runs, no fresh context is made for that step, and no context is closed."""
    log = []

    class Faulting(cm.ModelGpak):
        def __init__(self, p, fresh=False):
            super().__init__(p, CACHE)
            log.append("fresh context" if fresh else "context")

        def solve_alpha(self):
            log.append("solve_alpha")
            raise cm.ModelError(status, "hipMemcpyAsync: an illegal memory access was encountered")

        def logLikelihood(self):
            log.append("logLikelihood")
            return super().logLikelihood()

        def close(self):
            log.append("close")

    seq = dict(name="fault", group="fault", precision=cs.F64,
               steps=[cs.S("set_train", train="T129"), cs.S("set_params", kern="E"), cs.S("logLikelihood"), cs.S("solve_alpha"),
                      cs.S("logLikelihood")])
    try:
        with pytest.raises(cm.ModelError) as ei:
            list(cs.run(seq, Faulting, lambda p: Faulting(p, fresh=True), {}))
        assert ei.value.status == status and "illegal memory access" in str(ei.value)
        assert len(cs.DEVICE_ERROR) == 1 and "illegal memory access" in cs.DEVICE_ERROR[0]
        # one long-lived context, one fresh one for the first logLikelihood (closed before the failure), then the failing call
        assert log == ["context", "logLikelihood", "fresh context", "logLikelihood", "close", "solve_alpha"], log
        assert len(cs.LEAKED) == 1
    finally:
        del cs.DEVICE_ERROR[:], cs.LEAKED[:]
    # the statuses the header lists as answers ARE results
    for ok in cs.API_STATUSES:
        class Refusing(cm.ModelGpak):
            def solve_alpha(self):
                raise cm.ModelError(ok, "refused")
        assert cs.invoke(Refusing(), "solve_alpha", {}, 0) == (ok, []) and not cs.DEVICE_ERROR
    assert -1 not in cs.API_STATUSES and cm.ENOMEM not in cs.API_STATUSES and cs.OK not in cs.API_STATUSES


def test_a_refused_setter_ends_the_run():
    class NoTrain(cm.ModelGpak):
        def set_train(self, X, y):
            raise cm.ModelError(cm.ENOTIMPL, "refused")
    seq = dict(name="setter", group="setter", precision=cs.F64, steps=[cs.S("set_train", train="T129"), cs.S("logLikelihood")])
    try:
        with pytest.raises(RuntimeError):
            list(cs.run(seq, lambda p: NoTrain(p, CACHE)))
        assert cs.DEVICE_ERROR
    finally:
        del cs.DEVICE_ERROR[:], cs.LEAKED[:]


def test_every_declared_function_is_called_in_some_sequence():
    called = set(cs.ALWAYS)
    for seq in cs.SEQUENCES:
        called |= {cs.ENTRY[m] for _c, m, _kw in seq["steps"]}
    declared = set(header_functions())
    assert EXCLUDED <= declared
    missing = declared - called - EXCLUDED
    assert not missing, sorted(missing)
    assert called <= declared, sorted(called - declared)
    named = {cs.ENTRY[m] for s in cs.SEQUENCES if s["group"] != "random" for _c, m, _kw in s["steps"]}
    assert named | cs.ALWAYS == called          # the named sequences alone reach every one of them


def test_random_sequences_are_fixed_and_cover_the_vocabulary():
    assert [s["steps"] for s in cs.SEQUENCES if s["group"] == "random"] == [cs.seq_random(k) for k in range(cs.RANDOM_COUNT)]
    methods = {m for s in cs.SEQUENCES if s["group"] == "random" for _c, m, _kw in s["steps"]}
    assert len(methods) >= 18, sorted(methods)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
_DEVICE_TROUBLE = []       # set by the first worker that faulted, aborted, was killed or timed out: no further GPU process
# Measured on an MI355X: the slowest group (`random`) takes 5.5 to 6.4 s in its worker over three runs, about 7 s with the start of the process
# and the model's side on the CPU; the limit is ten times that, for a busy shared machine.
WORST_GROUP_SECONDS = 7
TIMEOUT = 10 * WORST_GROUP_SECONDS


def _worker(group, out):
    return subprocess.run([sys.executable, os.path.join(HERE, "ctx_seq_worker.py"), "--group", group, "--out", out], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)


@pytest.mark.gpu
@pytest.mark.parametrize("group", cs.GROUPS)
def test_sequences_on_the_device(group, tmp_path):
    if _DEVICE_TROUBLE:
        pytest.fail(f"not started: {_DEVICE_TROUBLE[0]}")
    out = str(tmp_path / "results.npz")
    try:
        r = _worker(group, out)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"the worker of group {group} did not finish in {TIMEOUT} s")
        pytest.fail(_DEVICE_TROUBLE[0])
    err = r.stderr.decode()
    if r.returncode != 0 or "HIP error" in err or "hipError" in err or "illegal memory access" in err:
        # a worker ends with 0 only when every step ran; anything else (a signal, an abort, GPAK_EHIP raised by a step: status 2)
        # may be a faulted device
        _DEVICE_TROUBLE.append(f"the worker of group {group} ended with status {r.returncode}: {err[-1500:]}")
        pytest.fail(_DEVICE_TROUBLE[0])
    lines = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
    failures, summary = judge_group(group, lines, np.load(out))
    print(summary)
    assert not failures, "\n".join(failures)


def judge_group(group, lines, arrays):
    """The worker's records and arrays of one group against fresh contexts (a) and the model (b): (failures, summary)."""
    done = lines.pop()
    assert done["done"] == group
    failures, bit_equal, compared, worst = [], 0, 0, (0.0, None)
    index = {s["name"]: k for k, s in enumerate(cs.SEQUENCES)}
    for seq in (s for s in cs.SEQUENCES if s["group"] == group):
        mine = [x for x in lines if x["seq"] == seq["name"]]
        want = expected(seq)
        counts = model_run(seq, mut=())
        assert len(mine) == len(want)
        for x, w, c in zip(mine, want, counts):
            assert x["i"] == w["i"] and x["method"] == w["method"]
            where = f"{seq['name']} step {x['i']} ({x['method']} {w['kw']})"
            if x["method"] in cs.SETTERS:
                continue
            vals = [arrays[f"{index[seq['name']]}/{x['i']}/{k}"] if f"{index[seq['name']]}/{x['i']}/{k}" in arrays.files else None
                    for k in range(x["n"])]
            if x["method"] == "timing":      # how often the context factored: the unmutated restatement of api.hip says
                if int(vals[0][0]) != int(c["res"][1][0][0]):
                    failures.append(f"{where}: {int(vals[0][0])} factorisations since set_train, {int(c['res'][1][0][0])} expected")
                continue
            compared += 1
            if (seq["name"], x["i"]) not in MODEL_ONLY:
                if x["bits"]:
                    bit_equal += 1
                else:
                    failures.append(f"{where}: not bit-equal to a fresh context (status {x['status']}, fresh {x['fresh_status']})")
            ratio, errs = judge(seq, w, w, got=(x["status"], vals))
            if ratio > worst[0]:
                worst = (ratio, where)
            if ratio > 1.0:
                failures.append(f"{where}: {ratio:.3g} bounds off the model: {errs}")
    assert compared > 0
    return failures, (f"{group}: {compared} compared steps, {bit_equal} bit-equal to a fresh context, worst error / bound against the "
                      f"model {worst[0]:.3g} ({worst[1]}); {done['contexts']} contexts, {done['seconds']} s")
