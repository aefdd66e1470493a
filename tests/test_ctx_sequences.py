"""One long-lived context against fresh ones across call orders (tests/ctx_sequences.py, tests/ctx_model.py).

CPU (-m "not gpu"): every sequence runs on ModelGpak and, step for step equal, on the unmutated CachingModel; each named
mutation of the context's validity logic is caught by a named sequence; any two distinct states of a sequence give model
answers at least 1000 bounds apart, so that an answer from the wrong state cannot hide inside a bound; every function
include/gpak.h declares is called somewhere.

GPU (-m gpu): one fresh process per group (tests/ctx_seq_worker.py).  Every step of the long-lived context is (a)
bit-equal to a fresh context's answer (four steps excepted: MODEL_ONLY says why) and (b) within the method's existing bound of
the model; the count of factorisations (gpak_timing) is that of the unmutated CachingModel.  Figures per group:
DESIGN.md section 8, "Call sequences on one context".

Groups (gpak_create_multi; second half of the module): the same on cs.GROUP_SEQUENCES with GroupCaching; on the CPU also
the group's own host code over NumPy engines in a worker process; on the GPU one worker per worker group, which asks every
fresh question of two fresh groups.  DESIGN.md section 8, "Call sequences on a multi-GPU context".

Feature calls (last part of the module): the same three halves on cs.FEATURE_SEQUENCES -- models, FEATURE_MUTATIONS, separation,
coverage of the ten feature headers on the CPU; test_feature_sequences_on_the_device on the GPU -- and `g feature refusals` among
the group sequences.  DESIGN.md section 8, "Call sequences across the feature calls".
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
# declared in include/gpak.h and out of this module's scope: the calibration microbenchmarks, the process-wide tuning reload,
# the error text before a context exists
EXCLUDED = {"gpak_calibrate", "gpak_reload_tuning", "gpak_global_error"}
# Steps held to the model alone, (sequence, step) -> why their bits legitimately depend on earlier calls.
# How a context substitutes backwards is settled when it FACTORS (CtxState::factorisation_succeeded, csrc/ctx_state.h, takes
# the options the factor was built under: the explicit 512-block inverses and the [R ; T] stacks are built beside the
# factorisation's forward substitution only), so GPAK_OPT_INV512 / GPAK_OPT_BWD_FUSED changed afterwards take effect at the
# next factorisation.  Until then the long-lived context keeps the back substitution
# of the options it factored under while a fresh context, given the current options, uses another: the same alpha and
# solve_chol in another summation order (measured: they differ in the last bits, and are equal again after gpak_set_params).
_BACKSOLVE = "options of the back substitution changed since the factorisation"
MODEL_ONLY = {("solve scratch", 11): _BACKSOLVE, ("solve scratch", 12): _BACKSOLVE, ("solve scratch", 15): _BACKSOLVE,
              ("solve scratch", 16): _BACKSOLVE}


def model_run(seq, mut=None):
    if mut is None:
        make = lambda p, r=1: cm.ModelGpak(p, CACHE, r)                                                        # noqa: E731
    else:      # a mutation belongs to one of the two restatements: the other kind of context of the sequence runs unmutated
        single = [m for m in mut if m in cm.MUTATIONS + cm.FEATURE_MUTATIONS + cm.FEATURE_REDUNDANT]
        make = lambda p, r=1: cm.CachingModel(p, CACHE, single) if r == 1 else cm.GroupCaching(p, CACHE, r, [m for m in mut if m not in single])  # noqa: E731
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
    assert cols == [0, 1, 1, 1, cs.BAD200_COLUMN, 0]           # the columns themselves: the last failure is past the first tile


# mutation -> (the named sequence that catches it, index and method of its first step off the model).  That step is the
# first one after the call whose invalidation was dropped that reads what the call should have invalidated: the very next
# step everywhere but for `gram keeps factor` (gram at 5; solve_alpha at 6 returns the alpha the context still rightly holds;
# the variance at 7 reads the matrix buffer), `predict leaks pooled mean` (prediction at 7; loo and compute_k do not read the
# training points' transformed copy, the Gram matrix at 10 does) and `recovery keeps failed_column` (good parameters at 36,
# the factorisation at 37, the question at 38: the column it keeps is 200, the failure before it, not 1).
CAUGHT_BY = {
    "memo ignores composition": ("memo", 6, "logLikelihood"),
    "gram keeps factor": ("gram between [direct]", 7, "posteriorMeanVar"),
    "set_train keeps alpha": ("size walk", 19, "posteriorMeanVar"),
    "set_kernel keeps U": ("gradients", 9, "GradLL_hyb"),
    "failed factor keeps alpha": ("fail and recover", 13, "logLikelihood"),
    "solve_chol keeps z": ("solve scratch", 4, "solve_alpha"),
    "predict leaks pooled mean": ("gram between [expansion]", 10, "gram"),
    "f32 image kept": ("f32", 5, "posteriorMeanVar"),
    "recovery keeps failed_column": ("fail and recover", 38, "failed_column"),
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
    if mutation == "recovery keeps failed_column":       # the value kept is the column of the LAST failure, which is not 1
        assert dropped[0][1] == cs.BAD200_COLUMN and int(rec["res"][1][0][0]) == cs.BAD200_COLUMN
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
    separation(cs.BY_NAME[name], single_state=("out of order",))


def separation(seq, single_state):
    name = seq["name"]
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
    if name not in single_state:
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


def test_a_setter_accepted_where_a_refusal_was_due_ends_the_run():
    """cs.refused: the status must be exactly the one the step names; a refused setter is not noted, an accepted one ends the run."""
    class FiveColumns(cm.ModelGpak):
        def set_train(self, X, y):
            self.X, self.y, (self.N, self.d), self.tkey = X, y, X.shape, "five"      # accepts what it must refuse
    seq = dict(name="refusal", group="refusal", precision=cs.F64,
               steps=[cs.S("set_train", train="T129"), cs.no("set_train", cs.ENOTIMPL, train="T129x5"), cs.S("failed_column")])
    recs = list(cs.run(seq, lambda p: cm.ModelGpak(p, CACHE)))
    assert [r["res"][0] for r in recs] == [cs.OK, cs.ENOTIMPL, cs.OK] and recs[2]["train"] == "T129" and not cs.DEVICE_ERROR
    try:
        with pytest.raises(RuntimeError):
            list(cs.run(seq, lambda p: FiveColumns(p, CACHE)))
        assert cs.DEVICE_ERROR
        with pytest.raises(RuntimeError):      # another refusal than the one that was due
            list(cs.run(dict(seq, steps=[cs.no("set_train", cs.EINVAL, train="T129x5")]), lambda p: cm.ModelGpak(p, CACHE)))
    finally:
        del cs.DEVICE_ERROR[:], cs.LEAKED[:]


def test_every_declared_function_is_called_in_some_sequence():
    called = set(cs.ALWAYS)
    for seq in cs.SEQUENCES:
        called |= {cs.ENTRY[m] for _c, m, _kw in seq["steps"]}
    # the multi-GPU surface: every group sequence makes its contexts with gpak_create_multi; gpak_loo_grad, which the groups
    # are asked for (and refuse), is declared in include/gpak_loo_grad.h
    assert all(max(np.atleast_1d(s["ranks"])) >= 2 for s in cs.GROUP_SEQUENCES)
    called |= {"gpak_create_multi"} | {cs.ENTRY[m] for s in cs.GROUP_SEQUENCES if not s["name"].startswith("random") for _c, m, _kw in s["steps"]}
    called.discard("gpak_loo_grad")
    called -= set(cs.FEATURE_ENTRY.values())      # `g feature refusals`: declared in the feature headers (test_the_feature_sequences_cover_...)
    declared = set(header_functions())
    assert EXCLUDED <= declared
    missing = declared - called - EXCLUDED
    assert not missing, sorted(missing)
    assert called <= declared, sorted(called - declared)
    named = {cs.ENTRY[m] for s in cs.SEQUENCES if s["group"] != "random" for _c, m, _kw in s["steps"]}
    named |= {"gpak_create_multi", "gpak_n_gpus", "gpak_transport"} & called
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


def _sequences_on_the_device(group, tmp_path, sequences):
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
    failures, summary = judge_group(group, lines, np.load(out), sequences)
    print(summary)
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("group", cs.GROUPS)
def test_sequences_on_the_device(group, tmp_path):
    _sequences_on_the_device(group, tmp_path, cs.SEQUENCES)


def judge_group(group, lines, arrays, sequences=cs.SEQUENCES):
    """The worker's records and arrays of one group against fresh contexts (a) and the model (b): (failures, summary)."""
    done = lines.pop()
    assert done["done"] == group
    failures, bit_equal, compared, worst = [], 0, 0, (0.0, None)
    index = {s["name"]: k for k, s in enumerate(sequences)}
    for seq in (s for s in sequences if s["group"] == group):
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
            if (seq["name"], x["i"]) not in MODEL_ONLY and (seq["name"], x["i"]) not in FEATURE_MODEL_ONLY:
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


# ======== groups (gpak_create_multi): DESIGN.md section 8, "Call sequences on a multi-GPU context" ============================
GROUP_NAMES = [s["name"] for s in cs.GROUP_SEQUENCES]


def counts_of(seq):
    """evaluations at each `timing` step as the unmutated restatements of multi.hip / api.hip count them"""
    return {c["i"]: int(c["res"][1][0][0]) for c in model_run(seq, mut=()) if c["method"] == "timing"}


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_group_sequence_on_the_models(name):
    seq = cs.GROUP_BY_NAME[name]
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
    print(f"{name}: {len(want)} steps, {counted} compared, statuses {sorted({w['res'][0] for w in want})}, counts {counts_of(seq)}")


def test_the_group_sequences_meet_what_the_issue_names():
    seen = {}
    for seq in cs.GROUP_SEQUENCES:
        for w in expected(seq):
            seen.setdefault(w["res"][0], set()).add((seq["name"], w["method"]))
    assert {("refusals (group)", m) for m in cs.REFUSED_ON_A_GROUP} <= seen[cs.ENOTIMPL]
    assert ("compositions (group)", "GradLL") in seen[cs.ENOTIMPL] and ("compositions (group)", "GradLL_hyb") in seen[cs.EINVAL]
    assert ("size walk (group) [P=2]", "posteriorMeanVar") in seen[cs.EINVAL]
    assert {("out of order (group)", m) for m in ("logLikelihood", "gram", "posteriorMeanVar", "solve_chol", "chol_upper")} <= seen[cs.ESTATE]
    assert {("fail and recover (group)", m) for m in ("posteriorMeanVar", "solve_chol", "chol_upper", "GradLL")} <= seen[cs.ENOTPD]
    fail = expected(cs.GROUP_BY_NAME["fail and recover (group)"])
    assert sum(1 for w in fail if w["method"] == "logLikelihood" and np.isnan(w["res"][1][0]).all()) == 4
    cols = [int(w["res"][1][0][0]) for w in fail if w["method"] == "failed_column"]
    assert cols == [0, 1, 1, cs.BAD200_COLUMN, 0]
    # the counts the hazards are about: they restart at the new set's first factorisation; a failing ask counts every time;
    # gram, compute_k, the imports and the refused calls count for nothing
    assert list(counts_of(cs.GROUP_BY_NAME["group count"]).values()) == [1, 1, 1, 1, 2, 2, 0, 1, 2, 2, 3]
    assert list(counts_of(cs.GROUP_BY_NAME["fail and recover (group)"]).values()) == [2, 3, 10, 11, 12, 13]   # seven more failing asks between the second and the third timing
    assert set(counts_of(cs.GROUP_BY_NAME["refusals (group)"]).values()) == {1}
    assert list(counts_of(cs.GROUP_BY_NAME["gram between (group) [direct]"]).values()) == [2, 2, 2]
    methods = {m for s in cs.GROUP_SEQUENCES if not s["name"].startswith("random") for _c, m, _kw in s["steps"]}
    assert {"logLikelihood", "nlz_terms", "solve_alpha", "solve_chol", "chol_upper", "gram", "compute_k", "posteriorMeanVar", "GradLL",
            "GradLL_hyb", "factor", "failed_column", "timing", "n_gpus", "transport"} | set(cs.REFUSED_ON_A_GROUP) <= methods
    assert [s["steps"] for s in cs.GROUP_SEQUENCES if s["name"].startswith("random")] == [cs.seq_g_random(k) for k in range(2)]
    assert {(cs.TRAIN[s["steps"][0][2]["train"]][0], s["ranks"]) for s in cs.GROUP_SEQUENCES if s["name"].startswith("random")} == {(129, 2), (300, 3)}


# mutation -> (named sequence, index and method of the first step off the model, what is off there).  "count": the step is a
# `timing` whose evaluations differ from the unmutated restatement's (the answers themselves are right: the ranks factor
# whenever THEIR flag says so); "answer": the step's status or numbers.
GROUP_CAUGHT_BY = {
    "set_train keeps factor_current": ("group count", 8, "timing", "count"),          # fault 1 of the issue
    "set_train keeps count": ("group count", 8, "timing", "count"),
    "set_params keeps factor_current": ("group count", 13, "timing", "count"),
    "set_params keeps have_result": ("group count", 12, "GradLL", "answer"),
    "set_train keeps replica train": ("late replicas [P=2]", 7, "posteriorMeanVar", "answer"),
    "set_params keeps replica params": ("late replicas [P=2]", 4, "posteriorMeanVar", "answer"),
    "gram keeps replica factor": ("gram between (group) [direct]", 14, "posteriorMeanVar", "answer"),
    "set_params keeps general_kernel": ("compositions (group)", 8, "GradLL", "answer"),
    "recovery keeps failed_column": ("fail and recover (group)", 28, "failed_column", "answer"),
    "import keeps f32 image": ("f32 (group)", 4, "posteriorMeanVar", "answer"),
}
# A mutation that changes only WHERE something is computed gives the same values and the same count on the models.  `gram
# keeps replica factor` is one wherever the next reader of the factor goes through the replica's own ensure_factor: at
# ("gram between (group) [direct]", 11) gpak_solve_chol follows gpak_gram directly, the replica would factor for itself (N^3 / 3
# flops on one device instead of an import) and answer with the bits of ITS factorisation, which the bit comparison of the
# GPU run holds against a fresh group's imported factor; on the models nothing shows there.  (The prediction at step 14 follows a
# gpak_gram directly and reads the matrix buffer without ensure_factor: there the same mutation changes the variance, which is why
# the table above catches it.  At the first gpak_gram, step 6, replica 0 has imported nothing yet: there is no flag to keep.)
WHERE_ONLY = {"gram keeps replica factor": ("gram between (group) [direct]", 11, "solve_chol")}


def group_divergence(seq, mut):
    """First step of seq on the mutated GroupCaching that is off: (record, 'answer' or 'count', detail, dropped)."""
    want, counts = expected(seq), counts_of(seq)
    made = []

    def make(p, r=1):
        made.append(cm.GroupCaching(p, CACHE, r, mut) if r > 1 else cm.CachingModel(p, CACHE))
        return made[-1]

    it = cs.run(seq, make)
    dropped = lambda: [d for g in made for d in g.dropped]    # noqa: E731
    for w, rec in zip(want, it):
        if rec["method"] in cs.SETTERS:
            continue
        if rec["method"] == "timing":
            got = int(rec["res"][1][0][0])
            if got != counts[rec["i"]]:
                it.close()
                return rec, "count", (got, counts[rec["i"]]), dropped()
            continue
        ratio, errs = judge(seq, rec, w)
        if ratio > 1.0:
            it.close()
            return rec, "answer", ratio, dropped()
    return None, None, None, dropped()


@pytest.mark.parametrize("mutation", cm.GROUP_MUTATIONS)
def test_each_group_mutation_is_caught(mutation):
    name, index, method, how = GROUP_CAUGHT_BY[mutation]
    rec, what, detail, dropped = group_divergence(cs.GROUP_BY_NAME[name], [mutation])
    assert rec is not None, f"{mutation}: the sequence '{name}' runs on the mutated model without a difference"
    print(f"{mutation}: '{name}' step {rec['i']} ({rec['method']} {rec['kw']}): {what} {detail}")
    assert dropped and all(d[0] == mutation for d in dropped)
    assert (rec["i"], rec["method"], what) == (index, method, how), (rec["i"], rec["method"], what)
    if mutation == "recovery keeps failed_column":       # the column it keeps is the last failure's, which is not 1
        assert int(rec["res"][1][0][0]) == cs.BAD200_COLUMN


@pytest.mark.parametrize("mutation", cm.GROUP_REDUNDANT)
def test_a_reset_that_another_reset_covers_changes_nothing(mutation):
    """Listed, not dropped: these resets of multi.hip are covered by replica_train_ok / replica_params_ok (ensure_replica clears
    replica_factor_ok whenever it sets parameters again), so no sequence can tell whether they are there."""
    hit = 0
    for seq in cs.GROUP_SEQUENCES:
        rec, what, detail, dropped = group_divergence(seq, [mutation])
        assert rec is None, (mutation, seq["name"], rec["i"], rec["method"], what, detail)
        hit += len(dropped)
    assert hit > 0          # the mutation did take effect somewhere


def test_the_group_mutation_tables_are_the_models():
    assert set(GROUP_CAUGHT_BY) == set(cm.GROUP_MUTATIONS) and len(cm.GROUP_MUTATIONS) == 10 and len(cm.GROUP_REDUNDANT) == 2
    named = {s["name"] for s in cs.GROUP_SEQUENCES if not s["name"].startswith("random")}
    assert {v[0] for v in GROUP_CAUGHT_BY.values()} <= named and {v[0] for v in WHERE_ONLY.values()} <= named
    for mutation, (name, index, method) in WHERE_ONLY.items():
        steps = cs.GROUP_BY_NAME[name]["steps"]
        assert steps[index][1] == method and steps[index - 1][1] == "gram" and mutation in cm.GROUP_MUTATIONS
        rec, what, _detail, dropped = group_divergence(dict(cs.GROUP_BY_NAME[name], name=name + " without step 14", steps=steps[:14] + steps[15:]),
                                                         [mutation])
        assert dropped and rec is None          # without the prediction of step 14 the models see nothing anywhere


# sequences whose group goes through one state only (or none): nothing to separate
ONE_STATE = ("refusals (group)", "out of order (group)", "g feature refusals")


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_distinct_group_states_are_a_thousand_bounds_apart(name):
    """test_distinct_states_are_a_thousand_bounds_apart for the group sequences."""
    separation(cs.GROUP_BY_NAME[name], single_state=ONE_STATE)


# ---- the group's own host code on the CPU: gpak_create_multi_with_engines over tests/np_dist_engine.py ---------------------------
def judge_worker(seqs, lines, arrays, group, model_only=()):
    """The worker's records and arrays against fresh groups (a), the model (b) and the restatement's counts (c):
    (failures, [(where, both fresh values) for questions two fresh groups answer differently], summary)."""
    done = lines.pop()
    assert done["done"] == group
    failures, unrepeatable, bit_equal, compared, worst = [], [], 0, 0, (0.0, None)
    for si, seq in seqs:
        mine = [x for x in lines if x["seq"] == seq["name"]]
        want, counts = expected(seq), counts_of(seq)
        assert len(mine) == len(want) == len(seq["steps"])
        for x, w in zip(mine, want):
            assert x["i"] == w["i"] and x["method"] == w["method"]
            where = f"{seq['name']} step {x['i']} ({x['method']} {w['kw']})"
            if x["method"] in cs.SETTERS:
                continue
            vals = [arrays[f"{si}/{x['i']}/{k}"] if f"{si}/{x['i']}/{k}" in arrays.files else None for k in range(x["n"])]
            if x["method"] == "timing":
                if int(vals[0][0]) != counts[x["i"]]:
                    failures.append(f"{where}: {int(vals[0][0])} evaluations since set_train, {counts[x['i']]} expected")
                continue
            compared += 1
            if x.get("fresh_twice") is False:
                both = {k: arrays[k] for k in arrays.files if k.startswith(f"{si}/{x['i']}/fresh") or k.startswith(f"{si}/{x['i']}/again")}
                unrepeatable.append((where, both))
            if (seq["name"], x["i"]) not in model_only:
                if x["bits"]:
                    bit_equal += 1
                else:
                    failures.append(f"{where}: not bit-equal to a fresh group (status {x['status']}, fresh {x['fresh_status']})")
            ratio, errs = judge(seq, w, w, got=(x["status"], vals))
            if ratio > worst[0]:
                worst = (ratio, where)
            if ratio > 1.0:
                failures.append(f"{where}: {ratio:.3g} bounds off the model: {errs}")
    assert compared > 0
    return failures, unrepeatable, (f"{group}: {compared} compared steps, {bit_equal} bit-equal to a fresh group, worst error / bound against "
                                    f"the model {worst[0]:.3g} ({worst[1]}); {done['contexts']} contexts, {done['seconds']} s")


def _run_worker(args, out, timeout):
    return subprocess.run([sys.executable, os.path.join(HERE, "ctx_seq_worker.py")] + args + ["--out", out], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT, OPENBLAS_NUM_THREADS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout)


ENGINE_RANKS = (2, 3)
ENGINE_RUNS = [(g, p) for p in ENGINE_RANKS for g in cs.WORKER_GROUPS
               if any(cs.engine_sequence(s, p) for s in cs.GROUP_SEQUENCES if s["group"] == g)]


@pytest.mark.parametrize("group,ranks", ENGINE_RUNS)
def test_group_sequences_on_the_host_code_over_numpy_engines(group, ranks, tmp_path):
    """multi.hip and dist.hip themselves, on the CPU: every step bit-equal to a fresh engine group, within the method's bound of
    the model, the evaluations those of GroupCaching.  Shows fault 1 of the issue (the lost count) without a GPU."""
    out = str(tmp_path / "results.npz")
    r = _run_worker(["--group", group, "--ranks", str(ranks), "--engine", "numpy"], out, 600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
    seqs = [(si, cs.engine_sequence(s, ranks)) for si, s in enumerate(cs.GROUP_SEQUENCES) if s["group"] == group]
    seqs = [(si, dict(s, name=s["name"])) for si, s in seqs if s is not None]
    for _si, s in seqs:                       # the model's run of the cut-down sequence, under a name of its own
        _MODEL_RUNS.pop(s["name"], None)
    try:
        failures, _unrep, summary = judge_worker(seqs, lines, np.load(out), group)
    finally:
        for _si, s in seqs:
            _MODEL_RUNS.pop(s["name"], None)
    print(f"P={ranks} {summary}")
    assert not failures, "\n".join(failures)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
# Steps of a group sequence held to the model and the count alone because two FRESH groups were measured to answer the
# question with different bits: (sequence, step) -> the measurement.  No other ground exempts a step.
GROUP_MODEL_ONLY = {}
_GROUP_RUNS = {}


def _group_run(group, tmp_path):
    """One worker process per worker group, run once and shared by the two tests below."""
    if group not in _GROUP_RUNS:
        if _DEVICE_TROUBLE:
            pytest.fail(f"not started: {_DEVICE_TROUBLE[0]}")
        out = str(tmp_path / "results.npz")
        try:
            r = _run_worker(["--group", group, "--ranks", str(cs.WORKER_GROUPS[group])], out, TIMEOUT)
        except subprocess.TimeoutExpired:
            _DEVICE_TROUBLE.append(f"the worker of group {group} did not finish in {TIMEOUT} s")
            pytest.fail(_DEVICE_TROUBLE[0])
        err = r.stderr.decode()
        if r.returncode != 0 or "HIP error" in err or "hipError" in err or "illegal memory access" in err:
            _DEVICE_TROUBLE.append(f"the worker of group {group} ended with status {r.returncode}: {err[-1500:]}")
            pytest.fail(_DEVICE_TROUBLE[0])
        lines = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
        seqs = [(si, s) for si, s in enumerate(cs.GROUP_SEQUENCES) if s["group"] == group]
        _GROUP_RUNS[group] = judge_worker(seqs, lines, np.load(out), group, GROUP_MODEL_ONLY)
    return _GROUP_RUNS[group]


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(cs.WORKER_GROUPS))
def test_two_fresh_groups_answer_with_the_same_bits(group, tmp_path):
    """The premise of (a): each compared question, asked of two fresh groups of the same rank count and precision."""
    _failures, unrepeatable, _summary = _group_run(group, tmp_path)
    exempt = [u for u in unrepeatable if any(u[0].startswith(f"{n} step {i} ") for n, i in GROUP_MODEL_ONLY)]
    for where, both in unrepeatable:
        print(where, {k: v.ravel()[:4] for k, v in both.items()})
    assert len(exempt) == len(unrepeatable), [u[0] for u in unrepeatable]


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(cs.WORKER_GROUPS))
def test_group_sequences_on_the_device(group, tmp_path):
    """(a) bit-equal to a fresh group, (b) within the method's existing bound of the model, (c) evaluations as GroupCaching
    counts them."""
    failures, _unrepeatable, summary = _group_run(group, tmp_path)
    print(summary)
    assert not failures, "\n".join(failures)


# ======== the feature calls (cs.FEATURE_SEQUENCES): DESIGN.md section 8, "Call sequences across the feature calls" ===============
FEATURE_NAMES = [s["name"] for s in cs.FEATURE_SEQUENCES]
FEATURE_NAMED = [s for s in cs.FEATURE_SEQUENCES if not s["name"].startswith("feature random")]
TWELVE = ("gpak_cv_groups", "gpak_cv_groups_grad", "gpak_cv_folds", "gpak_cv_folds_grad", "gpak_design", "gpak_condition", "gpak_sample_path",
          "gpak_local_metric", "gpak_predict_local", "gpak_predict_local_ok", "gpak_local_neighbours_dev")
# declared in the feature headers and out of scope: the two host searches take no context
FEATURE_EXCLUDED = {"gpak_local_neighbours": "host code, no context", "gpak_local_neighbours_octant": "host code, no context"}
# (sequence, step) -> why the step's bits legitimately depend on earlier calls (a code line, never a failure)
FEATURE_MODEL_ONLY = {}


@pytest.mark.parametrize("name", FEATURE_NAMES)
def test_feature_sequence_on_the_models(name):
    seq = cs.FEATURE_BY_NAME[name]
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
    print(f"{name}: {len(want)} steps, {counted} compared, statuses {sorted({w['res'][0] for w in want})}")


def test_the_feature_sequences_meet_the_statuses_the_headers_promise():
    seen = {}
    for seq in FEATURE_NAMED:
        for w in expected(seq):
            seen.setdefault(w["res"][0], set()).add((seq["name"], w["method"]))
    factor_calls = set(cm.FEATURE_FACTOR_CALLS) | {"loo_grad"}
    assert {("feature fail and recover", m) for m in factor_calls} <= seen[cs.ENOTPD]
    assert {("feature refused", m) for m in factor_calls} <= seen[cs.ESTATE]
    # the local calls: no parameters (GPAK_ESTATE), a column count other than the training set's (GPAK_ENOTIMPL), k = 129 (GPAK_EINVAL)
    assert {("feature refused", m) for m in ("local_metric", "predict_local", "predict_local_ok")} <= seen[cs.ESTATE]
    assert {("feature refused", m) for m in ("predict_local", "predict_local_ok")} <= seen[cs.ENOTIMPL]
    assert ("feature refused", "local_neighbours_dev") in seen[cs.EINVAL]
    refused = expected(cs.FEATURE_BY_NAME["feature refused"])
    for m in cs.FEATURE_ENTRY:                     # every one of the eleven is refused somewhere, and answers somewhere after it
        at = [w["i"] for w in refused if w["method"] == m and w["res"][0] != cs.OK]
        assert at and any(w["res"][0] == cs.OK and w["i"] > at[0] and w["method"] not in cs.SETTERS + ("timing",) for w in refused), m
    assert [w["res"][0] for w in refused if w["method"] == "local_neighbours_dev"] == [cs.EINVAL, cs.EINVAL, cs.OK, cs.OK]
    assert {("feature refused", m) for m in ("cv_groups", "cv_groups_grad", "cv_folds_grad", "loo_grad", "design", "condition", "sample_path")} <= seen[cs.EINVAL]
    assert {("feature refused", m) for m in ("cv_groups_grad", "cv_folds_grad", "loo_grad")} <= seen[cs.ENOTIMPL]
    fail = expected(cs.FEATURE_BY_NAME["feature fail and recover"])
    for w in fail:                                 # quiet NaN in every floating-point output of a failed call
        if w["res"][0] == cs.ENOTPD:
            nan = [np.isnan(v).all() for v in w["res"][1]]
            assert sum(nan) >= len(nan) - 2, (w["i"], w["method"])          # design: picked and the counts; the others: the counts
    assert [int(w["res"][1][0][0]) for w in fail if w["method"] == "failed_column"] == [1, cs.BAD200_COLUMN, 0]
    # at the column-200 failure too, every factor-dependent call
    late = [w["method"] for w in fail if w["res"][0] == cs.ENOTPD and w["kern"][1] == "BAD200"]
    assert set(late) == factor_calls and len(late) == 8
    # the counts the device run is held to: a failing ask factors (and counts) every time, a refusal and a local call never;
    # every named sequence carries them
    assert [int(c["res"][1][0][0]) for c in model_run(cs.FEATURE_BY_NAME["feature fail and recover"], mut=()) if c["method"] == "timing"] == [9, 17, 18]
    assert all(any(m == "timing" for _c, m, _kw in s["steps"]) for s in FEATURE_NAMED)
    assert sum(m == "timing" for s in cs.FEATURE_SEQUENCES for _c, m, _kw in s["steps"]) >= 25
    # the local calls that need no factor answer at the failing parameters, with numbers
    assert all(w["res"][0] == cs.OK and np.isfinite(w["res"][1][0]).all() for w in fail if w["method"] in ("local_metric", "local_neighbours_dev"))
    # nothing is factored for a refusal
    counts = [int(c["res"][1][0][0]) for c in model_run(cs.FEATURE_BY_NAME["feature refused"], mut=()) if c["method"] == "timing"]
    assert counts == [1, 1, 1, 2, 1], counts


# mutation -> (the named feature sequence that catches it, index and method of its first step off the model): the call itself,
# as the first reader of a factor after new parameters or a new training set
FEATURE_CAUGHT_BY = {
    "cv_groups answers from the factor as it stands": ("cv workspace", 2, "cv_groups"),
    "cv_groups_grad answers from the factor as it stands": ("feature fail and recover", 5, "cv_groups_grad"),
    "cv_folds answers from the factor as it stands": ("feature two contexts", 4, "cv_folds"),
    "cv_folds_grad answers from the factor as it stands": ("feature fail and recover", 7, "cv_folds_grad"),
    "design answers from the factor as it stands": ("scratch", 2, "design"),
    "condition answers from the factor as it stands": ("simulation", 2, "condition"),
    "sample_path answers from the factor as it stands": ("feature fail and recover", 11, "sample_path"),
    # the design at 6 (the condition at 9); logLikelihood after it reads the factor, which stands; the Gram matrix two steps on is
    # the first thing built from U again, as for `predict leaks pooled mean`
    "design leaks pooled mean": ("feature prediction buffers [expansion]", 8, "gram"),
    "condition leaks pooled mean": ("feature prediction buffers [expansion]", 11, "gram"),
}


def test_the_feature_mutation_table_is_the_models():
    assert set(FEATURE_CAUGHT_BY) == set(cm.FEATURE_MUTATIONS) and len(cm.FEATURE_MUTATIONS) == 9 and cm.FEATURE_REDUNDANT == ("condition keeps z",)
    assert {v[0] for v in FEATURE_CAUGHT_BY.values()} <= {s["name"] for s in FEATURE_NAMED}
    assert not set(cm.FEATURE_MUTATIONS) & set(cm.MUTATIONS) and len(cm.MUTATIONS) == 9


@pytest.mark.parametrize("mutation", cm.FEATURE_MUTATIONS)
def test_each_feature_mutation_is_caught(mutation):
    name, index, method = FEATURE_CAUGHT_BY[mutation]
    seq = cs.FEATURE_BY_NAME[name]
    rec, ratio, dropped = first_divergence(seq, [mutation])
    assert rec is not None, f"{mutation}: the sequence '{name}' runs on the mutated model without a difference"
    print(f"{mutation}: '{name}' step {rec['i']} ({rec['method']} {rec['kw']}) is {ratio:.3g} bounds off the model")
    assert dropped and all(d[0] == mutation for d in dropped)
    assert (rec["i"], rec["method"]) == (index, method), (rec["i"], rec["method"])


@pytest.mark.parametrize("mutation", cm.FEATURE_REDUNDANT)
def test_a_feature_reset_that_another_covers_changes_nothing(mutation):
    """gpak_condition's work_vectors_overwritten follows ensure_nlz, whose back substitution has consumed L^-1 y / sn2 and lowered
    the flag already: no sequence can tell whether the event is raised."""
    hit = 0
    for seq in cs.FEATURE_SEQUENCES:
        rec, _ratio, dropped = first_divergence(seq, [mutation])
        assert rec is None, (mutation, seq["name"], rec["i"], rec["method"])
        hit += len(dropped)
    assert hit > 0


# sequences whose contexts with a training set go through one state only
FEATURE_ONE_STATE = ()


@pytest.mark.parametrize("name", FEATURE_NAMES)
def test_distinct_feature_states_are_a_thousand_bounds_apart(name):
    """test_distinct_states_are_a_thousand_bounds_apart for the feature sequences."""
    separation(cs.FEATURE_BY_NAME[name], single_state=FEATURE_ONE_STATE)


def test_sizing_the_binding_before_a_training_set_is_undone_and_guarded():
    """cs._sized lends Gpak.N the size the no-training-set data was made for (the binding checks labels and realisations against N
    before the library can answer GPAK_ESTATE; tests/lgo_grad_model.py does the same): only on a binding object without a
    training set, undone after the call, also when the call raises; a model is left alone."""
    from gp_ss_ak_amd import gpak
    b = gpak.Gpak.__new__(gpak.Gpak)               # the binding's own class without a device, as Gpak.__init__ leaves it
    b._h, b.N = None, 0
    with cs._sized(b, 0, 300):
        assert b.N == 300
    assert b.N == 0
    with pytest.raises(RuntimeError):
        with cs._sized(b, 0, 300):
            raise RuntimeError("refused")
    assert b.N == 0
    with cs._sized(b, 129, 129):                   # with a training set: nothing to lend
        assert b.N == 0
    b.N = 129
    with pytest.raises(AssertionError):            # a stale size would be hidden
        with cs._sized(b, 0, 300):
            pass
    m = cm.ModelGpak()
    with cs._sized(m, 0, 300):
        assert m.N == 0


def test_every_pick_of_a_design_is_decided_beyond_its_bound():
    """`picked` is compared for equality: in every state a sequence asks a design in, the gain a pick was taken by leads the
    runner-up by more than 1000 times the bound on a gain (1e-8 prior variance sum of weights), or the two are the same hole
    twice (the tie of layout "twins", which the header gives to the smaller number)."""
    asked = 0
    for seq in cs.FEATURE_SEQUENCES:
        for w in expected(seq):
            if w["method"] != "design" or w["res"][0] != cs.OK:
                continue
            m = cs.model_at(w, CACHE, seq["precision"])
            Xt, nd, Xc, hole, wt, k = cs.design_args(w["kw"]["design"])
            gain, _picked, _pg, ex = m.design(Xt, nd, Xc, hole, wt, k, True)
            for gap in ex["gaps"]:
                assert gap == 0.0 or gap * float(np.nanmax(gain)) > SEPARATION * 1e-8 * m.prior_variance() * ex["weight_sum"], (seq["name"], w["i"], gap)
            asked += 1
    assert asked >= 10


def test_the_feature_sequences_cover_the_feature_headers():
    assert [s["steps"] for s in cs.FEATURE_SEQUENCES if s["name"].startswith("feature random")] == \
        [cs.seq_feature_random(k) for k in range(cs.FEATURE_RANDOM_COUNT)]
    assert cs.FEATURE_RANDOM_COUNT == 3 and all(len(cs.seq_feature_random(k)) == 30 for k in range(3))
    random_methods = {m for s in cs.FEATURE_SEQUENCES if s["name"].startswith("feature random") for _c, m, _kw in s["steps"]}
    assert set(cs.FEATURE_ENTRY) | {"loo_grad"} <= random_methods, sorted(set(cs.FEATURE_ENTRY) - random_methods)
    assert len(random_methods - set(cs.FEATURE_ENTRY) - set(cs.SETTERS)) >= 8          # and the old vocabulary
    named = {cs.ENTRY[m] for s in FEATURE_NAMED for _c, m, _kw in s["steps"]}
    assert set(TWELVE) | {"gpak_loo_grad"} <= named, sorted(set(TWELVE) - named)
    declared = set()
    for h in cs.FEATURE_HEADERS:
        declared |= set(header_functions(h))
    assert set(FEATURE_EXCLUDED) <= declared
    missing = declared - named - set(FEATURE_EXCLUDED)
    assert not missing, sorted(missing)
    assert set(cs.FEATURE_ENTRY.values()) | {"gpak_loo_grad"} == declared - set(FEATURE_EXCLUDED)
    # both forms of the calls that have two
    kws = [(m, kw) for s in FEATURE_NAMED for _c, m, kw in s["steps"]]
    assert any(m == "cv_folds" and kw.get("no_batch") for m, kw in kws) and any(m == "cv_folds_grad" and kw.get("no_batch") for m, kw in kws)
    assert any(m == "condition" and kw.get("unfused") for m, kw in kws) and any(m == "condition" and kw.get("fsim") is False for m, kw in kws)
    assert {kw["S"] for m, kw in kws if m == "condition"} == {3, 130} and {kw["prior"] for m, kw in kws if m == "sample_path"} == {"F96", "F1100"}
    assert {kw["k"] for m, kw in kws if m == "local_neighbours_dev"} == {17, 128, 129}          # 129: the refusal


@pytest.mark.gpu
@pytest.mark.parametrize("group", cs.FEATURE_GROUPS)
def test_feature_sequences_on_the_device(group, tmp_path):
    """One fresh process per group; every non-setter step (a) bit-equal to a fresh context and (b) within the bound of the model;
    the count of factorisations that of the unmutated CachingModel.  Shares _DEVICE_TROUBLE with the groups above."""
    _sequences_on_the_device(group, tmp_path, cs.FEATURE_SEQUENCES)


def test_a_group_refuses_every_feature_call():
    """`g feature refusals`: GPAK_ENOTIMPL from each of the eleven calls of the feature headers that take a context (gpak_loo_grad:
    `refusals (group)`), one factorisation over the whole sequence, and the NumPy-engine run asks none of them."""
    seq = cs.GROUP_BY_NAME["g feature refusals"]
    want = expected(seq)
    refused = {w["method"] for w in want if w["res"][0] == cs.ENOTIMPL}
    assert refused == set(cs.FEATURE_ENTRY) and len(refused) == 11
    assert all(w["res"][0] == cs.OK for w in want if w["method"] not in cs.FEATURE_ENTRY)
    assert set(counts_of(seq).values()) == {1}
    cut = cs.engine_sequence(seq, 2)
    assert cut is not None and not {m for _c, m, _kw in cut["steps"]} & set(cs.FEATURE_ENTRY)
