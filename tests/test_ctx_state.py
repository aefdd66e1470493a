"""CtxState (gp_ss_ak_amd/csrc/ctx_state.h), the C++ struct that holds every validity fact of a single-GPU context, against
its Python restatement tests/ctx_model.py::CachingModel.  No GPU.

tests/ctx_state_driver.cpp includes the header alone and is built with plain g++, nothing of HIP on the include path
(which is the proof that the header is HIP-free).  The unmutated CachingModel runs every sequence of cs.SEQUENCES and logs
the events it passes through; the driver replays them, and after every step its state -- points, rung, z, backsolve,
image, failed_col, factorisations -- must be the model's flags.  Then the comparison is shown to be able to fail: for each
of the nine MUTATIONS the driver, fed the UNMUTATED events, must part from the mutated model's flags at or before the step
at which tests/test_ctx_sequences.py catches that mutation.  The same for cs.FEATURE_SEQUENCES and the FEATURE_MUTATIONS.
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_model as cm  # noqa: E402
import ctx_sequences as cs  # noqa: E402
from test_ctx_sequences import CACHE, CAUGHT_BY, FEATURE_CAUGHT_BY  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp_ss_ak_amd", "csrc")
FRESH = (0, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctx_state") / "ctx_state_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "ctx_state_driver.cpp"),
                           "-o", exe])

    def run(lines):
        """the state after each line"""
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout
        states = [tuple(int(t) for t in ln.split()) for ln in out.splitlines()]
        assert len(states) == len(lines)
        return states
    return run


def trace(seq, mut=()):
    """Per step of the sequence: (context, the events the step raised in it, its flags afterwards)."""
    made, seen, out = [], {}, []

    def make(p):
        made.append(cm.CachingModel(p, CACHE, mut))
        return made[-1]

    for rec in cs.run(seq, make):
        if rec["ctx"] not in seen:
            seen[rec["ctx"]] = [made[-1], 0]               # cs.run makes a context at the first step that names it
        m, n = seen[rec["ctx"]]
        out.append((rec["ctx"], m.events[n:], m.flags()))
        seen[rec["ctx"]][1] = len(m.events)
    assert len(out) == len(seq["steps"]) and len(made) == len(seen)
    return out


def driver_states(replay, steps):
    """The driver's state after each step, from the steps' events: one context after the other, `reset` in between."""
    lines, last = [], {}           # last: step -> index of the line after which the step's context stands
    for c in sorted({c for c, _ev, _fl in steps}):
        lines.append("reset")
        for i, (ci, ev, _fl) in enumerate(steps):
            if ci == c:
                lines += ev
                last[i] = len(lines) - 1
    states = replay(lines)
    assert all(states[k] == FRESH for k, ln in enumerate(lines) if ln == "reset")
    return [states[last[i]] for i in range(len(steps))]


@pytest.mark.parametrize("name", [s["name"] for s in cs.SEQUENCES])
def test_the_struct_is_the_model_step_for_step(replay, name):
    steps = trace(cs.BY_NAME[name])
    got = driver_states(replay, steps)
    for i, ((c, ev, flags), state) in enumerate(zip(steps, got)):
        assert state == flags, (name, i, cs.BY_NAME[name]["steps"][i][1], ev, "driver", state, "model", flags)
    events = [e.split()[0] for _c, ev, _fl in steps for e in ev]
    print(f"{name}: {len(steps)} steps, {len(events)} events of {len(set(events))} kinds")
    assert events


def test_the_sequences_raise_every_event_but_the_import():
    """gpak_import_factor is raised by a group on its replicas only (tests/test_ctx_sequences.py, the group half)."""
    raised = {e.split()[0] for s in cs.SEQUENCES for _c, ev, _fl in trace(s) for e in ev}
    assert raised == {"set_memoise", "new_training_set", "new_kernel", "same_kernel", "points_built", "matrix_overwritten",
                      "factorisation_started", "factorisation_succeeded", "factorisation_failed", "work_vectors_overwritten",
                      "alpha_built", "nlz_built", "image_built"}


def test_an_imported_factor(replay):
    """The one event no sequence raises: the 128-block back substitution only, alpha and the nlZ terms current, failed_col 0,
    no z, no image, the count and the points as they were."""
    s = replay(["new_training_set", "new_kernel", "points_built", "factorisation_started", "factorisation_failed 7",
                "factor_imported", "new_kernel", "factor_imported"])
    assert s[4] == (1, 0, 0, 0, 0, 7, 1) and s[5] == (1, 3, 0, 0, 0, 0, 1) and s[7] == (0, 3, 0, 0, 0, 0, 1)


@pytest.mark.parametrize("mutation", cm.MUTATIONS)
def test_the_comparison_can_fail(replay, mutation):
    name, index, _method = CAUGHT_BY[mutation]
    seq = cs.BY_NAME[name]
    want = driver_states(replay, trace(seq))                  # the struct, fed what the unmutated model passes through
    mutated = trace(seq, [mutation])
    off = [i for i, (state, (_c, _ev, flags)) in enumerate(zip(want, mutated)) if state != flags]
    assert off, f"{mutation}: the mutated model's flags are the struct's over all of '{name}'"
    print(f"{mutation}: '{name}' step {off[0]} ({seq['steps'][off[0]][1]}): struct {want[off[0]]}, mutated model {mutated[off[0]][2]}; "
          f"test_ctx_sequences catches it at step {index}")
    assert off[0] <= index


# ---- the feature calls (cs.FEATURE_SEQUENCES) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s["name"] for s in cs.FEATURE_SEQUENCES])
def test_the_struct_is_the_model_over_the_feature_sequences(replay, name):
    seq = cs.FEATURE_BY_NAME[name]
    steps = trace(seq)
    got = driver_states(replay, steps)
    for i, ((c, ev, flags), state) in enumerate(zip(steps, got)):
        assert state == flags, (name, i, seq["steps"][i][1], ev, "driver", state, "model", flags)
    assert [e for _c, ev, _fl in steps for e in ev]


def test_a_condition_call_raises_work_vectors_overwritten():
    """gpak_condition_impl solves through dWork (csrc/condition.hip): the event follows the call's own bring-up-to-date."""
    seq = cs.FEATURE_BY_NAME["simulation"]
    for (_c, method, _kw), (_ctx, ev, _fl) in zip(seq["steps"], trace(seq)):
        if method in ("condition", "sample_path"):
            assert ev and ev[-1] == "work_vectors_overwritten", (method, ev)


@pytest.mark.parametrize("mutation", cm.FEATURE_MUTATIONS)
def test_the_feature_comparison_can_fail(replay, mutation):
    name, index, _method = FEATURE_CAUGHT_BY[mutation]
    seq = cs.FEATURE_BY_NAME[name]
    want = driver_states(replay, trace(seq))
    mutated = trace(seq, [mutation])
    off = [i for i, (state, (_c, _ev, flags)) in enumerate(zip(want, mutated)) if state != flags]
    assert off, f"{mutation}: the mutated model's flags are the struct's over all of '{name}'"
    print(f"{mutation}: '{name}' step {off[0]} ({seq['steps'][off[0]][1]}): struct {want[off[0]]}, mutated model {mutated[off[0]][2]}; "
          f"test_ctx_sequences catches it at step {index}")
    assert off[0] <= index
