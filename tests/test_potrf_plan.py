"""The schedule of the single-GPU blocked Cholesky as data: gpak_potrf_plan (gp_ss_ak_amd/csrc/potrf_plan.h), printed by
tests/potrf_plan_driver.cpp -- built here with plain g++ and nothing of HIP on the include path, which is also the proof
that the header is HIP-free -- and checked without a GPU against

* the panel tiers / bulk launches of the sizes the project quotes (46 bulk launches at N = 32768 is what
  profiles/r03_* and VERDICT.md record),
* `loop_model` below: the decisions of the loop gpak_potrf_blocked consisted of before the plan existed, re-stated in
  Python line by line (local variable names kept), for every Np = 128 k, k = 1..64, crossed with the schedule cases of
  test_tuning_environment_matrix (tests/test_gpu_parity.py) and with the optional queues present / absent,
* invariants any schedule must keep.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp_ss_ak_amd", "csrc")
PB, PANEL_MID = 128, 512
NEXT_NONE, NEXT_PANEL, NEXT_SPLIT, NEXT_DONE = range(4)
Q_NONE, Q_MAIN, Q_BULK, Q_TAIL = range(4)
FIELDS = ("J", "W", "J2", "tail_panel", "beside_bulk", "next", "bulk", "ticket", "inv_begin", "inv_end")

# GpakSchedule's defaults (the fields gpak_potrf_plan reads)
DEFAULTS = dict(nb_outer=512, nb_wide=1024, nb_wide_rows=16384, nb_xwide=2048, nb_xwide_rows=32768, first_narrow=1,
                tail_rows=12288, sub_next=0, next_split_rows=0, inv512=1, bwd_fused=2, lookahead=1, fwd_in_factor=1)
ALL_QUEUES = dict(tail_queue=1, bulk_queue=1, side_stream=1)

# the cases of test_tuning_environment_matrix that touch the schedule (the others only select kernels), under the
# environment names they are written with there
MATRIX = [
    {},
    {"GPAK_NB_XWIDE": "1024", "GPAK_NB_XWIDE_ROWS": "3000", "GPAK_NB_WIDE": "768", "GPAK_NB_WIDE_ROWS": "1500", "GPAK_NB_OUTER": "256"},
    {"GPAK_NB_XWIDE": "0", "GPAK_NB_WIDE": "0", "GPAK_TAIL_ROWS": "100000"},
    {"GPAK_BWD_BLOCK": "1024", "GPAK_BWD_FUSED": "2"}, {"GPAK_BWD_BLOCK": "2048", "GPAK_BWD_FUSED": "1"},
    {"GPAK_BWD_BLOCK": "1024", "GPAK_BWD_FUSED": "0"}, {"GPAK_INV512": "0"},
    {"GPAK_NEXT_SPLIT_ROWS": "100000"}, {"GPAK_SUB_NEXT": "1", "GPAK_TAIL_ROWS": "100000"},
    {"GPAK_NEXT_SPLIT_ROWS": "100000", "GPAK_SUB_NEXT": "1", "GPAK_NB_OUTER": "384"},
    {"GPAK_POTRF_CO": "2", "GPAK_LOOKAHEAD": "0"},
    {"GPAK_FWD_IN_FACTOR": "0"}, {"GPAK_TAIL_MASK": "0", "GPAK_BULK_QUEUE": "0"},
]


def from_env(case):
    """(schedule fields, queues, bwd_bw) the library derives from such an environment: gpak_create makes the tail queue
    unless GPAK_TAIL_MASK is 0 and the bulk queue unless GPAK_BULK_QUEUE is 0, gpak_set_train takes the block width."""
    sched, caps, bw = dict(DEFAULTS), dict(ALL_QUEUES), 512
    for k, v in case.items():
        name = k[len("GPAK_"):].lower()
        if name in sched:
            sched[name] = int(v)
        elif name == "tail_mask":
            caps["tail_queue"] = int(int(v) > 0)
        elif name == "bulk_queue":
            caps["bulk_queue"] = int(int(v) != 0)
        elif name == "bwd_block":
            bw = int(v)
        else:
            assert name == "potrf_co", k      # which block kernel a panel takes: not part of the plan
    return sched, caps, bw


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("potrf_plan") / "potrf_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "potrf_plan_driver.cpp"), "-o", exe])

    def run(nps, sched=DEFAULTS, caps=ALL_QUEUES, bw=512):
        args = [exe, ",".join(str(n) for n in nps), str(bw), str(caps["tail_queue"]), str(caps["bulk_queue"]),
                str(caps["side_stream"])] + [f"{k}={v}" for k, v in sched.items()]
        plans = {}
        for ln in subprocess.check_output(args).decode().splitlines():
            if ln.startswith("Np "):
                cur = plans.setdefault(int(ln.split()[1]), [])
            else:
                cur.append(dict(zip(FIELDS, (int(t) for t in ln.split()))))
        assert sorted(plans) == sorted(nps)
        return plans
    return run


def loop_model(Np, t, caps, bw):
    """What the loop of gpak_potrf_blocked decided, panel by panel, before gpak_potrf_plan took the decisions over."""
    lookahead, stream_x = t["lookahead"], caps["side_stream"]
    stream_tail, stream_bulk = caps["tail_queue"], caps["bulk_queue"]
    NB = max(t["nb_outer"], PB) // PB * PB
    nb_wide, nb_xwide = t["nb_wide"] // PB * PB, t["nb_xwide"] // PB * PB
    Js, J = [], 0
    while J < Np:
        Js.append(J)
        first = t["first_narrow"] and J == 0
        if nb_xwide > NB and nb_xwide > nb_wide and Np - J > t["nb_xwide_rows"] and not first:
            J += nb_xwide
        elif nb_wide > NB and Np - J > t["nb_wide_rows"] and not first:
            J += nb_wide
        else:
            J += NB
    nJ = len(Js)
    Js.append(Np)
    next_split_rows = t["next_split_rows"] if stream_x and lookahead else 0
    steps, done512, tl, next_col_done = [], 0, 0, False
    for b in range(nJ):
        J, W = Js[b], Js[b + 1] - Js[b]
        J1 = J + W
        s = dict(J=J, W=W, J2=Js[b + 2] if J1 < Np else Np, tail_panel=0, beside_bulk=0, next=NEXT_NONE, bulk=Q_NONE,
                 ticket=-1, inv_begin=done512, inv_end=done512)
        steps.append(s)
        tail_step = bool(t["sub_next"] and lookahead and stream_x and W <= 512 and J1 < Np and Np - J1 <= t["tail_rows"])
        if tail_step:
            s["tail_panel"] = 1
            next_col_done = True
        else:
            s["beside_bulk"] = int(bool(lookahead and b > 0 and not (stream_tail and Np - (J + W) <= t["tail_rows"])))
            next_col_done = False
        if t["fwd_in_factor"]:
            while t["inv512"] and done512 * bw < Np and min(Np, (done512 + 1) * bw) <= J + W:
                done512 += 1
            s["inv_end"] = done512
        if J1 >= Np:
            break
        J2 = Js[b + 2]
        if next_col_done:
            s["next"] = NEXT_DONE
        elif next_split_rows > 0 and Np - J1 <= next_split_rows and J2 - J1 > PB and J2 - J1 <= PANEL_MID:
            s["next"] = NEXT_SPLIT
        else:
            s["next"] = NEXT_PANEL
        if J2 < Np:
            s["bulk"] = (Q_TAIL if stream_tail and lookahead and Np - J2 <= t["tail_rows"]
                         else Q_BULK if stream_bulk and lookahead else Q_MAIN)
            s["ticket"] = tl
            tl += 1
    return steps


def run_lengths(ws):
    return [(w, len(list(g))) for w, g in itertools.groupby(ws)]


@pytest.mark.parametrize("Np,widths,panels,bulk,on_tail", [
    (1408, [(512, 2), (384, 1)], 3, 1, 1),                                    # N = 1300
    (5120, [(512, 10)], 10, 8, 8),                                            # N = 5000
    (8192, [(512, 16)], 16, 14, 14),
    (32768, [(512, 1), (1024, 16), (512, 31)], 48, 46, 24),
    (65536, [(512, 1), (2048, 16), (1024, 16), (512, 31)], 64, 62, 24),
    (131072, [(512, 1), (2048, 48), (1024, 16), (512, 31)], 96, 94, 24),
])
def test_default_plan_of_the_quoted_sizes(driver, Np, widths, panels, bulk, on_tail):
    plan = driver([Np])[Np]
    assert run_lengths([s["W"] for s in plan]) == widths
    assert len(plan) == panels
    assert sum(s["bulk"] != Q_NONE for s in plan) == bulk
    assert sum(s["bulk"] == Q_TAIL for s in plan) == on_tail
    assert plan == loop_model(Np, DEFAULTS, ALL_QUEUES, 512)


def test_three_tiers_inside_5000_rows(driver):
    """The first tier case of test_tuning_environment_matrix."""
    sched, caps, bw = from_env(MATRIX[1])
    plan = driver([5120], sched, caps, bw)[5120]
    assert run_lengths([s["W"] for s in plan]) == [(256, 1), (1024, 2), (768, 2), (256, 5)]


def check_invariants(Np, plan, sched, caps, bw):
    la = sched["lookahead"]
    # panels tile [0, Np) exactly, in multiples of 128
    J = 0
    for i, s in enumerate(plan):
        assert s["J"] == J and s["W"] > 0 and s["W"] % PB == 0
        J += s["W"]
        assert s["J2"] == (J + plan[i + 1]["W"] if i + 1 < len(plan) else Np)
    assert J == Np
    assert not plan[0]["beside_bulk"]
    ticket = 0
    due = []
    for i, s in enumerate(plan):
        J1, last = s["J"] + s["W"], i == len(plan) - 1
        if not la:
            assert not s["beside_bulk"]
        assert not (s["tail_panel"] and s["beside_bulk"])
        # the next block column: none after the last panel, exactly one way otherwise
        assert (s["next"] == NEXT_NONE) == last
        assert (s["next"] == NEXT_DONE) == bool(s["tail_panel"])
        # nothing on the side stream when it is absent or look-ahead is off
        if not (la and caps["side_stream"]):
            assert not s["tail_panel"] and s["next"] in (NEXT_NONE, NEXT_PANEL)
        # the split needs columns beyond the first 128 and never follows a tail panel
        if s["next"] == NEXT_SPLIT:
            assert PB < s["J2"] - J1 <= PANEL_MID and not s["tail_panel"]
        # bulk updates: only where columns are left beyond the next panel, tickets 0, 1, 2, ... in order
        assert (s["bulk"] != Q_NONE) == (s["J2"] < Np)
        if s["bulk"] != Q_NONE:
            assert s["ticket"] == ticket
            ticket += 1
        else:
            assert s["ticket"] == -1
        if s["bulk"] == Q_TAIL:
            assert la and caps["tail_queue"]
        if s["bulk"] == Q_BULK:
            assert la and caps["bulk_queue"]
        # diagonal inverses: contiguous ranges, never before the panel that completes the block
        assert s["inv_begin"] == (plan[i - 1]["inv_end"] if i else 0) and s["inv_end"] >= s["inv_begin"]
        for k in range(s["inv_begin"], s["inv_end"]):
            assert min(Np, (k + 1) * bw) <= J1
            due.append(k)
    # ... and each exactly once -- or none at all
    if sched["fwd_in_factor"] and sched["inv512"]:
        assert due == list(range((Np + bw - 1) // bw))
    else:
        assert due == []


def test_plan_equals_the_former_loop_and_keeps_the_invariants(driver):
    nps = [PB * k for k in range(1, 65)]
    n = 0
    for case in MATRIX:
        sched, caps, bw = from_env(case)
        # as the library would run the case, and with each optional queue taken away
        for drop in (None, "tail_queue", "bulk_queue", "side_stream"):
            c = dict(caps)
            if drop:
                c[drop] = 0
            plans = driver(nps, sched, c, bw)
            for Np in nps:
                assert plans[Np] == loop_model(Np, sched, c, bw), (Np, case, c)
                check_invariants(Np, plans[Np], sched, c, bw)
                n += 1
    assert n == 64 * len(MATRIX) * 4
