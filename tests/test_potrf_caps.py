"""Which queues gpak_potrf_blocked hands to the plan, and which block kernel a panel takes: gpak_potrf_caps and
gpak_potrf_block_co (gp_ss_ak_amd/csrc/potrf_plan.h), printed by tests/potrf_caps_driver.cpp (plain g++, nothing of HIP on
the include path) and checked without a GPU.

* gpak_potrf_caps never reports a queue the context lacks; with tail_queue_max_np = 0 it is the stream flags themselves
  (the behaviour before the rule existed is that one setting); with a limit, sizes up to it keep the tail queue and larger
  ones lose only that; the struct's default behaves like whichever of the two it is.
* The plan made from those caps has Q_TAIL launches iff the caps say so (and the size has launches in the tail at all)
  and keeps the invariants of tests/test_potrf_plan.py.
* gpak_potrf_block_co: never the 8-wave build for a panel that runs beside a bulk launch with two or more workgroups per
  compute unit; potrf_co 0 and 2 override everything.
"""
import os
import subprocess

import pytest

from test_potrf_plan import DEFAULTS, FIELDS, Q_NONE, Q_TAIL, ROOT, CSRC, check_invariants

NPS = [128 * k for k in range(1, 513, 8)]
CU = 256   # compute units of an MI355X


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("potrf_caps") / "potrf_caps_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "potrf_caps_driver.cpp"), "-o", exe])
    return exe


def caps_and_plans(exe, max_np, bw=512):
    """(default of tail_queue_max_np, {(Np, have_tail, have_bulk, have_side): (caps, plan)})."""
    out = subprocess.check_output([exe, "caps", ",".join(str(n) for n in NPS), str(bw), str(max_np)]).decode().splitlines()
    assert out[0].startswith("default ")
    default, res, cur = int(out[0].split()[1]), {}, None
    for ln in out[1:]:
        t = ln.split()
        if t[0] == "Np":
            v = [int(x) for x in t[1:]]
            cur = []
            res[tuple(v[:4])] = (dict(tail_queue=v[4], bulk_queue=v[5], side_stream=v[6]), cur)
        else:
            cur.append(dict(zip(FIELDS, (int(x) for x in t))))
    assert len(res) == 8 * len(NPS)
    return default, res


def check(res, limit):
    for (Np, ht, hb, hs), (caps, plan) in res.items():
        # never a queue the context lacks; the bulk queue and the side stream are passed through
        assert caps["tail_queue"] <= ht and caps["bulk_queue"] == hb and caps["side_stream"] == hs
        # the tail queue: kept up to the limit, withheld above it, 0 = no limit
        assert caps["tail_queue"] == int(bool(ht and (limit == 0 or Np <= limit))), (Np, limit)
        # the plan uses the tail queue iff the caps have it (the default schedule has look-ahead on; sizes of at most
        # two panels have no bulk update at all)
        has_bulk = any(s["bulk"] != Q_NONE for s in plan)
        on_tail = any(s["bulk"] == Q_TAIL for s in plan)
        assert on_tail == bool(caps["tail_queue"] and has_bulk), (Np, caps)
        if on_tail:
            assert [s["bulk"] for s in plan if s["bulk"] != Q_NONE][-1] == Q_TAIL    # the tail is the end
        check_invariants(Np, plan, DEFAULTS, caps, 512)


def test_no_limit_is_the_stream_flags(driver):
    _, res = caps_and_plans(driver, 0)
    for (Np, ht, hb, hs), (caps, _) in res.items():
        assert caps == dict(tail_queue=ht, bulk_queue=hb, side_stream=hs)
    check(res, 0)


@pytest.mark.parametrize("limit", [1, 8192, 16384, 24576, 65536, 1 << 30])
def test_sizes_above_the_limit_lose_only_the_tail_queue(driver, limit):
    _, res = caps_and_plans(driver, limit)
    check(res, limit)
    _, ref = caps_and_plans(driver, 0)
    for key, (caps, plan) in res.items():
        Np, ht, hb, hs = key
        # up to the limit nothing changes; above it the plan is the one of a context without that queue
        assert plan == ref[key if Np <= limit else (Np, 0, hb, hs)][1]


def test_struct_default(driver):
    default, res = caps_and_plans(driver, -1)
    assert default >= 0
    check(res, default)


@pytest.mark.parametrize("surplus", [0, 6, 100])
def test_block_kernel_by_load(driver, surplus):
    rows = [[int(x) for x in ln.split()]
            for ln in subprocess.check_output([driver, "co", str(CU), str(surplus)]).decode().splitlines()]
    assert len(rows) == 3 * 2 * 65
    seen_8w_beside = False
    for potrf_co, beside, mt, wg, co in rows:
        tiles = mt * (mt + 1) // 2
        assert tiles <= wg <= tiles * (100 + surplus) // 100 + 8       # the launcher's grid: tiles plus the surplus, rounded up per XCD
        if potrf_co == 0:
            assert co == 0
        elif potrf_co == 2:
            assert co == 1
        elif not beside:
            assert co == 0                                             # nothing runs beside the panel
        else:
            if wg >= 2 * CU:
                assert co == 1                                         # the chip is full: only the 4-wave build fits
            seen_8w_beside |= co == 0
    assert seen_8w_beside                                              # the last panels do get the 8-wave build
