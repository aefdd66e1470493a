"""The failure paths of the built-in RCCL transport (csrc/dist.hip: core_init_rccl, shared by gpak_dist_init_rccl and
gpak_grid_init_rccl) without a GPU and without RCCL: tests/rccl_standin.cpp, built here with plain g++, stands in for
librccl (GPAK_RCCL_LIB), and every case runs in a child process of its own (tests/rccl_standin_child.py) because the
binding is process-wide.

* a rendezvous that does not complete ends after GPAK_RCCL_INIT_TIMEOUT_S with an error that names it, for the 1-D rank
  and for the grid rank alike;
* a failed ncclCommSplit gives every communicator made so far back and leaves the handle with none, so that a second
  call starts again from the rendezvous and cannot report success with the row / column groups missing.
"""
import json
import os
import subprocess
import sys

import pytest

from gp_ss_ak_amd import gpak

HERE = os.path.dirname(os.path.abspath(__file__))
SLEEP_S = 6


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    d = tmp_path_factory.mktemp("rccl_standin")
    libs = {}
    for name, flags in (("full", []), ("no_abort", ["-DSTANDIN_NO_ABORT"])):
        libs[name] = str(d / f"librccl_standin_{name}.so")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", *flags,
                               os.path.join(HERE, "rccl_standin.cpp"), "-o", libs[name], "-lpthread"])

    def run(kind, calls, env, lib="full"):
        log = str(d / f"log_{len(os.listdir(d))}.txt")
        penv = dict(os.environ, GPAK_RCCL_LIB=libs[lib], STANDIN_LOG=log, **env)
        penv.pop("GPAK_RCCL_DISABLE", None)
        out = subprocess.run([sys.executable, os.path.join(HERE, "rccl_standin_child.py"), kind, str(calls)], env=penv,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text[-3000:]
        events = [ln.split() for ln in open(log)] if os.path.exists(log) else []
        return json.loads([ln for ln in text.splitlines() if ln.startswith("[")][-1]), events
    return run


@pytest.mark.parametrize("kind", ["grid", "dist"])
def test_rendezvous_that_does_not_complete_times_out(standin, kind):
    (r,), events = standin(kind, 1, {"STANDIN_INIT_SLEEP_S": str(SLEEP_S), "GPAK_RCCL_INIT_TIMEOUT_S": "1"})
    assert r["rc"] == gpak.EHIP
    assert 0.9 <= r["seconds"] < SLEEP_S - 1, r
    assert "rendezvous" in r["error"] and "ncclCommInitRank" in r["error"]
    assert events == []                       # the call returned while the stand-in was still asleep


@pytest.mark.parametrize("fail_at,lib", [(1, "full"), (2, "full"), (2, "no_abort")])
def test_failed_split_releases_everything_and_the_next_call_starts_again(standin, fail_at, lib):
    calls, events = standin("grid", 2, {"STANDIN_SPLIT_FAIL": str(fail_at)}, lib)
    release = "abort" if lib == "full" else "destroy"    # aborted where the library can, destroyed otherwise
    per_call = fail_at + 2 + (fail_at - 1)
    assert len(events) == 2 * per_call                   # ... and nothing was left for gpak_grid_destroy to release
    worlds = []
    for r, ev in zip(calls, (events[:per_call], events[per_call:])):
        # neither call reports success: the second one does not find a world communicator left behind, it goes
        # through the rendezvous again and meets the same failing split
        assert r["rc"] == gpak.EHIP and "ncclCommSplit" in r["error"]
        # the world communicator, fail_at - 1 good splits, the failing one, then every communicator made so far given
        # back, the groups before the world they were split from
        assert ev[0][0] == "init"
        world = ev[0][1]
        assert [e[:2] for e in ev[1:fail_at]] == [["split", world]] * (fail_at - 1)
        made = [e[2] for e in ev[1:fail_at]]
        assert ev[fail_at] == ["split-failed", world]
        assert ev[fail_at + 1:] == [[release, c] for c in made] + [[release, world]]
        worlds.append(world)
    assert worlds[0] != worlds[1]
