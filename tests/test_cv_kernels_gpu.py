"""GPU tests (-m gpu) of every kernel of the cross-validation code alone, through include/gpak_dev_cv_kernels.h: the Gram, solve
and mix kernels of the batched groups, the stage kernels of a one-at-a-time fold and the leave-one-out kernels, each held
to the long-double reference of its own operation (tests/cv_kernels_ref.py, where every bound is derived and pinned on the
CPU by tests/test_cv_kernels.py).

One worker process per family (tests/cv_kernels_worker.py), five in all, each under its own timeout.  The first worker
that faults, aborts, is killed or runs out of time stops the rest: no further GPU process is started (the rule of
tests/test_ctx_sequences.py).  Every record of a worker asserts
  (a) the payload within its elementwise bound of the reference: every ratio <= 1;
  (b) everything the header calls untouched bit for bit: inputs, guard bands, skew rows, unlisted rows and columns, lists;
  (c) the same bytes from a second call on fresh copies;
and (d), that the bounds bite, is computed on the CPU (tests/test_cv_kernels.py).
"""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_kernels_ref as kr  # noqa: E402
import cv_kernels_worker as worker  # noqa: E402
import dev_ops_cases as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 240
# records per family: what a worker that stopped early or skipped a shape would not deliver
RECORDS = {"gram": 1 + len(kr.GRAM_SIZES), "solve": 1 + len(kr.GRAM_SIZES), "mix": 1 + len(kr.MIX_WIDTHS), "fold": 11 * len(kr.FOLD_M),
           "loo": 12 + 6}

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not dc.long_double_ok(), reason="numpy's long double is no wider than double here")]

_DEVICE_TROUBLE = []       # set by the first worker that faulted, aborted, was killed or timed out: no further GPU process


def records(family):
    if _DEVICE_TROUBLE:
        pytest.fail(f"not started: {_DEVICE_TROUBLE[0]}")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cv_kernels_worker.py"), family], cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"the worker of family {family} did not finish in {TIMEOUT} s")
        pytest.fail(_DEVICE_TROUBLE[0])
    err = r.stderr.decode()
    if r.returncode < 0 or r.returncode in (134, 139) or "HIP error" in err or "hipError" in err:
        _DEVICE_TROUBLE.append(f"the worker of family {family} ended with status {r.returncode}: {err[-1500:]}")
        pytest.fail(_DEVICE_TROUBLE[0])
    assert r.returncode == 0, err[-3000:]
    return [json.loads(line) for line in r.stdout.decode().splitlines() if line.startswith("{")]


@pytest.mark.parametrize("family", worker.FAMILIES)
def test_cv_kernels_alone(family):
    recs = records(family)
    names = [rec["name"] for rec in recs]
    assert len(names) == len(set(names)) == RECORDS[family], names
    assert {rec["kernel"] for rec in recs} == set(worker.ENTRIES[family])
    worst, failed = {}, []
    for rec in recs:
        for k, v in rec["ratios"].items():
            worst[rec["kernel"]] = max(worst.get(rec["kernel"], 0.0), v)
            if not v <= 1.0:
                failed.append((rec["name"], k, v))
        failed += [(rec["name"], k, v) for k, v in rec["flags"].items() if v is not True]
    print("\nworst error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    for rec in recs:
        print(rec["name"], {k: float(f"{v:.3g}") for k, v in rec["ratios"].items()})
    assert not failed, failed
