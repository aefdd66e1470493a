#!/usr/bin/env python3
"""Oracle-driven trajectory of the exact-gradient driver (tests/golden/golden_exact_lbfgs_N<k>.json).

What `gp_ss_ak --gradient exact train -o LBFGS` must reproduce on the GPU: tests/exact_grad_ref.projected_lbfgs (the
line-for-line port of Opt_Algs::ProjectedLBFGSOptimise) driven on the host by the oracle's objective (orc_gram with
DIRECT distances + orc_nlz_lean, OpenBLAS LAPACK) and by the NumPy restatement of the exact gradient
(exact_grad_ref.grad_exact on W formed from the same K).  No HIP code takes part.

Per iteration: kept objective, cumulative evaluation count (factorisations), kept point (10 values), the accepted step
of the backtracking (1 = the first trial), all at 17 digits.  Data as make_golden_lbfgs.prepared(N): the CLI sees
bit-identical inputs through its text file.

Run from the repo root:  python tests/golden/make_golden_exact.py 8192 6
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import exact_grad_ref  # noqa: E402
import make_golden_lbfgs  # noqa: E402
from gp_ss_ak_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

IS_ANGLE = [True, False, True, False, True, False, False, False, False, False]


def main(N, maxit):
    assert orc.use_lapack(0), "SciPy's OpenBLAS is part of the image"
    Xs, ys = make_golden_lbfgs.prepared(N)
    x0 = list(synth.DEFAULT_EXPANS) + [synth.DEFAULT_BIAS, synth.DEFAULT_SN2]
    state = {"K": None, "x": None, "n": 0, "t0": time.time()}

    def fun(x):
        K = orc.gram(Xs, Xs, np.array(x[:8], dtype=float), float(x[8]), orc.DIST_DIRECT)
        info, _, _ = orc.nlz_lean(K, ys, float(x[9]), want_L=False)
        state.update(K=K, x=np.array(x))
        state["n"] += 1
        print(f"  eval {state['n']:3d}  nlz {info.nlz:.15g}  ({time.time() - state['t0']:.0f} s)", flush=True)
        return float("nan") if info.chol_fail else info.nlz

    def grad(x):
        assert np.array_equal(state["x"], np.array(x))     # the driver asks at the point it has just evaluated
        W = exact_grad_ref.weights(state["K"], ys, float(x[9]))
        g = exact_grad_ref.grad_exact(Xs, ys, [(0, x[:8])], float(x[8]), float(x[9]), W=W)
        print(f"  grad |g|inf {np.abs(g).max():.6g}  ({time.time() - state['t0']:.0f} s)", flush=True)
        return g

    trace = []
    exact_grad_ref.projected_lbfgs(fun, grad, x0, IS_ANGLE, maxit, trace=trace)
    ev = [1] + [n for _, n, _ in trace]
    out = {"N": N, "maxit": maxit, "x0": [float(v) for v in x0],
           "data": "synth.drillholes(N), extremes set to exactly -1/+1 (make_golden_lbfgs.prepared)",
           "how": "tests/exact_grad_ref.py: projected_lbfgs over orc_gram (DIRECT) + orc_nlz_lean (OpenBLAS LAPACK) and "
                  "grad_exact (NumPy)",
           "rows": [{"iteration": k + 1, "objective": float(h), "evaluations": int(n), "trials": int(n - ev[k]),
                     "x": [float(v) for v in xk]} for k, (h, n, xk) in enumerate(trace)]}
    with open(os.path.join(HERE, f"golden_exact_lbfgs_N{N}.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}),
          [(r["objective"], r["evaluations"]) for r in out["rows"]])


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8192, int(sys.argv[2]) if len(sys.argv) > 2 else 6)
