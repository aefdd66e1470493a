"""TEST INFRASTRUCTURE: runs one group of tests/dev_ops_cases.py on one engine in THIS process and prints one JSON
line per case (name, worst error / bound ratio, elements written that must not be, guard bands, return codes, whether
two runs agreed bit for bit, and the measured float64-vs-long-double ratios that set the substitution tolerances).

    python tests/dev_ops_worker.py --engine {hip,numpy} --group {gemm,solve_rows,trsv,reduce,fill,grad,pairs,panel,f32}

Exit status 0: every case RAN (whether it passed is in its line); 3: no usable long double on this host.
"""
import argparse
import json
import sys

import dev_ops_cases as dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", choices=("hip", "numpy"), required=True)
    ap.add_argument("--group", choices=dc.GROUPS, required=True, nargs="+", help="one group, or several to run in turn")
    a = ap.parse_args()
    if not dc.long_double_ok():
        print(json.dumps({"skip": "np.longdouble is no wider than float64 on this host"}), flush=True)
        return 3
    ops = dc.HipOps() if a.engine == "hip" else dc.numpy_ops()
    for group in a.group:
        n = 0
        for rec in dc.run_group(ops, group):
            print(json.dumps(dict(rec, group=group)), flush=True)
            n += 1
        print(json.dumps({"done": group, "engine": a.engine, "cases": n}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
