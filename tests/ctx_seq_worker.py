"""TEST INFRASTRUCTURE: runs the sequences of one group of tests/ctx_sequences.py on libgpak_hip.so in THIS process.

    python tests/ctx_seq_worker.py --group {memo,gram,walk,...} --out FILE.npz

Every step's result is compared bit for bit with a fresh context's here (the fresh answers are cached by state, so a group
makes tens of contexts); one JSON line per step goes to stdout (sequence, index, method, status, fresh status, bits), and
the arrays themselves into FILE.npz under "<sequence index>/<step>/<k>" for the comparison with the model, which the
test does on the CPU.  The last line holds the number of contexts made and the wall time of the group.

Exit status 0: every step RAN (whether it agreed is in its line).  A call that fails in any way the header does not list
as an answer (GPAK_EHIP: a HIP failure, GPAK_ENOMEM, a setter refused) ends the process AT ONCE with status 2 and the
library's message on stderr: no context is closed, no further step, sequence or fresh context is started.
"""
import argparse
import json
import sys
import time

import numpy as np

import ctx_sequences as cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=cs.GROUPS, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from gp_ss_ak_amd import gpak
    made = [0]

    def make(precision):
        made[0] += 1
        return gpak.Gpak(0, precision)

    t0 = time.time()
    arrays, fresh_cache = {}, {}
    for si, seq in enumerate(cs.SEQUENCES):
        if seq["group"] != a.group:
            continue
        for rec in cs.run(seq, make, make, fresh_cache):
            st, vals = rec["res"]
            for k, v in enumerate(vals):
                if v is not None:
                    arrays[f"{si}/{rec['i']}/{k}"] = v
            fr = rec["fresh"]
            print(json.dumps(dict(seq=seq["name"], i=rec["i"], method=rec["method"], status=st, n=len(vals),
                                  fresh_status=None if fr is None else fr[0], bits=None if fr is None else bool(cs.same_bits(rec["res"], fr)))),
                  flush=True)
    np.savez(a.out, **arrays)
    print(json.dumps(dict(done=a.group, contexts=made[0], fresh_states=len(fresh_cache), seconds=round(time.time() - t0, 2))), flush=True)
    return 0


if __name__ == "__main__":
    try:
        rc = main()
    except BaseException as e:     # noqa: B036 -- whatever it is, the device is not touched again
        import os
        import traceback
        traceback.print_exc()
        print(f"ctx_seq_worker: stopped: {type(e).__name__}: {e}; {cs.DEVICE_ERROR}", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(2)                # not sys.exit: no destructor may call into the library on the way out
    sys.exit(rc)
