"""TEST INFRASTRUCTURE: runs the sequences of one group of tests/ctx_sequences.py on libgpak_hip.so in THIS process.

    python tests/ctx_seq_worker.py --group {memo,gram,walk,...} --out FILE.npz
    python tests/ctx_seq_worker.py --group {f-cv,f-scratch,...} --out FILE.npz                      (cs.FEATURE_SEQUENCES)
    python tests/ctx_seq_worker.py --group {g-count,g-late2,...} --ranks P --out FILE.npz          (groups of up to P ranks on device 0)
    python tests/ctx_seq_worker.py --group {g-count,...} --ranks P --engine numpy --out FILE.npz   (no GPU: see below)

Every step's result is compared bit for bit with a fresh context's here (the fresh answers are cached by state, so a group
makes tens of contexts); one JSON line per step goes to stdout (sequence, index, method, status, fresh status, bits), and
the arrays themselves into FILE.npz under "<sequence index>/<step>/<k>" for the comparison with the model, which the
test does on the CPU.  The last line holds the number of contexts made and the wall time of the group.

--ranks P: the sequences of cs.GROUP_SEQUENCES, each context a gpak_create_multi group (gpak.Gpak(devices=[0] * ranks)), a
fresh answer from a fresh group of the same rank count.  Every fresh answer is asked of TWO fresh groups; `fresh_twice` says
whether they agree bit for bit (whether a group's answers repeat from one fresh group to the next is measured, not assumed).

--engine numpy: the same group sequences, cut down to what a group answers without device replicas (cs.engine_sequence),
on gpak_create_multi_with_engines over tests/np_dist_engine.py: the group's own host code -- the flags of csrc/multi.hip and
csrc/dist.hip -- on a machine without a GPU.  Every group has P ranks and is closed while the interpreter lives (the engines
are Python callbacks).

Exit status 0: every step RAN (whether it agreed is in its line).  A call that fails in any way the header does not list
as an answer (GPAK_EHIP: a HIP failure, GPAK_ENOMEM, a setter refused or accepted against the sequence) ends the process AT ONCE
with status 2 and the library's message on stderr: no context is closed, no further step, sequence or fresh context is started.
"""
import argparse
import json
import sys
import time

import numpy as np

import ctx_sequences as cs


def engine_group(P):
    """A group of P ranks over NumPy engines, with the face of gpak.Gpak (as tests/san_worker.py builds it)."""
    import ctypes as C
    from gp_ss_ak_amd import dist as gd, gpak
    from np_dist_engine import NumpyDistEngine
    lib = gd._load()
    lib.gpak_create_multi_with_engines.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.POINTER(gd.Engine))]
    engines = [NumpyDistEngine() for _ in range(P)]
    arr = (C.POINTER(gd.Engine) * P)(*[C.pointer(e.table) for e in engines])
    h = C.c_void_p()
    rc = lib.gpak_create_multi_with_engines(C.byref(h), P, arr)
    if rc != 0:
        raise RuntimeError(f"gpak_create_multi_with_engines: status {rc}: {lib.gpak_global_error()}")
    g = gpak.Gpak.__new__(gpak.Gpak)
    g._lib, g._h, g.N, g.d = lib, h, 0, 0
    g._engines = (engines, arr)          # the callbacks live as long as the group
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=cs.GROUPS + list(cs.WORKER_GROUPS) + cs.FEATURE_GROUPS, required=True)
    ap.add_argument("--ranks", type=int, default=0)
    ap.add_argument("--engine", choices=["hip", "numpy"], default="hip")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    made = [0]
    if a.engine == "numpy":
        assert a.ranks >= 2

        def make(precision, ranks):
            assert precision == cs.F64 and ranks == a.ranks
            made[0] += 1
            return engine_group(ranks)
        sequences = [(si, cs.engine_sequence(s, a.ranks)) for si, s in enumerate(cs.GROUP_SEQUENCES) if s["group"] == a.group]
        sequences = [(si, s) for si, s in sequences if s is not None]
    else:
        from gp_ss_ak_amd import gpak

        def make(precision, ranks=1):
            made[0] += 1
            return gpak.Gpak(0, precision) if ranks == 1 else gpak.Gpak(devices=[0] * ranks, precision=precision)
        if a.ranks:
            assert a.group in cs.WORKER_GROUPS and a.ranks == cs.WORKER_GROUPS[a.group], "--ranks is the group's largest rank count"
        pool = cs.GROUP_SEQUENCES if a.ranks else cs.FEATURE_SEQUENCES if a.group in cs.FEATURE_GROUPS else cs.SEQUENCES
        sequences = [(si, s) for si, s in enumerate(pool) if s["group"] == a.group]
    assert sequences, "nothing to run"

    t0 = time.time()
    arrays, fresh_cache, second = {}, {}, {}
    for si, seq in sequences:
        for rec in cs.run(seq, make, make, fresh_cache):
            st, vals = rec["res"]
            for k, v in enumerate(vals):
                if v is not None:
                    arrays[f"{si}/{rec['i']}/{k}"] = v
            fr = rec["fresh"]
            line = dict(seq=seq["name"], i=rec["i"], method=rec["method"], status=st, n=len(vals),
                        fresh_status=None if fr is None else fr[0], bits=None if fr is None else bool(cs.same_bits(rec["res"], fr)))
            if fr is not None and a.ranks and a.engine == "hip":
                fk = (rec["track"], rec["method"], cs.arg_key(rec["kw"]))
                if fk not in second:      # the same question to a second fresh group
                    again = cs.fresh_answer(make, rec["tracker"], rec["method"], rec["kw"], rec["n_train"])
                    second[fk] = bool(cs.same_bits(fr, again))
                    if not second[fk]:
                        for k, v in enumerate(again[1]):
                            if v is not None:
                                arrays[f"{si}/{rec['i']}/again{k}"] = v
                        for k, v in enumerate(fr[1]):
                            if v is not None:
                                arrays[f"{si}/{rec['i']}/fresh{k}"] = v
                line["fresh_twice"] = second[fk]
            print(json.dumps(line), flush=True)
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
