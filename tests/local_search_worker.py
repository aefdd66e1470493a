"""TEST INFRASTRUCTURE: gpak_dev_local_search (include/gpak_dev_local_search.h) alone on caller-owned device buffers, in a
process of its own (torch holds the buffers, and its HIP runtime must come up before the library's).  The grids are built
by tests/local_search_ref.py for chosen cell sizes, not by the library; the outputs sit between guard words.  One JSON
record per (inputs, grid, k, radius) on stdout: every comparison is of bytes."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dev_ops_cases as dc  # noqa: E402
import local_ref  # noqa: E402
import local_search_ref as sr  # noqa: E402

OK, EINVAL = 0, 2
GUARD = 64            # guard words on either side of every output
RADIUS = {"random": 0.12, "d4": 0.3}     # the finite radii tests/test_local.py uses on these inputs
CASES = [(i, g, k, r) for i in sr.KERNEL_INPUTS for g in sr.KERNEL_GRIDS for k in sr.KERNEL_K for r in (0.0,)] + \
        [(i, g, 17, RADIUS[i]) for i in sr.KERNEL_INPUTS for g in sr.KERNEL_GRIDS]


def name_of(case):
    return "%s-%s-k%d-r%g" % case


def guarded(eng, n, fill, dtype):
    host = np.full(n + 2 * GUARD, fill, dtype=dtype)
    return host, eng.from_numpy(host)


def run(ops, _cache, inputs, which, k, radius):
    eng, lib = ops.eng, ops.lib
    if (inputs, which) not in _cache:
        _cache.clear()
        _cache[(inputs, which)] = sr.kernel_case(inputs, which)
    Ts, Tc, G, g = _cache[(inputs, which)]
    n, d, nB = Ts.shape[0], Ts.shape[1], Tc.shape[0]
    # the lists of a full sort over the TRANSFORMED points (the identity as G: nothing is transformed twice)
    want, want_used = local_ref.brute_neighbours(Ts, Tc, k, None, radius)
    want_d2 = sr.dist2_lists(Ts, Tc, want)
    operands = {"pts": g["pts"].ravel(), "ids": g["ids"], "start": g["start"], "tc": np.ascontiguousarray(Tc).ravel()}
    dev = {key: eng.from_numpy(v) for key, v in operands.items()}
    h_nbr, d_nbr = guarded(eng, k * nB, -7, np.int32)
    h_used, d_used = guarded(eng, nB, -7, np.int32)
    h_d2, d_d2 = guarded(eng, k * nB, 0.0, np.float64)
    h_d2[...] = dc.sentinel(h_d2.size)
    d_d2 = eng.from_numpy(h_d2)
    d_vis = eng.from_numpy(np.array([5], dtype=np.int64))
    a = {"pts": dev["pts"].data_ptr(), "ids": dev["ids"].data_ptr(), "start": dev["start"].data_ptr(), "n": n, "d": d,
         "lo0": g["lo"][0], "lo1": g["lo"][1], "lo2": g["lo"][2], "h": g["h"], "n0": g["n"][0], "n1": g["n"][1], "n2": g["n"][2],
         "scale": g["scale"], "tc": dev["tc"].data_ptr(), "nB": nB, "k": k, "radius": radius, "nbr": d_nbr.data_ptr() + 4 * GUARD,
         "used": d_used.data_ptr() + 4 * GUARD, "dist2": d_d2.data_ptr() + 8 * GUARD, "visited": d_vis.data_ptr()}

    def launch(**kw):
        b = dict(a)
        b.update(kw)
        return lib.gpak_dev_local_search(eng._st(), *b.values())

    def outputs():
        eng.sync()
        return d_nbr.cpu().numpy(), d_used.cpu().numpy(), d_d2.cpu().numpy(), int(d_vis.cpu().numpy()[0])

    rcs = [launch(**kw) for kw in ({"pts": None}, {"ids": None}, {"start": None}, {"tc": None}, {"nbr": None}, {"n": 0}, {"nB": 0},
                                   {"d": 2}, {"d": 5}, {"k": 0}, {"k": 129}, {"n0": 0}, {"n1": 0}, {"n2": 0}, {"h": 0.0}, {"h": -1.0},
                                   {"h": float("inf")}, {"h": float("nan")}, {"radius": float("nan")})]
    o = outputs()
    rec = {"name": name_of((inputs, which, k, radius)), "refusals": rcs == [EINVAL] * len(rcs),
           "refusals_write_nothing": bool(np.array_equal(o[0], h_nbr) and np.array_equal(o[1], h_used) and
                                          np.array_equal(dc.bits(o[2]), dc.bits(h_d2)) and o[3] == 5)}
    rc = launch()
    nbr, used, d2, vis = outputs()
    body = slice(GUARD, -GUARD)
    got = nbr[body].reshape(nB, k)
    floor = sr.visited_floor(Ts, Tc, want, k, radius)
    rec.update({
        "rc": rc == OK, "centres": nB, "cells": int(g["start"].size - 1),
        "lists": bool(got.tobytes() == want.tobytes()), "used": bool(used[body].tobytes() == want_used.tobytes()),
        "dist2": bool(d2[body].reshape(nB, k).tobytes() == want_d2.tobytes()),
        "wrong_centres": np.flatnonzero((got != want).any(axis=1)).tolist()[:8],
        "visited": vis - 5, "visited_floor": floor, "visited_ceiling": n * nB,
        "guards": bool(np.all(nbr[:GUARD] == -7) and np.all(nbr[-GUARD:] == -7) and np.all(used[:GUARD] == -7) and np.all(used[-GUARD:] == -7)
                       and np.array_equal(dc.bits(d2[:GUARD]), dc.bits(h_d2[:GUARD])) and np.array_equal(dc.bits(d2[-GUARD:]), dc.bits(h_d2[-GUARD:]))),
        "operands_untouched": bool(all(dev[key].cpu().numpy().tobytes() == operands[key].tobytes() for key in operands)),
        "some_list_short": bool(want_used.min() < k)})
    # without the optional outputs: the same lists
    d_nbr2 = eng.from_numpy(h_nbr)
    rc2 = launch(nbr=d_nbr2.data_ptr() + 4 * GUARD, used=None, dist2=None, visited=None)
    eng.sync()
    rec["optional_outputs"] = bool(rc2 == OK and d_nbr2.cpu().numpy().tobytes() == nbr.tobytes())
    return rec


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_local_search
    fn.restype = C.c_int
    vp, i, dbl = C.c_void_p, C.c_int, C.c_double
    fn.argtypes = [vp, vp, vp, vp, i, i, dbl, dbl, dbl, dbl, i, i, i, dbl, vp, i, i, dbl, vp, vp, vp, vp]
    cache = {}
    for case in CASES if len(sys.argv) < 2 else [c for c in CASES if name_of(c) in sys.argv[1:]]:
        print(json.dumps(run(ops, cache, *case)), flush=True)


if __name__ == "__main__":
    main()
