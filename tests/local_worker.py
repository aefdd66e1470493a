"""TEST INFRASTRUCTURE: gpak_dev_local_krige (include/gpak_dev_local.h) alone on caller-owned device buffers, in a process
of its own (torch holds the buffers, and its HIP runtime must come up before the library's).  The points are transformed by
gpak_dev_transform_k, the nodes' point-major; outputs are guarded and sentinel-filled as tests/dev_ops_cases.py's buffers
are.  One JSON record per shape on stdout.

Bound per node (s samples, K = K_II = R R', kb = kbar, y = y_I, u = 2^-53, tau = the project's fill tolerance of the direct
form, relative to kmax = max|K|; first order, 2-norms, n1 = |K^-1|):
  (a) the evaluations: |dK|_F <= s tau kmax;  |dkb| <= sqrt(s) (tau + (nd + 2) u) kmax  (nd values added, one scaling, the bias);
  (b) the Cholesky, R^ R^' = K + E1, |E1|_F <= (s + 1) u |R|_F^2 = (s + 1) u tr K (Higham, Accuracy and Stability, thm 10.3),
      and the two forward substitutions, (R^ + D) z^ = b with |D| <= s u |R^| each (thm 8.5): to first order one more
      perturbation of K of at most 2 s u tr K.  E = (3 s + 1) u tr K in all;
  (c) the two dot products, element j by lane j mod 64 then a butterfly of 6 levels: at most s / 64 + 7 roundings each.
mean = kb' K^-1 y:   |d mean| <= n1 |dkb| |y| + n1^2 |kb| |y| (|dK| + E) + (s / 64 + 7) u n1 |kb| |y|
q = kb' K^-1 kb:     |d q|    <= 2 n1 |dkb| |kb| + n1^2 |kb|^2 (|dK| + E) + (s / 64 + 7) u n1 |kb|^2
kbb: nd^2 evaluations, nd^2 / 64 + 8 roundings: (tau + (nd^2 / 64 + 8) u) kmax;  var = (kbb - q) + add: 2 u |var| more.
The noise is the call's own argument: SN2 = 1 here (as tests/design_worker.py takes noise = 1), so that n1 <= 1 and the
bound stays close to the errors it bounds; the context-level tests run the compositions' own sn2.
"bites": against a reference in which the first two values of y of the largest node were swapped the ratio is beyond 1e3.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dev_ops_cases as dc  # noqa: E402
import design_ref  # noqa: E402
import local_cases as lc  # noqa: E402
import local_ref  # noqa: E402
import test_block_gpu as tb  # noqa: E402

OK, EINVAL = 0, 2
HYB, D4 = 0x20, 0x10
TAU = dc.FILL_TOL[1]
SN2 = 1.0
# (id, Ns, M, nd, k, composition)
SHAPES = [("defaults-k128", 300, 37, 8, 128, "defaults"), ("white-k128", 300, 37, 2, 128, "expans+rbf+bias+white"),
          ("d4-k64", 300, 26, 1, 64, "d4-defaults"), ("rbf-k32", 300, 30, 27, 32, "rbf"), ("exp-k16", 300, 9, 8, 16, "expans+exp")]


def kern_of(comp):
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    plain = len(terms) == 1 and terms[0][0] == 0
    kern = np.array(terms[0][1] if plain else dc.serialise(terms, 0.0), dtype=np.float64)   # kern[4] is not read: white travels alone
    return kern, (0 if plain else HYB) | (D4 if cols == 4 else 0), (1 if plain else len(terms))


def device_inputs(ops, name, Ns, M, nd, k, comp):
    """everything the call reads, on the device: the transformed samples and nodes, ys, the lists"""
    eng, lib = ops.eng, ops.lib
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    Xs, ys = tb.data(Ns, cols)
    Xd = tb.blocks(Ns, cols, M, nd)
    full, _ = local_ref.brute_neighbours(Xs, lc.centres(Xd, nd), k)
    nbr = full.copy()
    sizes = [s for s in lc.S if s <= k] + [0]
    for b in range(M):
        nbr[b, sizes[b % len(sizes)]:] = -1
    kern, mode, nterms = kern_of(comp)
    arrays = 5 * (3 if mode & HYB else 1)
    mu = np.zeros(4)
    mu[:cols] = Xs.mean(axis=0)
    ucap, cap = Ns + 11, M + 5
    raw_s = np.zeros((4, Ns))
    raw_s[:cols] = Xs.T
    raw_n = np.zeros((4, nd * cap))                           # point a of node b at a * cap + b
    for a in range(nd):
        raw_n[:cols, a * cap:a * cap + M] = Xd[a::nd].T
    du, dP = eng.zeros(arrays * ucap), eng.zeros(arrays * nd * cap)
    dxs, dxn = eng.from_numpy(raw_s.ravel()), eng.from_numpy(raw_n.ravel())
    kp, mp = kern.ctypes.data_as(C.POINTER(C.c_double)), mu.ctypes.data_as(C.POINTER(C.c_double))
    st = eng._st()
    assert lib.gpak_dev_transform_k(st, dxs.data_ptr(), Ns, Ns, ucap, kp, mode, mp, du.data_ptr()) == OK
    assert lib.gpak_dev_transform_k(st, dxn.data_ptr(), nd * cap, nd * cap, nd * cap, kp, mode, mp, dP.data_ptr()) == OK
    eng.sync()
    return {"Xs": Xs, "ys": ys, "Xd": Xd, "nbr": nbr, "kern": kern, "mode": mode, "ucap": ucap, "cap": cap, "du": du, "dP": dP,
            "dys": eng.from_numpy(ys), "dnbr": eng.from_numpy(np.ascontiguousarray(nbr, dtype=np.int32).ravel())}


def bounds(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2):
    M = nbr.shape[0]
    bm, bv = np.zeros(M), np.zeros(M)
    u = dc.U
    for b in range(M):
        I = nbr[b][nbr[b] >= 0]
        s = len(I)
        pts = Xd[b * nd:(b + 1) * nd]
        kmax = bias + sum(p[{0: 6, 1: 1, 2: 2}[kd]] ** 2 for kd, p in terms) + sn2 + white
        bkbb = (TAU + (nd * nd / 64 + 8) * u) * kmax
        if s == 0:
            bm[b], bv[b] = 0.0, bkbb + 4 * u * kmax
            continue
        K = design_ref.averaged(Xs[I], Xs[I], 1, 1, terms, bias, float) + (sn2 + white) * np.eye(s)
        kb = design_ref.averaged(Xs[I], pts, 1, nd, terms, bias, float)[:, 0]
        n1 = float(np.linalg.norm(np.linalg.inv(K), 2))
        ny, nk = float(np.linalg.norm(ys[I])), float(np.linalg.norm(kb))
        dK, dkb = s * TAU * kmax, np.sqrt(s) * (TAU + (nd + 2) * u) * kmax
        E = (3 * s + 1) * u * float(np.trace(K))
        dot = (s / 64 + 7) * u
        bm[b] = n1 * dkb * ny + n1 * n1 * nk * ny * (dK + E) + dot * n1 * nk * ny
        bq = 2 * n1 * dkb * nk + n1 * n1 * nk * nk * (dK + E) + dot * n1 * nk * nk
        bv[b] = bq + bkbb + 4 * u * kmax
    return bm, bv


def launch(base, **kw):
    ops, d, nd, M, k, bias, white, noise, flags, mean, var, dinfo = base
    a = {"P": d["dP"].data_ptr(), "cap": d["cap"], "nB": M, "nd": nd, "u": d["du"].data_ptr(), "ucap": d["ucap"], "n": len(d["ys"]),
         "ys": d["dys"].data_ptr(), "kern": d["kern"].ctypes.data_as(C.POINTER(C.c_double)), "bias": bias, "mode": d["mode"],
         "white": white, "noise": noise, "nbr": d["dnbr"].data_ptr(), "k": k, "flags": flags, "mean": mean, "var": var,
         "info": dinfo.data_ptr()}
    a.update(kw)
    return ops.lib.gpak_dev_local_krige(ops.eng._st(), *a.values())


def run(ops, name, Ns, M, nd, k, comp):
    eng = ops.eng
    cols, terms, bias, white, _ = tb.COMPS[comp]
    sn2 = SN2
    d = device_inputs(ops, name, Ns, M, nd, k, comp)
    ref = local_ref.local_predict(d["Xs"], d["ys"], d["Xd"], nd, d["nbr"], terms, bias, white, sn2)
    bm, bv = bounds(d["Xs"], d["ys"], d["Xd"], nd, d["nbr"], terms, bias, white, sn2)
    before = {key: d[key].cpu().numpy().copy() for key in ("du", "dP", "dys", "dnbr")}
    rec = {"name": name, "notpd_in_reference": bool(ref["notpd"].any())}
    outs = []
    for rep, flags in enumerate((0, 0, 1)):                   # the second call: the same bytes; the third: latent
        mean, var = dc.Mat(np.zeros(M)), dc.Mat(np.zeros(M))
        mean.full[...] = dc.sentinel(mean.full.size)
        var.full[...] = dc.sentinel(var.full.size)
        mean.before, var.before = mean.data.copy(), var.data.copy()
        dmean, dvar = eng.from_numpy(mean.full), eng.from_numpy(var.full)
        dinfo = eng.from_numpy(np.array([-55, -77], dtype=np.int32))
        mp, vp = dmean.data_ptr() + 8 * dc.GUARD, dvar.data_ptr() + 8 * dc.GUARD
        args = (ops, d, nd, M, k, bias, white, sn2 + white, flags, mp, vp, dinfo)
        if rep == 0:                                          # every refusal first, on the sentinel-filled outputs
            rcs = [launch(args, **kw) for kw in (
                {"P": None}, {"u": None}, {"ys": None}, {"kern": None}, {"nbr": None}, {"mean": None}, {"info": None}, {"nB": 0},
                {"nd": 0}, {"n": 0}, {"cap": M - 1}, {"ucap": Ns - 1}, {"k": 0}, {"k": 129}, {"flags": 2})]
            eng.sync()
            rec["refusals"] = rcs == [EINVAL] * len(rcs)
            rec["refusals_write_nothing"] = bool(
                np.array_equal(dc.bits(dmean.cpu().numpy()), dc.bits(mean.full)) and np.array_equal(dc.bits(dvar.cpu().numpy()), dc.bits(var.full))
                and dinfo.cpu().numpy().tolist() == [-55, -77])
        rc = launch(args)
        eng.sync()
        mean.full[...], var.full[...] = dmean.cpu().numpy(), dvar.cpu().numpy()
        outs.append((mean.data.copy(), var.data.copy()))
        info = dinfo.cpu().numpy().tolist()
        if rep == 0:
            c_mean = dc.Check("mean", mean, ref=ref["mean"], bound=bm, cmp=True)
            c_var = dc.Check("var", var, ref=ref["var"], bound=bv, cmp=True)
            rec.update({"rc": rc == OK, "info": info == [0, -77], "ratio_mean": c_mean.ratio(), "ratio_var": c_var.ratio(),
                        "guards": mean.guards_ok() and var.guards_ok()})
            big = int(np.argmax(ref["used"]))
            if ref["used"][big] >= 2:
                wrong_y = d["ys"].copy()
                i0, i1 = d["nbr"][big, 0], d["nbr"][big, 1]
                wrong_y[[i0, i1]] = wrong_y[[i1, i0]]
                nb1 = d["nbr"][big:big + 1]
                wrong = local_ref.local_predict(d["Xs"], wrong_y, d["Xd"][big * nd:(big + 1) * nd], nd, nb1, terms, bias, white, sn2)
                rec["bites"] = float(abs(np.longdouble(mean.get()[big, 0]) - wrong["mean"][0]) / bm[big])
        elif rep == 2:
            c_lat = dc.Check("latent", var, ref=ref["latent"], bound=bv, cmp=True)
            rec["ratio_latent"] = c_lat.ratio()
            rec["latent_mean_same"] = bool(np.array_equal(dc.bits(outs[0][0]), dc.bits(mean.data)))
    rec["repeatable"] = bool(np.array_equal(dc.bits(outs[0][0]), dc.bits(outs[1][0])) and np.array_equal(dc.bits(outs[0][1]), dc.bits(outs[1][1])))
    rec["operands_untouched"] = bool(all(np.array_equal(d[key].cpu().numpy().view(np.uint8), before[key].view(np.uint8)) for key in before))
    return rec


def failing(ops):
    """noise = -(kdiag + 1): the first pivot of every node with a sample is negative"""
    eng = ops.eng
    name, Ns, M, nd, k, comp = SHAPES[0]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    d = device_inputs(ops, name, Ns, M, nd, k, comp)
    before = {key: d[key].cpu().numpy().copy() for key in ("du", "dP", "dys", "dnbr")}
    used = (d["nbr"] >= 0).sum(axis=1)
    dmean, dvar = eng.from_numpy(np.zeros(M)), eng.from_numpy(np.zeros(M))
    dinfo = eng.from_numpy(np.array([123], dtype=np.int32))
    rc = launch((ops, d, nd, M, k, bias, white, -(tb.prior_variance(comp) + 1.0), 0, dmean.data_ptr(), dvar.data_ptr(), dinfo))
    eng.sync()
    mean, var = dmean.cpu().numpy(), dvar.cpu().numpy()
    quiet = np.uint64(0x7FF8000000000000)
    first = int(np.flatnonzero(used > 0)[0]) + 1
    return {"name": "failing", "rc": rc == OK, "info": int(dinfo.cpu().numpy()[0]), "first": first,
            "nan": bool(np.all(dc.bits(mean[used > 0]) == quiet) and np.all(dc.bits(var[used > 0]) == quiet)),
            "empty_nodes_finite": bool(np.all(mean[used == 0] == 0.0) and np.all(np.isfinite(var[used == 0]))),
            "operands_untouched": bool(all(np.array_equal(d[key].cpu().numpy().view(np.uint8), before[key].view(np.uint8)) for key in before))}


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_local_krige
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                   C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    tk = ops.lib.gpak_dev_transform_k
    tk.restype = C.c_int
    tk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_void_p]
    for shape in SHAPES:
        print(json.dumps(run(ops, *shape)), flush=True)
    print(json.dumps(failing(ops)), flush=True)


if __name__ == "__main__":
    main()
