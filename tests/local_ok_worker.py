"""TEST INFRASTRUCTURE: gpak_dev_local_krige_ok (include/gpak_dev_local_ok.h) alone on caller-owned device buffers, in a
process of its own, as tests/local_worker.py runs gpak_dev_local_krige: the same device inputs (its device_inputs), the
outputs guarded and sentinel-filled.  One JSON record per shape on stdout.

Bound per node.  The notation and the parts (a) - (c) are local_worker's: s samples, K = K_II, kb = kbar, y = y_I,
one = the ones vector (|one| = sqrt(s), exact), u = 2^-53, tau the fill tolerance relative to kmax, n1 = |K^-1|_2,
  |dK| <= s tau kmax,   |dkb| <= sqrt(s) (tau + (nd + 2) u) kmax,   dy = d one = 0.
THREE rows are substituted now, so the factorisation and the substitutions together are one perturbation of K of at most
  E = (s + 1) u tr K + 3 s u tr K = (4 s + 1) u tr K                          (Higham thm 10.3 and, per row, thm 8.5)
and every one of the FIVE dots f(p, r) = p' K^-1 r = (L^-1 p) . (L^-1 r), summed with at most s / 64 + 7 roundings, has
  |d f(p, r)| <= n1 (|dp| |r| + |p| |dr|) + n1^2 |p| |r| (|dK| + E) + (s / 64 + 7) u n1 |p| |r|
(|L^-1 p|^2 = p' K^-1 p <= n1 |p|^2).  With p, r from {kb, y, one}:
  m0 = f(kb, y), q = f(kb, kb) as in local_worker (with this E), a = f(one, one), b_y = f(one, y), b_k = f(one, kb).
The epilogue, first order, every operation one rounding (the order gpak_dev_local_ok.h states):
  mu   = b_y / a           |d mu|   <= |d b_y| / a + |b_y| |d a| / a^2 + u |mu|
  r    = 1 - b_k           |d r|    <= |d b_k| + u |r|
  t    = r / a             |d t|    <= |d r| / a + |r| |d a| / a^2 + u |t|
  mean = fma(r, mu, m0)    |d mean| <= |d m0| + |r| |d mu| + |mu| |d r| + u |mean|
  var  = fma(r, t, kbb - q) + add
                           |d var|  <= |d kbb| + |d q| + |r| |d t| + |t| |d r| + 4 u (kmax + r t)
with |d kbb| = (tau + (nd^2 / 64 + 8) u) kmax as in local_worker.  a, b_y, b_k, mu, r, t are taken from the float64
restatement.  The noise is SN2 = 1, as in local_worker and for its reason.
"bites": against SIMPLE kriging's long-double variance (local_ref.local_predict) the worst ratio is beyond 1e3.
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
import local_ok_ref as okr  # noqa: E402
import local_ref  # noqa: E402
import local_worker as lw  # noqa: E402
import test_block_gpu as tb  # noqa: E402

OK, EINVAL = lw.OK, lw.EINVAL
TAU, SN2 = lw.TAU, lw.SN2
# (id, Ns, M, nd, k, composition): k = 128, 64, 32 and 16, a plain composition and one with a White child
SHAPES = [("ok-defaults-k128", 300, 37, 8, 128, "defaults"), ("ok-white-k128", 300, 37, 2, 128, "expans+rbf+bias+white"),
          ("ok-white-k64", 300, 26, 1, 64, "expans+rbf+bias+white"), ("ok-defaults-k32", 300, 30, 27, 32, "defaults"),
          ("ok-white-k16", 300, 9, 8, 16, "expans+rbf+bias+white"), ("ok-defaults-k16", 300, 9, 1, 16, "defaults")]
QUIET = np.uint64(0x7FF8000000000000)


def bounds(Xs, ys, Xd, nd, nbr, terms, bias, white, sn2):
    """(bound of mean, of var / latent, of mu) per node; 0 for a node without a sample (nothing is compared there)"""
    M = nbr.shape[0]
    bm, bv, bu = np.zeros(M), np.zeros(M), np.zeros(M)
    u = dc.U
    for b in range(M):
        I = nbr[b][nbr[b] >= 0]
        s = len(I)
        if s == 0:
            continue
        pts = Xd[b * nd:(b + 1) * nd]
        kmax = bias + sum(p[{0: 6, 1: 1, 2: 2}[kd]] ** 2 for kd, p in terms) + sn2 + white
        bkbb = (TAU + (nd * nd / 64 + 8) * u) * kmax
        K = design_ref.averaged(Xs[I], Xs[I], 1, 1, terms, bias, float) + (sn2 + white) * np.eye(s)
        kb = design_ref.averaged(Xs[I], pts, 1, nd, terms, bias, float)[:, 0]
        Ki = np.linalg.inv(K)
        n1 = float(np.linalg.norm(Ki, 2))
        ny, nk, no = float(np.linalg.norm(ys[I])), float(np.linalg.norm(kb)), float(np.sqrt(s))
        dK, dkb = s * TAU * kmax, np.sqrt(s) * (TAU + (nd + 2) * u) * kmax
        E = (4 * s + 1) * u * float(np.trace(K))
        dot = (s / 64 + 7) * u

        def form(np_, nr, dp, dr):
            return n1 * (dp * nr + np_ * dr) + n1 * n1 * np_ * nr * (dK + E) + dot * n1 * np_ * nr

        d_m0, d_q = form(nk, ny, dkb, 0.0), form(nk, nk, dkb, dkb)
        d_a, d_by, d_bk = form(no, no, 0.0, 0.0), form(no, ny, 0.0, 0.0), form(no, nk, 0.0, dkb)
        one = np.ones(s)
        a, by, bk = float(one @ Ki @ one), float(one @ Ki @ ys[I]), float(one @ Ki @ kb)
        mu, r = by / a, 1.0 - bk
        t = r / a
        mean = float(kb @ Ki @ ys[I]) + r * mu
        d_mu = d_by / a + abs(by) * d_a / (a * a) + u * abs(mu)
        d_r = d_bk + u * abs(r)
        d_t = d_r / a + abs(r) * d_a / (a * a) + u * abs(t)
        bu[b] = d_mu
        bm[b] = d_m0 + abs(r) * d_mu + abs(mu) * d_r + u * abs(mean)
        bv[b] = bkbb + d_q + abs(r) * d_t + abs(t) * d_r + 4 * u * (kmax + r * t)
    return bm, bv, bu


def launch(base, **kw):
    ops, d, nd, M, k, bias, white, noise, flags, mean, var, mu, dinfo = base
    a = {"P": d["dP"].data_ptr(), "cap": d["cap"], "nB": M, "nd": nd, "u": d["du"].data_ptr(), "ucap": d["ucap"], "n": len(d["ys"]),
         "ys": d["dys"].data_ptr(), "kern": d["kern"].ctypes.data_as(C.POINTER(C.c_double)), "bias": bias, "mode": d["mode"],
         "white": white, "noise": noise, "nbr": d["dnbr"].data_ptr(), "k": k, "flags": flags, "mean": mean, "var": var, "mu": mu,
         "info": dinfo.data_ptr()}
    a.update(kw)
    return ops.lib.gpak_dev_local_krige_ok(ops.eng._st(), *a.values())


def run(ops, name, Ns, M, nd, k, comp):
    eng = ops.eng
    cols, terms, bias, white, _ = tb.COMPS[comp]
    sn2 = SN2
    d = lw.device_inputs(ops, name, Ns, M, nd, k, comp)
    ref = okr.local_predict_ok(d["Xs"], d["ys"], d["Xd"], nd, d["nbr"], terms, bias, white, sn2)
    sk = local_ref.local_predict(d["Xs"], d["ys"], d["Xd"], nd, d["nbr"], terms, bias, white, sn2)
    bm, bv, bu = bounds(d["Xs"], d["ys"], d["Xd"], nd, d["nbr"], terms, bias, white, sn2)
    live = (ref["used"] > 0)[:, None]
    before = {key: d[key].cpu().numpy().copy() for key in ("du", "dP", "dys", "dnbr")}
    rec = {"name": name, "notpd_in_reference": bool(ref["notpd"].any()), "sizes": sorted(set(int(v) for v in ref["used"]))}
    outs = []
    for rep, flags in enumerate((0, 0, 1)):                   # the second call: the same bytes; the third: latent
        mats = [dc.Mat(np.zeros(M)) for _ in range(3)]
        for m in mats:
            m.full[...] = dc.sentinel(m.full.size)
            m.before = m.data.copy()
        dev = [eng.from_numpy(m.full) for m in mats]
        dinfo = eng.from_numpy(np.array([-55, -77], dtype=np.int32))
        ptr = [t.data_ptr() + 8 * dc.GUARD for t in dev]
        args = (ops, d, nd, M, k, bias, white, sn2 + white, flags, ptr[0], ptr[1], ptr[2], dinfo)
        if rep == 0:                                          # every refusal first, on the sentinel-filled outputs
            rcs = [launch(args, **kw) for kw in (
                {"P": None}, {"u": None}, {"ys": None}, {"kern": None}, {"nbr": None}, {"mean": None}, {"info": None}, {"nB": 0},
                {"nd": 0}, {"n": 0}, {"cap": M - 1}, {"ucap": Ns - 1}, {"k": 0}, {"k": 129}, {"flags": 2}, {"flags": 3})]
            eng.sync()
            rec["refusals"] = rcs == [EINVAL] * len(rcs)
            rec["refusals_write_nothing"] = bool(
                all(np.array_equal(dc.bits(t.cpu().numpy()), dc.bits(m.full)) for t, m in zip(dev, mats))
                and dinfo.cpu().numpy().tolist() == [-55, -77])
        rc = launch(args)
        eng.sync()
        for t, m in zip(dev, mats):
            m.full[...] = t.cpu().numpy()
        mean, var, mu = mats
        outs.append([m.data.copy() for m in mats])
        info = dinfo.cpu().numpy().tolist()
        if rep == 0:
            rec.update({"rc": rc == OK, "info": info == [0, -77],
                        "ratio_mean": dc.Check("mean", mean, ref=ref["mean"], bound=bm, cmp=live).ratio(),
                        "ratio_var": dc.Check("var", var, ref=ref["var"], bound=bv, cmp=live).ratio(),
                        "ratio_mu": dc.Check("mu", mu, ref=ref["mu"], bound=bu, cmp=live).ratio(),
                        "guards": all(m.guards_ok() for m in mats)})
            dead = ~live[:, 0]
            rec["empty_nodes_nan"] = bool(dead.any() and all(np.all(dc.bits(m.get()[dead, 0]) == QUIET) for m in mats))
            rec["bites"] = dc.Check("var", var, ref=sk["var"], bound=bv, cmp=live).ratio()
            # mu and var may be NULL: the same mean bytes
            only = dc.Mat(np.zeros(M))
            donly = eng.from_numpy(only.full)
            rc2 = launch(args[:9] + (donly.data_ptr() + 8 * dc.GUARD, None, None, dinfo))
            eng.sync()
            only.full[...] = donly.cpu().numpy()
            rec["mean_alone_same"] = bool(rc2 == OK and np.array_equal(dc.bits(only.data), dc.bits(mean.data)))
        elif rep == 2:
            rec["ratio_latent"] = dc.Check("latent", var, ref=ref["latent"], bound=bv, cmp=live).ratio()
            rec["latent_mean_same"] = bool(np.array_equal(dc.bits(outs[0][0]), dc.bits(mean.data))
                                           and np.array_equal(dc.bits(outs[0][2]), dc.bits(mu.data)))
    rec["repeatable"] = bool(all(np.array_equal(dc.bits(a), dc.bits(b)) for a, b in zip(outs[0], outs[1])))
    rec["operands_untouched"] = bool(all(np.array_equal(d[key].cpu().numpy().view(np.uint8), before[key].view(np.uint8)) for key in before))
    return rec


def failing(ops):
    """noise = -(kdiag + 1): the first pivot of every node with a sample is negative"""
    eng = ops.eng
    name, Ns, M, nd, k, comp = SHAPES[0]
    cols, terms, bias, white, sn2 = tb.COMPS[comp]
    d = lw.device_inputs(ops, name, Ns, M, nd, k, comp)
    before = {key: d[key].cpu().numpy().copy() for key in ("du", "dP", "dys", "dnbr")}
    used = (d["nbr"] >= 0).sum(axis=1)
    dev = [eng.from_numpy(np.zeros(M)) for _ in range(3)]
    dinfo = eng.from_numpy(np.array([123], dtype=np.int32))
    rc = launch((ops, d, nd, M, k, bias, white, -(tb.prior_variance(comp) + 1.0), 0, dev[0].data_ptr(), dev[1].data_ptr(),
                 dev[2].data_ptr(), dinfo))
    eng.sync()
    out = [t.cpu().numpy() for t in dev]
    first = int(np.flatnonzero(used > 0)[0]) + 1
    return {"name": "failing", "rc": rc == OK, "info": int(dinfo.cpu().numpy()[0]), "first": first,
            "nan": bool(all(np.all(dc.bits(v) == QUIET) for v in out)), "has_empty": bool((used == 0).any()),
            "operands_untouched": bool(all(np.array_equal(d[key].cpu().numpy().view(np.uint8), before[key].view(np.uint8)) for key in before))}


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_local_krige_ok
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                   C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    tk = ops.lib.gpak_dev_transform_k
    tk.restype = C.c_int
    tk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_void_p]
    for shape in SHAPES:
        print(json.dumps(run(ops, *shape)), flush=True)
    print(json.dumps(failing(ops)), flush=True)


if __name__ == "__main__":
    main()
