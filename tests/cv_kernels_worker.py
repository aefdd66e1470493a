"""TEST INFRASTRUCTURE: every entry of include/gpak_dev_cv_kernels.h alone on caller-owned device buffers, one process per
family (torch holds the buffers, and its HIP runtime must come up before the library's):

    python tests/cv_kernels_worker.py gram | solve | mix | fold | loo

Buffers are allocated as tests/dev_ops_cases.py's HipOps allocates them: guarded, skewed, sentinel-filled.  One JSON record
per shape on stdout: {"name", "kernel", "ratios": {...}, "flags": {...}}.  A ratio is the worst |out - ref| / bound of one
output against the long-double reference of tests/cv_kernels_ref.py (where every bound is derived) and must be <= 1; a flag
is one property that must hold: a status code, memory that must come back bit for bit (inputs, guard bands, skew rows,
unlisted rows and columns, index lists), exact values, the same bytes from a second call on fresh copies or from another
way of asking for the same numbers.  tests/test_cv_kernels_gpu.py asserts them; that the bounds bite is shown on the CPU
(tests/test_cv_kernels.py).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cv_kernels_ref as kr  # noqa: E402
import dev_ops_cases as dc  # noqa: E402

OK, EINVAL = 0, 2
LD, INT_MAX = kr.LD, kr.INT_MAX
FAMILIES = ("gram", "solve", "mix", "fold", "loo")
SENT = dc.sentinel(1)[0]
# the entries each family launches: tests/test_cv_kernels.py holds their union to the header
ENTRIES = {"gram": ("cvg_gram",), "solve": ("cvg_solve",), "mix": ("cvg_mix",),
           "fold": ("cvf_pad", "cvf_w", "cvf_ev", "cvf_sums", "cvf_beta", "cvf_q", "cvf_gather", "cvf_unmix"),
           "loo": ("loo_rowsumsq", "loo_finish", "loo_vectors", "loo_mirror_scale", "loo_rank2", "lgo_colscale")}


def blank(rows, cols=1, ld=None):
    """an output buffer: the sentinel in every word of the payload"""
    M = dc.Mat(np.zeros((rows, cols)), ld=ld)
    M.full[...] = dc.sentinel(M.full.size)
    M.before = M.data.copy()
    return M


def same(a, b):
    return bool(np.array_equal(dc.bits(a), dc.bits(b)))


def untouched(*mats):
    """inputs: guard bands, skew rows and payload as they went in"""
    return all(bool(m.guards_ok() and same(m.data, m.before)) for m in mats)


def is_sent(a):
    return bool((dc.bits(a) == dc.SENTINEL).all())


def is_pzero(a):
    return bool((dc.bits(a) == 0).all())


class Off:
    """a Mat's payload pointer moved on by `elems` doubles"""

    def __init__(self, mat, elems):
        self.mat, self.elems = mat, elems


class Run:
    """Uploads each host buffer once, issues the calls on them, synchronises and downloads every buffer again (guard bands
    and index lists included)."""

    def __init__(self, ops):
        self.eng, self.lib, self.dev = ops.eng, ops.lib, {}

    def _ptr(self, v):
        if isinstance(v, Off):
            return self._ptr(v.mat) + 8 * v.elems
        host = v.full if isinstance(v, dc.Mat) else v
        if id(v) not in self.dev:
            self.dev[id(v)] = (host, self.eng.from_numpy(host))
        return self.dev[id(v)][1].data_ptr() + (8 * dc.GUARD if isinstance(v, dc.Mat) else 0)

    def call(self, name, *args):
        conv = [self._ptr(a) if isinstance(a, (dc.Mat, np.ndarray, Off)) else a for a in args]
        return int(getattr(self.lib, "gpak_dev_" + name)(self.eng._st(), *conv))

    def done(self):
        self.eng.sync()                     # a fault surfaces here and ends the worker
        for host, t in self.dev.values():
            host[...] = t.cpu().numpy()


def emit(name, kernel, ratios, flags):
    print(json.dumps({"name": name, "kernel": kernel, "ratios": {k: float(v) for k, v in ratios.items()},
                      "flags": {k: bool(v) for k, v in flags.items()}}), flush=True)


# ------------------------------------------------------------------------------------------------------------------------
def gram_family(ops):
    gc = kr.gram_case()
    Np, nG = gc.Np, len(gc.groups)

    def launch(order, ld, refused=False):
        perm, offs, soff = kr.lists(gc.groups, order)
        lists0 = [perm.copy(), offs.copy(), soff.copy()]
        Gm, Sm = dc.Mat(gc.G, ld=ld), blank(int(soff[-1]))
        r = Run(ops)
        rcs = [r.call("cvg_gram", Gm, ld, Np, perm, offs, len(order), soff, Sm)]
        if refused:
            rcs += [r.call("cvg_gram", Gm, ld, Np, perm, offs, 0, soff, Sm), r.call("cvg_gram", Gm, ld, Np - 24, perm, offs, nG, soff, Sm),
                    r.call("cvg_gram", Gm, Np - 1, Np, perm, offs, nG, soff, Sm), r.call("cvg_gram", Gm, ld, Np, perm, offs, nG, soff, None)]
        r.done()
        blocks = {g: Sm.data[soff[k]:soff[k + 1]].copy() for k, g in enumerate(order)}
        clean = untouched(Gm) and Sm.guards_ok() and all(np.array_equal(a, b) for a, b in zip(lists0, [perm, offs, soff]))
        return rcs, blocks, clean

    every = list(range(nG))
    rcs, first, clean = launch(every, Np, refused=True)
    runs = {"again": launch(every, Np), "odd ld": launch(every, Np + 33), "reversed": launch(every[::-1], Np + 33),
            "alone": launch([kr.GRAM_ALONE], Np)}
    emit("launches", "cvg_gram", {}, {"rc": rcs == [OK] + [EINVAL] * 4, "inputs, lists and guards": clean,
                                      **{f"rc, inputs, lists and guards ({k})": v[0] == [OK] and v[2] for k, v in runs.items()}})
    for g, I in enumerate(gc.groups):
        S, bound, k0 = gc.ref[g]
        s, sp = len(I), kr.pad16(len(I))
        ref, bnd, written = kr.s_layout(S, bound)
        M = first[g].reshape(sp, sp).T
        pad = written & ((np.arange(sp)[:, None] >= s) | (np.arange(sp)[None, :] >= s))
        flags = {"padding is +0": is_pzero(M[pad]), "tiles above the diagonal keep the sentinel": is_sent(M[~written])}
        for k, v in runs.items():
            if g in v[1]:
                flags[f"same bytes ({k})"] = same(first[g], v[1][g])
        emit(f"g={g} s={s} k0={k0}", "cvg_gram", {"S": kr.worst(M[written].astype(LD) - ref[written], bnd[written])}, flags)


# ------------------------------------------------------------------------------------------------------------------------
def solve_family(ops):
    sc = kr.solve_case()
    Np, nG = sc.Np, len(sc.groups)
    perm, offs, soff = kr.lists(sc.groups)
    qoff = (np.arange(nG) * 128 * 128).astype(np.int64)
    member = np.zeros(Np, dtype=bool)
    member[perm] = True

    def launch(weights, fail, refused=False):
        S_list = [sc.S_fail[g] if fail and g in sc.S_fail else sc.S[g] for g in range(nG)]
        b = {"S": dc.Mat(kr.s_buffer(S_list, SENT)), "y": dc.Mat(sc.y), "alpha": dc.Mat(sc.alpha), "mean": blank(Np), "var": blank(Np),
             "logp": blank(nG), "gsum": blank(3 * nG), "E": blank(Np), "Qb": blank(nG * 128 * 128)}
        ints = {"perm": perm.copy(), "offs": offs.copy(), "soff": soff.copy(), "qoff": qoff.copy(), "info": np.array([INT_MAX], dtype=np.int32)}
        w = (b["E"], b["Qb"], ints["qoff"]) if weights else (None, None, None)
        head = (b["S"], ints["soff"], ints["perm"], ints["offs"])
        tail = (b["mean"], b["var"], b["logp"], b["gsum"], ints["info"])
        r = Run(ops)
        rcs = [r.call("cvg_solve", *head, nG, 128, b["y"], b["alpha"], sc.sn2, *tail, *w)]
        if refused:
            rcs += [r.call("cvg_solve", *head, 0, 128, b["y"], b["alpha"], sc.sn2, *tail, *w),
                    r.call("cvg_solve", *head, nG, 129, b["y"], b["alpha"], sc.sn2, *tail, *w),
                    r.call("cvg_solve", *head, nG, 0, b["y"], b["alpha"], sc.sn2, *tail, *w),
                    r.call("cvg_solve", *head, nG, 128, b["y"], b["alpha"], 0.0, *tail, *w),
                    r.call("cvg_solve", *head, nG, 128, b["y"], b["alpha"], sc.sn2, *tail, b["E"], None, None),
                    r.call("cvg_solve", *head, nG, 128, b["y"], b["alpha"], sc.sn2, *tail, None, b["Qb"], ints["qoff"])]
        r.done()
        clean = (untouched(b["S"], b["y"], b["alpha"]) and all(m.guards_ok() for m in b.values())
                 and all(np.array_equal(ints[k], v) for k, v in (("perm", perm), ("offs", offs), ("soff", soff), ("qoff", qoff)))
                 and all(same(b[k].data[~member], b[k].before[~member]) for k in ("mean", "var", "E")))
        if not weights:
            clean = clean and untouched(b["E"], b["Qb"])
        return rcs, b, int(ints["info"][0]), clean

    runs = {(w, f): launch(w, f, refused=not f) for w in (False, True) for f in (False, True)}
    again = {w: launch(w, False) for w in (False, True)}
    outs = ("mean", "var", "logp", "gsum")
    flags = {}
    for (w, f), (rcs, b, info, clean) in runs.items():
        tag = f"{'weights' if w else 'plain'}{', failing pivots' if f else ''}"
        flags[f"rc ({tag})"] = rcs == ([OK] if f else [OK] + [EINVAL] * 6)
        flags[f"inputs, lists, guards and non-members ({tag})"] = clean
        flags[f"info ({tag})"] = info == (min(kr.SOLVE_FAIL) + 1 if f else INT_MAX)
    for w in (False, True):
        flags[f"same bytes again ({'weights' if w else 'plain'})"] = (again[w][0] == [OK] and again[w][3] and all(
            same(runs[w, False][1][k].data, again[w][1][k].data) for k in outs + ("E", "Qb")))
    flags["plain and weights: the same bytes"] = all(same(runs[False, f][1][k].data, runs[True, f][1][k].data) for f in (False, True)
                                                     for k in outs)
    emit("launches", "cvg_solve", {}, flags)

    for g, I in enumerate(sc.groups):
        s, ref = len(I), sc.ref[g]
        ratios, flags = {}, {}
        for w in (False, True):
            b = runs[w, False][1]
            t = "weights" if w else "plain"
            ratios[f"e through mean ({t})"] = kr.worst(b["mean"].data[I].astype(LD) - ref["mean"], sc.mean_bound(g))
            ratios[f"var ({t})"] = kr.worst(b["var"].data[I].astype(LD) - ref["var"], sc.bound(g, "var"))
            ratios[f"logp ({t})"] = kr.worst(b["logp"].data[g].astype(LD) - ref["logp"], sc.bound(g, "logp"))
            ratios[f"gsum ({t})"] = kr.worst(b["gsum"].data[3 * g:3 * g + 3].astype(LD) - ref["gsum"], sc.bound(g, "gsum"))
        b = runs[True, False][1]
        blk = b["Qb"].data[qoff[g]:qoff[g] + 128 * 128].reshape(128, 128)                  # row-major, pitch 128
        Q = np.ascontiguousarray(blk[:s, :s])
        inside = np.zeros((128, 128), dtype=bool)
        inside[:s, :s] = True
        C, cb = sc.c_ref(g)
        ratios["E"] = kr.worst(b["E"].data[I].astype(LD) - ref["e"], sc.bound(g, "e"))
        ratios["Q"] = kr.worst(Q.astype(LD) - ref["Q"], sc.bound(g, "Q"))
        ratios["Q Q' against sn2 S^-1 + e e'"] = kr.worst(dc.mm_ld(Q, Q) - C, cb) if np.isfinite(Q).all() else np.inf
        flags["the block of Qb outside s x s keeps the sentinel"] = is_sent(blk[~inside])
        for w in (False, True):
            b, bf = runs[w, False][1], runs[w, True][1]
            t = "weights" if w else "plain"
            if g in kr.SOLVE_FAIL:
                flags[f"failed: NaN in mean, var, logp, gsum ({t})"] = bool(
                    np.isnan(bf["mean"].data[I]).all() and np.isnan(bf["var"].data[I]).all() and np.isnan(bf["logp"].data[g])
                    and np.isnan(bf["gsum"].data[3 * g:3 * g + 3]).all())
            else:
                flags[f"beside failing groups: the same bytes ({t})"] = (
                    same(b["mean"].data[I], bf["mean"].data[I]) and same(b["var"].data[I], bf["var"].data[I])
                    and same(b["logp"].data[g], bf["logp"].data[g]) and same(b["gsum"].data[3 * g:3 * g + 3], bf["gsum"].data[3 * g:3 * g + 3]))
        bf = runs[True, True][1]
        fb = bf["Qb"].data[qoff[g]:qoff[g] + 128 * 128].reshape(128, 128)
        if g in kr.SOLVE_FAIL:
            flags["failed: E and Q keep the sentinel"] = is_sent(bf["E"].data[I]) and is_sent(fb)
        else:
            flags["beside failing groups: the same E and Q"] = same(b["E"].data[I], bf["E"].data[I]) and same(blk, fb)
        emit(f"g={g} s={s} kappa={sc.kappa[g]:.3g}", "cvg_solve", ratios, flags)


# ------------------------------------------------------------------------------------------------------------------------
def mix_family(ops):
    mc = kr.mix_case()
    Np, nb = mc.Np, len(kr.MIX_WIDTHS)
    Qb0 = dc.sentinel(nb * 128 * 128).reshape(nb, 128, 128)
    for b, w in enumerate(kr.MIX_WIDTHS):
        Qb0[b, :w, :w] = mc.Q[b]                                       # row-major; the sentinel beyond the bin's width

    def launch(refused=False):
        H, Qb = dc.Mat(mc.H, ld=Np + 33), dc.Mat(Qb0.ravel())
        perm, bstart = mc.perm.copy(), mc.bstart.copy()
        r = Run(ops)
        rcs = [r.call("cvg_mix", H, H.ld, Np, perm, bstart, nb, Qb)]
        if refused:
            rcs += [r.call("cvg_mix", H, H.ld, Np, perm, bstart, 0, Qb), r.call("cvg_mix", H, Np - 1, Np, perm, bstart, nb, Qb),
                    r.call("cvg_mix", H, H.ld, Np - 64, perm, bstart, nb, Qb), r.call("cvg_mix", H, H.ld, Np, perm, bstart, nb, None)]
        r.done()
        return rcs, H, untouched(Qb) and np.array_equal(perm, mc.perm) and np.array_equal(bstart, mc.bstart)

    rcs, H, clean = launch(refused=True)
    rcs2, H2, clean2 = launch()
    ref, bound, mixed = np.zeros((Np, Np), dtype=LD), np.ones((Np, Np)), np.zeros((Np, Np), dtype=bool)
    for b in range(nb):
        ref[:, mc.cols[b]], bound[:, mc.cols[b]] = mc.expect(b)
        mixed[:, mc.cols[b]] = True
    chk = dc.Check("H", H, ref=ref, bound=bound, cmp=mixed)
    emit("launch", "cvg_mix", {}, {"rc": rcs == [OK] + [EINVAL] * 4 and rcs2 == [OK], "Qb and the lists": clean and clean2,
                                   "every other column and the skew rows": chk.violations() == 0, "guards": H.guards_ok(),
                                   "same bytes again": same(H.data, H2.data)})
    for b, w in enumerate(kr.MIX_WIDTHS):
        one = np.zeros((Np, Np), dtype=bool)
        one[:, mc.cols[b]] = True
        how = "contiguous" if np.all(np.diff(mc.cols[b]) == 1) and w > 1 else "scattered"
        emit(f"width={w} {how}", "cvg_mix", {"H": dc.Check("H", H, ref=ref, bound=bound, cmp=one).ratio()}, {})


# ------------------------------------------------------------------------------------------------------------------------
def twice(stage):
    """runs a stage on fresh buffers twice: its record, and whether the outputs of the two runs are the same bytes"""
    ratios, flags, outs = stage()
    _, _, outs2 = stage()
    flags["same bytes again"] = all(same(a, b) for a, b in zip(outs, outs2))
    return ratios, flags


def cmp(mat, ref, bound, mask=None):
    mask = np.ones((mat.rows, mat.cols), dtype=bool) if mask is None else mask
    return dc.Check("", mat, ref=ref, bound=bound, cmp=mask)


def fold_family(ops):
    for m in kr.FOLD_M:
        fc = kr.fold_case(m)
        mp, NpF = fc.mp, kr.FOLD_NP
        memb = np.zeros(NpF, dtype=bool)
        memb[fc.rows] = True

        def fresh():
            return {"T": dc.Mat(fc.T, ld=mp + 3), "alpha": dc.Mat(fc.alpha), "y": dc.Mat(fc.y), "wv": dc.Mat(fc.wv), "ev": dc.Mat(fc.ev),
                    "vv": dc.Mat(fc.vv), "sc": dc.Mat(fc.sc), "rows": fc.rows.copy()}

        def ins_ok(b, *names):
            return untouched(*[b[k] for k in names]) and np.array_equal(b["rows"], fc.rows)

        def pad():
            S = blank(mp, mp, ld=mp + 1)
            r = Run(ops)
            rcs = [r.call("cvf_pad", S, S.ld, m), r.call("cvf_pad", S, S.ld, 0), r.call("cvf_pad", S, mp - 1, m), r.call("cvf_pad", None, S.ld, m)]
            r.done()
            i, j = np.arange(mp)[:, None], np.arange(mp)[None, :]
            low = (i >= m) & (j >= m) & (i >= j)
            got = S.get()
            return {}, {"rc": rcs == [OK] + [EINVAL] * 3, "identity on the padding of the lower triangle": same(got[low], np.eye(mp)[low]),
                        "everything else keeps the sentinel": cmp(S, 0, 1, low).violations() == 0 and S.guards_ok()}, [S.data]

        def w():
            b, out = fresh(), blank(m)
            r = Run(ops)
            rcs = [r.call("cvf_w", b["T"], b["T"].ld, m, b["rows"], b["alpha"], out), r.call("cvf_w", b["T"], m - 1, m, b["rows"], b["alpha"], out),
                   r.call("cvf_w", b["T"], b["T"].ld, 0, b["rows"], b["alpha"], out)]
            r.done()
            ref, bound = fc.expect_w()["wv"]
            return {"w": cmp(out, ref, bound).ratio()}, {"rc": rcs == [OK, EINVAL, EINVAL], "inputs": ins_ok(b, "T", "alpha"),
                                                           "guards": out.guards_ok()}, [out.data]

        def ev(info):
            def stage():
                b, o = fresh(), {"ev": blank(m), "vv": blank(m), "mean": blank(NpF), "var": blank(NpF)}
                inf = np.array([info], dtype=np.int32)
                r = Run(ops)
                args = (b["wv"], b["rows"], b["y"], fc.sn2, inf, o["ev"], o["vv"], o["mean"], o["var"])
                rcs = [r.call("cvf_ev", b["T"], b["T"].ld, m, *args), r.call("cvf_ev", b["T"], m - 1, m, *args)]
                r.done()
                exp = fc.expect_ev()
                flags = {"rc": rcs == [OK, EINVAL], "inputs": ins_ok(b, "T", "wv", "y") and int(inf[0]) == info,
                         "guards": all(x.guards_ok() for x in o.values()),
                         "mean and var at the members only": all(same(o[k].data[~memb], o[k].before[~memb]) for k in ("mean", "var"))}
                if info != INT_MAX:
                    flags["NaN in ev, vv, mean, var"] = bool(np.isnan(o["ev"].data).all() and np.isnan(o["vv"].data).all()
                                                             and np.isnan(o["mean"].data[fc.rows]).all() and np.isnan(o["var"].data[fc.rows]).all())
                    return {}, flags, [x.data for x in o.values()]
                ratios = {k: kr.worst(o[k].data.astype(LD) - exp[k][0], exp[k][1]) for k in ("ev", "vv")}
                ratios.update({k: kr.worst(o[k].data[fc.rows].astype(LD) - exp[k][0], exp[k][1]) for k in ("mean", "var")})
                flags["var is vv"] = same(o["var"].data[fc.rows], o["vv"].data)
                return ratios, flags, [x.data for x in o.values()]
            return stage

        def sums(info):
            def stage():
                b, logp, gsum = fresh(), blank(1), blank(3)
                Rm = np.full((m, m), kr.NAN)
                Rm[np.arange(m), np.arange(m)] = fc.rdiag
                R = dc.Mat(Rm, ld=m + 1)
                inf = np.array([info], dtype=np.int32)
                r = Run(ops)
                args = (b["ev"], b["vv"], b["rows"], b["alpha"], fc.sn2, inf, logp, gsum)
                rcs = [r.call("cvf_sums", R, R.ld, m, *args), r.call("cvf_sums", R, m - 1, m, *args)]
                r.done()
                flags = {"rc": rcs == [OK, EINVAL], "inputs": ins_ok(b, "ev", "vv", "alpha") and untouched(R) and int(inf[0]) == info,
                         "guards": logp.guards_ok() and gsum.guards_ok()}
                if info != INT_MAX:
                    flags["NaN in gsum and logp"] = bool(np.isnan(gsum.data).all() and np.isnan(logp.data).all())
                    return {}, flags, [logp.data, gsum.data]
                exp = fc.expect_sums()
                return ({"gsum": kr.worst(gsum.data.astype(LD) - exp["gsum"][0], exp["gsum"][1]),
                         "logp": kr.worst(logp.data[0].astype(LD) - exp["logp"][0], exp["logp"][1])}, flags, [logp.data, gsum.data])
            return stage

        def beta():
            b, out = fresh(), blank(2)
            r = Run(ops)
            rcs = [r.call("cvf_beta", b["wv"], m, fc.sn2, out), r.call("cvf_beta", b["wv"], 0, fc.sn2, out)]
            r.done()
            exp = fc.expect_beta()
            return ({"sc1": kr.worst(out.data[1].astype(LD) - exp["sc1"][0], exp["sc1"][1])},
                    {"rc": rcs == [OK, EINVAL], "inputs": ins_ok(b, "wv"), "guards": out.guards_ok(),
                     "sc0 is sqrt(sn2) to the bit": same(out.data[0], np.sqrt(np.float64(fc.sn2)))}, [out.data])

        def q(transposed):
            def stage():
                b, Q, E = fresh(), blank(mp, mp, ld=mp + 2), blank(NpF)
                r = Run(ops)
                args = (b["wv"], b["ev"], b["sc"], b["rows"])
                rcs = [r.call("cvf_q", transposed, b["T"], b["T"].ld, m, *args, Q, Q.ld, E),
                       r.call("cvf_q", transposed, b["T"], b["T"].ld, m, *args, Q, mp - 1, E),
                       r.call("cvf_q", transposed, b["T"], m - 1, m, *args, Q, Q.ld, E)]
                r.done()
                ref, bound = fc.expect_q(bool(transposed))["Q"]
                chk = cmp(Q, ref, bound)
                outside = np.ones((mp, mp), dtype=bool)
                outside[:m, :m] = False
                return ({"Q": chk.ratio()},
                        {"rc": rcs == [OK, EINVAL, EINVAL], "inputs": ins_ok(b, "T", "wv", "ev", "sc"), "guards": Q.guards_ok() and E.guards_ok(),
                         "skew rows": chk.violations() == 0, "+0 on the rest of mp x mp": is_pzero(Q.get()[outside]),
                         "E at the members only": same(E.data[fc.rows], fc.ev) and same(E.data[~memb], E.before[~memb])}, [Q.data, E.data])
            return stage

        for name, kernel, stage in (("pad", "cvf_pad", pad), ("w", "cvf_w", w), ("ev", "cvf_ev", ev(INT_MAX)), ("ev, failed group", "cvf_ev", ev(7)),
                                    ("sums", "cvf_sums", sums(INT_MAX)), ("sums, failed group", "cvf_sums", sums(7)), ("beta", "cvf_beta", beta),
                                    ("q", "cvf_q", q(0)), ("q transposed", "cvf_q", q(1))):
            emit(f"m={m} {name}", kernel, *twice(stage))

        # the exact copies, Np = 640: 512 rows and a ragged chunk of 128
        Np = kr.GATHER_NP
        rng = np.random.default_rng(31 + m)
        cols = np.sort(rng.choice(Np, m, replace=False)).astype(np.int32)
        H0, Z0 = rng.standard_normal((Np, Np)), rng.standard_normal((Np, m))

        def gather():
            H, A, c = dc.Mat(H0, ld=Np + 5), blank(Np, mp, ld=Np + 3), cols.copy()
            r = Run(ops)
            rcs = [r.call("cvf_gather", H, H.ld, Np, c, m, A, A.ld), r.call("cvf_gather", H, H.ld, Np, c, 0, A, A.ld),
                   r.call("cvf_gather", H, H.ld, Np, c, Np + 1, A, A.ld), r.call("cvf_gather", H, Np - 1, Np, c, m, A, A.ld),
                   r.call("cvf_gather", H, H.ld, Np, c, m, A, Np - 1)]
            r.done()
            got = A.get()
            return {}, {"rc": rcs == [OK] + [EINVAL] * 4, "inputs": untouched(H) and np.array_equal(c, cols), "guards": A.guards_ok(),
                        "skew rows": cmp(A, 0, 1).violations() == 0, "the columns, to the bit": same(got[:, :m], H0[:, cols]),
                        "+0 in the columns m .. mp - 1": is_pzero(got[:, m:])}, [A.data]

        def unmix():
            H, Z, c = dc.Mat(H0, ld=Np + 5), dc.Mat(Z0, ld=Np + 1), cols.copy()
            r = Run(ops)
            rcs = [r.call("cvf_unmix", H, H.ld, Np, c, m, Z, Z.ld), r.call("cvf_unmix", H, H.ld, Np, c, 0, Z, Z.ld),
                   r.call("cvf_unmix", H, Np - 1, Np, c, m, Z, Z.ld), r.call("cvf_unmix", H, H.ld, Np, c, m, Z, Np - 1)]
            r.done()
            listed = np.zeros((Np, Np), dtype=bool)
            listed[:, cols] = True
            return {}, {"rc": rcs == [OK] + [EINVAL] * 3, "inputs": untouched(Z) and np.array_equal(c, cols), "guards": H.guards_ok(),
                        "every other column and the skew rows": cmp(H, 0, 1, listed).violations() == 0,
                        "the columns, to the bit": same(H.get()[:, cols], Z0)}, [H.data]

        emit(f"m={m} gather", "cvf_gather", *twice(gather))
        emit(f"m={m} unmix", "cvf_unmix", *twice(unmix))


# ------------------------------------------------------------------------------------------------------------------------
def loo_family(ops):
    lc = kr.loo_case()
    Np, N = lc.Np, lc.N
    nch = (Np + kr.LOO_CHUNK - 1) // kr.LOO_CHUNK

    def rowsumsq(P, a, extra, refused=False):
        vals, grows = lc.slab(P, a)
        rows = len(grows)
        slab, part, d = dc.Mat(vals, ld=rows + extra), blank(nch * rows), blank(Np)
        r = Run(ops)
        rcs = [r.call("loo_rowsumsq", slab, slab.ld, Np, P, a, part, d)]
        if refused:
            odd = dc.Mat(vals, ld=rows + 1)
            rcs += [r.call("loo_rowsumsq", odd, odd.ld, Np, P, a, part, d), r.call("loo_rowsumsq", Off(slab, 1), slab.ld, Np, P, a, part, d),
                    r.call("loo_rowsumsq", slab, slab.ld, Np, P, P, part, d), r.call("loo_rowsumsq", slab, slab.ld, Np, 0, 0, part, d),
                    r.call("loo_rowsumsq", slab, rows - 2, Np, P, a, part, d), r.call("loo_rowsumsq", slab, slab.ld, Np - 64, P, a, part, d),
                    r.call("loo_rowsumsq", slab, slab.ld, Np, 10, 9, part, d)]          # a pass without rows
        r.done()
        mine = np.zeros(Np, dtype=bool)
        mine[grows] = True
        pm = part.data.reshape(nch, rows)
        left = np.arange(nch)[:, None] < (grows // kr.TILE * kr.TILE // kr.LOO_CHUNK)[None, :]
        flags = {"rc": rcs == ([OK] + [EINVAL] * 7 if refused else [OK]), "the slab": untouched(slab),
                 "guards": part.guards_ok() and d.guards_ok(), "d at the rows of the pass only": same(d.data[~mine], d.before[~mine]),
                 "chunk sums left of the diagonal's keep the sentinel": is_sent(pm[left])}
        return kr.worst(d.data[grows].astype(LD) - lc.d_ld[grows], lc.d_bound[grows]), flags, d.data.copy(), grows

    _, _, d1, _ = rowsumsq(1, 0, 0)
    for P in (1, 2, 3):
        for a in range(P):
            for extra in (0, 6):
                ratio, flags, d, grows = rowsumsq(P, a, extra, refused=(P == 2 and extra == 6))
                _, _, d2, _ = rowsumsq(P, a, extra)
                flags["same bytes again"] = same(d, d2)
                flags["the bytes of P = 1"] = same(d[grows], d1[grows])
                emit(f"rowsumsq P={P} a={a} lds=rows+{extra}", "loo_rowsumsq", {"d": ratio}, flags)

    def finish():
        nfin = (N + 255) // 256
        b = {"d": dc.Mat(lc.d), "y": dc.Mat(lc.y), "alpha": dc.Mat(lc.alpha)}
        mean, var, part, sums = blank(Np), blank(Np), blank(nfin * 16), blank(3)
        r = Run(ops)
        args = (b["d"], b["y"], b["alpha"])
        rcs = [r.call("loo_finish", N, *args, lc.sn2, mean, var, part, sums), r.call("loo_finish", 0, *args, lc.sn2, mean, var, part, sums),
               r.call("loo_finish", N, *args, 0.0, mean, var, part, sums), r.call("loo_finish", N, *args, lc.sn2, mean, var, part, None)]
        r.done()
        exp = lc.expect_finish()
        work = np.tile(np.arange(16) < 3, nfin)
        return ({k: kr.worst(x.data[:N].astype(LD) - exp[k][0], exp[k][1]) for k, x in (("mean", mean), ("var", var))}
                | {"sums": kr.worst(sums.data.astype(LD) - exp["sums"][0], exp["sums"][1])},
                {"rc": rcs == [OK] + [EINVAL] * 3, "inputs": untouched(*b.values()), "guards": all(x.guards_ok() for x in (mean, var, part, sums)),
                 "nothing from N on": same(mean.data[N:], mean.before[N:]) and same(var.data[N:], var.before[N:]),
                 "three of every sixteen words of the workspace": same(part.data[~work], part.before[~work])},
                [mean.data, var.data, sums.data])

    def vectors():
        b = {"d": dc.Mat(lc.d), "alpha": dc.Mat(lc.alpha)}
        s, rr = blank(Np), blank(Np)
        r = Run(ops)
        rcs = [r.call("loo_vectors", N, Np, b["d"], b["alpha"], lc.sn2, s, rr), r.call("loo_vectors", Np + 1, Np, b["d"], b["alpha"], lc.sn2, s, rr),
               r.call("loo_vectors", N, Np, b["d"], b["alpha"], -1.0, s, rr)]
        r.done()
        exp = lc.expect_vectors()
        return ({"s": kr.worst(s.data.astype(LD) - exp["s"][0], exp["s"][1]), "r": kr.worst(rr.data.astype(LD) - exp["r"][0], exp["r"][1])},
                {"rc": rcs == [OK, EINVAL, EINVAL], "inputs": untouched(*b.values()), "guards": s.guards_ok() and rr.guards_ok(),
                 "+0 from N on": is_pzero(s.data[N:]) and is_pzero(rr.data[N:])}, [s.data, rr.data])

    low64 = kr.lower_tiles(Np, 64)

    def mirror(ones):
        def stage():
            sv = np.where(np.arange(Np) < N, 1.0, 0.0) if ones else lc.s
            Bm = np.where(low64, lc.Binv, kr.NAN)                      # NaN in every tile strictly above the diagonal tiles
            B, s, H = dc.Mat(Bm, ld=Np + 2), dc.Mat(sv), blank(Np, Np, ld=Np + 4)
            r = Run(ops)
            rcs = [r.call("loo_mirror_scale", N, Np, B, B.ld, s, H, H.ld)]
            if not ones:
                oddB, oddH = dc.Mat(Bm, ld=Np + 1), blank(Np, Np, ld=Np + 3)
                rcs += [r.call("loo_mirror_scale", N, Np, oddB, oddB.ld, s, H, H.ld), r.call("loo_mirror_scale", N, Np, B, B.ld, s, oddH, oddH.ld),
                        r.call("loo_mirror_scale", N, Np, Off(B, 1), B.ld, s, H, H.ld), r.call("loo_mirror_scale", N, Np, B, B.ld, s, Off(H, 1), H.ld),
                        r.call("loo_mirror_scale", Np + 1, Np, B, B.ld, s, H, H.ld), r.call("loo_mirror_scale", N, Np - 64, B, B.ld, s, H, H.ld),
                        r.call("loo_mirror_scale", N, Np, B, Np - 2, s, H, H.ld)]
            r.done()
            got = H.get()
            want = lc.Binv * sv[None, :]                               # one IEEE product per entry
            want[N:, :] = 0.0
            flags = {"rc": rcs == ([OK] if ones else [OK] + [EINVAL] * 7), "inputs": untouched(B, s), "guards": H.guards_ok(),
                     "skew rows": cmp(H, 0, 1).violations() == 0, "every entry the bits of s_k * Binv[max(i, k), min(i, k)]": same(got, want),
                     "zeros from N on": bool((got[N:, :] == 0).all() and (got[:, N:] == 0).all()) and is_pzero(got[N:, :])}
            if ones:
                flags["H diag(1 / s) is symmetric bit for bit"] = same(got[:N, :N], got[:N, :N].T)
            return {}, flags, [H.data]
        return stage

    def rank2():
        W, v, al = dc.Mat(lc.W, ld=Np + 2), dc.Mat(lc.v), dc.Mat(lc.alpha)
        r = Run(ops)
        oddW = dc.Mat(lc.W, ld=Np + 1)
        rcs = [r.call("loo_rank2", Np, W, W.ld, v, al), r.call("loo_rank2", Np, oddW, oddW.ld, v, al), r.call("loo_rank2", Np, Off(W, 1), W.ld, v, al),
               r.call("loo_rank2", Np, W, W.ld, Off(v, 1), al), r.call("loo_rank2", Np, W, W.ld, v, Off(al, 1)),
               r.call("loo_rank2", Np - 64, W, W.ld, v, al), r.call("loo_rank2", Np, W, Np - 2, v, al)]
        r.done()
        ref, bound = lc.expect_rank2()
        chk = cmp(W, ref, bound, low64)
        return {"W": chk.ratio()}, {"rc": rcs == [OK] + [EINVAL] * 6, "inputs": untouched(v, al), "guards": W.guards_ok(),
                                    "the tiles above the diagonal and the skew rows": chk.violations() == 0}, [W.data]

    def colscale():
        s = blank(Np)
        r = Run(ops)
        rcs = [r.call("lgo_colscale", N, Np, 1.0 / lc.sn2, s), r.call("lgo_colscale", Np + 1, Np, 1.0, s), r.call("lgo_colscale", N, Np, 1.0, None)]
        r.done()
        return {}, {"rc": rcs == [OK, EINVAL, EINVAL], "guards": s.guards_ok(), "c below N, to the bit": same(s.data[:N], np.full(N, 1.0 / lc.sn2)),
                    "+0 from N on": is_pzero(s.data[N:])}, [s.data]

    for name, kernel, stage in (("finish", "loo_finish", finish), ("vectors", "loo_vectors", vectors), ("mirror_scale", "loo_mirror_scale", mirror(False)),
                                ("mirror_scale, s = 1", "loo_mirror_scale", mirror(True)), ("rank2", "loo_rank2", rank2),
                                ("colscale", "lgo_colscale", colscale)):
        emit(name, kernel, *twice(stage))


def main():
    family = sys.argv[1]
    assert family in FAMILIES, family
    ops = dc.HipOps()
    for name in kr_entries():
        getattr(ops.lib, name).restype = C.c_int
    {"gram": gram_family, "solve": solve_family, "mix": mix_family, "fold": fold_family, "loo": loo_family}[family](ops)


def kr_entries():
    return ["gpak_dev_" + e for fam in FAMILIES for e in ENTRIES[fam]]


if __name__ == "__main__":
    main()
