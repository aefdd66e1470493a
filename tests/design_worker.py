"""TEST INFRASTRUCTURE: gpak_dev_design_score (include/gpak_dev_design.h) alone on caller-owned device buffers, in a
process of its own (torch holds the buffers, and its HIP runtime must come up before the library's).  Buffers are
allocated as tests/dev_ops_cases.py's HipOps allocates them: guarded, skewed, sentinel-filled.  One JSON record per shape
on stdout.

Input: a lower-stored matrix whose candidate rows carry, per hole, a synthetic A_h - noise I = G G' / m + I (so A_h has its
eigenvalues in [2, 2 + |G|^2 / m] with noise = 1: kappa(A_h) <= KAPPA, asserted) and a standard-normal P_{I,.}; everything
the kernel has no business reading -- the upper triangle, the blocks between different holes, the target x target block --
holds the sentinel NaN, so a stray read shows in the outputs.

Bound per column norm n_b = |X p_b|^2 (X = R^-1, A = R R', p_b = P_{I,b}, m = the hole's points, u = 2^-53), first order
in u, 2-norms:
  (a) the Cholesky: R^ R^' = A + E, |E|_F <= (m + 1) u |R^|_F^2 <= (m + 1) u m |A| (Higham, Accuracy and Stability,
      thm 10.3); p' (A + E)^-1 p - n_b = -p' A^-1 E A^-1 p, at most |X|^2 |E| n_b <= (m + 1) m kappa u n_b;
  (b) X^ column by column, each a substitution of at most m terms per entry: (R^ + D_i) x^_i = e_i, |D_i| <= m u |R^|, so
      |X^ - R^^-1|_F <= m u |X| |R|_F |X|_F <= m^2 u sqrt(kappa) |X|; it moves n_b by at most 2 |z| times that times |p|;
  (c) z^ = fl(X^ p): ONE fma chain over k ascending per entry (the MFMA accumulator), at most m terms:
      |z^ - X^ p| <= m u |X|_F |p| <= m^1.5 u |X| |p|; it moves n_b by at most 2 |z| times that;
  (d) the squares: per lane an fma chain over 4 rows, then 32 partial sums added in ascending order by one lane: at most
      4 + 32 + 1 roundings, 37 u n_b.
With n_b <= |X|^2 |p_b|^2 and |z| <= |X| |p|:  |n^_b - n_b| <= c(m) u |X|^2 |p_b|^2,
      c(m) = (m + 1) m KAPPA + 2 m^2 sqrt(KAPPA) + 2 m^1.5 + 37.
gain[h] = one chain over b ascending of the rounded products wt_b n^_b: sum_b wt_b bound_b + (T + 1) u sum_b wt_b n_b.
"bites": against a reference in which two rows of P_{I,.} of the largest hole were swapped the ratio must be beyond 1e6.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import design_ref  # noqa: E402
import dev_ops_cases as dc  # noqa: E402

OK, EINVAL = 0, 2
KAPPA = 4.0
NOISE = 1.0
SIZES = [1, 15, 16, 17, 127, 128]          # then two interleaved holes of 24 points (not contiguous)
# (id, T, weights?, live list or None)
SHAPES = [("T=1", 1, False, None), ("T=33", 33, True, None), ("T=70-live", 70, True, [7, 0, 5, 2]), ("T=130", 130, False, None)]


def c_of(m):
    return (m + 1) * m * KAPPA + 2 * m * m * np.sqrt(KAPPA) + 2 * m ** 1.5 + 37


def layout(T):
    rows, offs, at = [], [0], T
    for m in SIZES:
        rows += list(range(at, at + m))
        at += m
        offs.append(len(rows))
    a, b = list(range(at, at + 48, 2)), list(range(at + 1, at + 48, 2))
    rows += a + b
    offs += [offs[-1] + 24, offs[-1] + 48]
    return np.array(rows, dtype=np.int32), np.array(offs, dtype=np.int32), at + 48


def run(ops, name, T, weighted, live):
    eng, lib = ops.eng, ops.lib
    rng = np.random.default_rng(500 + T)
    rows, offs, S = layout(T)
    H = len(offs) - 1
    P0 = dc.sentinel(S * S).reshape(S, S).copy()
    kappa = 1.0
    for h in range(H):
        I = rows[offs[h]:offs[h + 1]]
        m = len(I)
        G = rng.standard_normal((m, m))
        A = G @ G.T / m + np.eye(m)
        ev = np.linalg.eigvalsh(A + NOISE * np.eye(m))
        kappa = max(kappa, float(ev[-1] / ev[0]))
        for i in range(m):
            P0[I[i], I[:i + 1]] = A[i, :i + 1]                  # the lower triangle through the hole's rows
        P0[I, :T] = rng.standard_normal((m, T))
    wt = (0.25 + rng.random(T)) if weighted else None
    if weighted and T > 2:
        wt[2] = 0.0
    hl = list(range(H)) if live is None else live
    want_red, want_gain = np.zeros((T, H), dtype=dc.LD), np.zeros(H, dtype=dc.LD)
    b_red, b_gain = np.ones((T, H)), np.ones(H)
    w = np.ones(T) if wt is None else wt
    swapped = None
    for h in hl:
        I = rows[offs[h]:offs[h + 1]]
        m = len(I)
        A = np.tril(P0[np.ix_(I, I)])
        A = (A + np.tril(A, -1).T).astype(dc.LD) + dc.LD(NOISE) * np.eye(m, dtype=dc.LD)
        R = design_ref.chol(A)
        Pm = P0[I, :T].astype(dc.LD)
        Z = design_ref.solve_lower(R, Pm)
        want_red[:, h] = (Z * Z).sum(axis=0)
        want_gain[h] = w.astype(dc.LD) @ want_red[:, h]
        x2 = float(np.linalg.norm(np.linalg.inv(R.astype(float)), 2) ** 2)
        b_red[:, h] = c_of(m) * dc.U * x2 * (P0[I, :T] ** 2).sum(axis=0)
        b_gain[h] = w @ b_red[:, h] + (T + 1) * dc.U * float(want_gain[h])
        if m == 128:
            Pw = Pm.copy()
            Pw[[0, 127]] = Pw[[127, 0]]
            Zw = design_ref.solve_lower(R, Pw)
            swapped = (h, (Zw * Zw).sum(axis=0))
    rec = {"name": name, "T": T, "H": H, "kappa": kappa}
    cmp_red = np.zeros((T, H), dtype=bool)
    cmp_red[:, hl] = True
    cmp_gain = np.zeros(H, dtype=bool)
    cmp_gain[hl] = True
    outs = []
    for rep in range(2):                                          # the second call on fresh copies: the same bytes
        Pm_, red, gain = dc.Mat(P0, ld=S + 6), dc.Mat(np.zeros((T, H)), ld=T + 3), dc.Mat(np.zeros(H))
        red.full[...] = dc.sentinel(red.full.size)
        gain.full[...] = dc.sentinel(gain.full.size)
        red.before, gain.before = red.data.copy(), gain.data.copy()
        info = np.array([dc.INT_MAX, -77], dtype=np.int32)
        livea = None if live is None else np.array(live, dtype=np.int32)
        dP, dred, dgain = eng.from_numpy(Pm_.full), eng.from_numpy(red.full), eng.from_numpy(gain.full)
        drows, doffs, dinfo = eng.from_numpy(rows), eng.from_numpy(offs), eng.from_numpy(info)
        dlive = None if live is None else eng.from_numpy(livea)
        dwt = None if wt is None else eng.from_numpy(dc.Mat(wt).full)
        pp, rp, gp = (t.data_ptr() + 8 * dc.GUARD for t in (dP, dred, dgain))
        wp = None if wt is None else dwt.data_ptr() + 8 * dc.GUARD
        lp = None if live is None else dlive.data_ptr()
        st = eng._st()
        args = (pp, Pm_.ld, T, drows.data_ptr(), doffs.data_ptr(), lp, len(hl), NOISE, wp, gp, rp, red.ld, dinfo.data_ptr())
        rcs = [lib.gpak_dev_design_score(st, *args)]
        if rep == 0:
            def bad(**kw):
                a = dict(zip(("P", "ld", "T", "rows", "offs", "live", "n", "noise", "wt", "gain", "red", "ldr", "info"), args))
                a.update(kw)
                return lib.gpak_dev_design_score(st, *a.values())
            rcs += [bad(P=None), bad(rows=None), bad(offs=None), bad(gain=None), bad(info=None), bad(T=0), bad(n=0), bad(ld=T),
                    bad(ldr=T - 1)]
        eng.sync()
        Pm_.full[...], red.full[...], gain.full[...] = dP.cpu().numpy(), dred.cpu().numpy(), dgain.cpu().numpy()
        outs.append((red.data.copy(), gain.data.copy()))
        if rep:
            continue
        c_red = dc.Check("reduction", red, ref=want_red, bound=b_red, cmp=cmp_red)
        c_gain = dc.Check("gain", gain, ref=want_gain, bound=b_gain, cmp=cmp_gain[:, None])
        rec.update({"rc": rcs == [OK] + [EINVAL] * 9,
                    "ratio_reduction": c_red.ratio(), "ratio_gain": c_gain.ratio(),
                    "others_untouched": c_red.violations() == 0 and c_gain.violations() == 0,
                    "guards": red.guards_ok() and gain.guards_ok(),
                    "P_untouched": bool(Pm_.guards_ok() and np.array_equal(dc.bits(Pm_.data), dc.bits(Pm_.before))),
                    "lists_untouched": bool(np.array_equal(drows.cpu().numpy(), rows) and np.array_equal(doffs.cpu().numpy(), offs)
                                            and (live is None or np.array_equal(dlive.cpu().numpy(), livea))
                                            and (wt is None or np.array_equal(dc.bits(dwt.cpu().numpy()), dc.bits(dc.Mat(wt).full)))),
                    "info": dinfo.cpu().numpy().tolist() == [dc.INT_MAX, -77]})
        if swapped is not None:
            wrong = want_red.copy()
            wrong[:, swapped[0]] = swapped[1]
            rec["bites"] = dc.Check("reduction", red, ref=wrong, bound=b_red, cmp=cmp_red).ratio()
        if weighted and T > 2:                                    # the zero weight is ignored exactly: the chain without it
            got_red = red.get()
            chain = np.zeros(H)
            for b in range(T):
                if b != 2:
                    chain = chain + wt[b] * got_red[b, :]
            rec["zero_weight_exact"] = bool(np.array_equal(dc.bits(chain[hl]), dc.bits(gain.get()[hl, 0])))
    rec["repeatable"] = bool(all(np.array_equal(dc.bits(a), dc.bits(b)) for a, b in zip(outs[0], outs[1])))
    return rec


def failing(ops):
    """a hole whose A is not positive definite: NaN outputs for that hole alone, info = the smallest such h + 1"""
    eng, lib = ops.eng, ops.lib
    T, S = 5, 5 + 6
    P0 = np.zeros((S, S))
    rng = np.random.default_rng(9)
    P0[5:, :5] = rng.standard_normal((6, 5))
    P0[5:, 5:] = np.eye(6)
    P0[8, 8] = -3.0                                               # hole 1 = rows 7..8 fails, hole 2 = rows 9..10 fails too
    P0[10, 10] = -3.0
    rows, offs = np.arange(5, 11, dtype=np.int32), np.array([0, 2, 4, 6], dtype=np.int32)
    Pm_, red, gain = dc.Mat(P0, ld=S), dc.Mat(np.zeros((T, 3))), dc.Mat(np.zeros(3))
    info = np.array([dc.INT_MAX], dtype=np.int32)
    dP, dred, dgain = eng.from_numpy(Pm_.full), eng.from_numpy(red.full), eng.from_numpy(gain.full)
    drows, doffs, dinfo = eng.from_numpy(rows), eng.from_numpy(offs), eng.from_numpy(info)
    pp, rp, gp = (t.data_ptr() + 8 * dc.GUARD for t in (dP, dred, dgain))
    rc = lib.gpak_dev_design_score(eng._st(), pp, Pm_.ld, T, drows.data_ptr(), doffs.data_ptr(), None, 3, NOISE, None, gp, rp,
                                   red.ld, dinfo.data_ptr())
    eng.sync()
    red.full[...], gain.full[...] = dred.cpu().numpy(), dgain.cpu().numpy()
    g, r = gain.get()[:, 0], red.get()
    return {"name": "failing", "rc": rc == OK, "info": int(dinfo.cpu().numpy()[0]),
            "nan": bool(np.isnan(g[1]) and np.isnan(g[2]) and np.isnan(r[:, 1:]).all()),
            "hole0_finite": bool(np.isfinite(g[0]) and np.isfinite(r[:, 0]).all())}


def main():
    ops = dc.HipOps()
    fn = ops.lib.gpak_dev_design_score
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    for shape in SHAPES:
        print(json.dumps(run(ops, *shape)), flush=True)
    print(json.dumps(failing(ops)), flush=True)


if __name__ == "__main__":
    main()
