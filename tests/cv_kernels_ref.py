"""TEST INFRASTRUCTURE: long-double restatements of the operations behind include/gpak_dev_cv_kernels.h, each from that
operation's OWN inputs, the elementwise bounds the kernels are held to, and the cases of tests/test_cv_kernels.py (CPU) and
tests/cv_kernels_worker.py (GPU).  Written from the header and the mathematics, not from the device code.

u = 2^-53.  A sum of n products added in ANY order is within n u sum|terms| of the exact sum (first order); every bound
of the form (n + 2) u sum|terms| below is that rule with room for two more roundings (dev_ops_cases.gemm_expect).
Where an output is a short expression its roundings are counted one by one in the function that states its bound.

Every case also carries `wrong`: the same reference with one deliberate error.  tests/test_cv_kernels.py asserts that it
misses the bound by at least 1000 times, so a kernel within the bound of the reference cannot be that wrong kernel.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dev_ops_cases as dc  # noqa: E402

LD, U = dc.LD, dc.U
TILE = 128
INT_MAX = 0x7FFFFFFF
LOG2PI_LD = LD("1.8378770664093454835606594728112353")
NAN = np.float64("nan")


def pad16(s):
    return (s + 15) // 16 * 16


def pad128(m):
    return (m + 127) // 128 * 128


def upper_factor(n, seed):
    """triu(randn) / sqrt(n) + I: upper triangular, exact zeros below the diagonal, well conditioned rows"""
    rng = np.random.default_rng(seed)
    return np.triu(rng.standard_normal((n, n))) / math.sqrt(n) + np.eye(n)


def worst(err, bound):
    """max |err| / bound (inf where the bound is 0 and the error is not)"""
    err, bound = np.abs(np.asarray(err, dtype=LD)).astype(np.float64), np.asarray(bound, dtype=np.float64)
    err, bound = np.broadcast_arrays(err, bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(err), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the batched groups: Gram, solve, mix
# ------------------------------------------------------------------------------------------------------------------------
GRAM_NP = 1024
GRAM_SIZES = (1, 15, 16, 17, 32, 33, 48, 64, 65, 80, 96, 112, 113, 127, 128)
GRAM_ALONE = 8            # the group that is also launched alone
SOLVE_FAIL = {3: 5, 7: 40}   # group -> the column at which its pivot is made to fail
SOLVE_SN2 = 0.37


def gram_groups():
    """The 15 groups in the order of GRAM_SIZES, members ascending, disjoint.  Their sizes add up to 947 of the 1024 rows, so
    every-7th-row scatters and contiguous holes can only coexist in separate row ranges: rows 0 .. 895 are seven lattices
    r (mod 7) of 128 slots each, filled group after group -- (128), (127, 1), (113, 15), (112, 16), (96, 32), (80, 48),
    (65, 33, 17) -- so the group of 128 starts at row 0 and the second group of a lattice starts in a later 128-tile; the group of 64 is a
    contiguous hole wholly inside the last 128-tile (rows 928 .. 991: the shortest loop).  77 rows are in no list: 13 slots
    of lattice 6 and rows 896 .. 927, 992 .. 1023."""
    lattices = ((128,), (127, 1), (113, 15), (112, 16), (96, 32), (80, 48), (65, 33, 17))
    by_size = {}
    for r, sizes in enumerate(lattices):
        slot = 0
        for s in sizes:
            by_size[s] = (r + 7 * (slot + np.arange(s))).astype(np.int32)
            slot += s
    by_size[64] = (928 + np.arange(64)).astype(np.int32)
    return [by_size[s] for s in GRAM_SIZES]


def lists(groups, order=None):
    """perm, offs, soff of the groups launched in `order`"""
    order = range(len(groups)) if order is None else order
    perm = np.concatenate([groups[g] for g in order]).astype(np.int32)
    sizes = [len(groups[g]) for g in order]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    soff = np.concatenate([[0], np.cumsum([pad16(s) ** 2 for s in sizes])]).astype(np.int64)
    return perm, offs, soff


def gram_ref(G, I, k0=None):
    """S = sum_{k >= k0} G[I, k] G[I, k]' in long double and its bound (K + 2) u |G_I| |G_I|', K = Np - k0; k0 = the 128-tile
    of the smallest member unless given"""
    I = np.asarray(I)
    k0 = int(I.min()) // TILE * TILE if k0 is None else k0
    A = np.ascontiguousarray(G[I][:, k0:])
    return dc.mm_ld(A, A), (G.shape[0] - k0 + 2) * U * (np.abs(A) @ np.abs(A).T), k0


def s_layout(S, bound):
    """(ref, bound, written) as the sp x sp column-major block of the header: the 16-tiles on and below the diagonal tiles
    are written whole, zero on the padding (bound 0 there); the tiles strictly above are not written"""
    s = S.shape[0]
    sp = pad16(s)
    ref, bnd = np.zeros((sp, sp), dtype=LD), np.zeros((sp, sp))
    ref[:s, :s], bnd[:s, :s] = S, bound
    t = np.arange(sp) // 16
    return ref, bnd, t[:, None] >= t[None, :]


class GramCase:
    def __init__(self):
        self.Np = GRAM_NP
        self.G = upper_factor(self.Np, 20240)
        self.groups = gram_groups()
        self.ref = [gram_ref(self.G, I) for I in self.groups]          # (S, bound, k0) per group

    def wrong(self, g):
        """k0 one tile to the right: the products of the group's first column tile are lost"""
        S, _, k0 = self.ref[g]
        return gram_ref(self.G, self.groups[g], k0 + TILE)[0] if k0 + TILE < self.Np else 2 * S


_GRAM = []


def gram_case():
    if not _GRAM:
        _GRAM.append(GramCase())
    return _GRAM[0]


def chol_lower(S, dtype):
    """(R, failed column or -1): S = R R' from the lower triangle of S, column by column; no BLAS (sums by numpy's own
    pairwise reduction), so that the float64 run is the same on every machine"""
    s = S.shape[0]
    A = np.tril(np.asarray(S)).astype(dtype)
    R = np.zeros((s, s), dtype=dtype)
    for j in range(s):
        d = A[j, j] - (R[j, :j] * R[j, :j]).sum()
        if not d > 0:
            return R, j
        R[j, j] = np.sqrt(d)
        R[j + 1:, j] = (A[j + 1:, j] - (R[j + 1:, :j] * R[j, :j]).sum(axis=1)) / R[j, j]
    return R, -1


def tri_inv(R, dtype):
    s = R.shape[0]
    X = np.zeros((s, s), dtype=dtype)
    for j in range(s):
        row = -(R[j, :j, None] * X[:j, :j + 1]).sum(axis=0)
        row[j] += 1
        X[j, :j + 1] = row / R[j, j]
    return X


def solve_ref(S, alpha, y, sn2, dtype=LD):
    """The outputs of the solve of one group from its S (lower triangle), alpha_I, y_I and sn2, in `dtype`: None when a
    pivot is not positive.  dtype = float64: the restatement whose error calibrates the constant c of the bound."""
    s = S.shape[0]
    R, fail = chol_lower(S, dtype)
    if fail >= 0:
        return None
    al, yy, sn = np.asarray(alpha).astype(dtype), np.asarray(y).astype(dtype), dtype(sn2)
    X = tri_inv(R, dtype)
    w = (X * al[None, :]).sum(axis=1)
    e = sn * (X * w[:, None]).sum(axis=0)
    var = sn * (X * X).sum(axis=0)
    md = (al * e).sum()
    logdet = np.log(np.diag(R)).sum()
    log2pi = LOG2PI_LD if dtype is LD else dtype(math.log(2.0 * math.pi))
    logp = -md / 2 - (s * np.log(sn) - 2 * logdet) / 2 - s * log2pi / 2
    beta = sn / (1 + np.sqrt(1 + sn * (w * w).sum()))
    Q = np.sqrt(sn) * X.T + (beta / np.sqrt(sn)) * e[:, None] * w[None, :]
    return {"e": e, "mean": yy - e, "var": var, "logp": logp, "gsum": np.array([(e * e).sum(), (e * e / var).sum(), md]),
            "Q": Q, "w": w, "X": X, "R": R}


SOLVE_OUTPUTS = ("e", "var", "logp", "gsum", "Q")


def solve_scale(ref, s, kappa):
    """per output: (s + 2) u kappa_2(S) max|ref| -- gsum entry by entry; the bound is c times this"""
    f = (s + 2) * U * kappa
    return {k: f * (np.abs(ref[k]).astype(np.float64) if k == "gsum" else float(np.abs(ref[k]).max())) for k in SOLVE_OUTPUTS}


class SolveCase:
    """S of every group: the long-double Gram of gram_case() rounded to double.  alpha, y: Np-vectors."""

    def __init__(self):
        gc = gram_case()
        self.Np, self.groups, self.sn2 = gc.Np, gc.groups, SOLVE_SN2
        rng = np.random.default_rng(515)
        self.alpha, self.y = rng.standard_normal(self.Np), rng.standard_normal(self.Np)
        self.S = [np.asarray(S, dtype=np.float64) for S, _, _ in gc.ref]
        self.kappa = [float(np.linalg.cond(S)) for S in self.S]
        self.ref = [solve_ref(S, self.alpha[I], self.y[I], self.sn2) for S, I in zip(self.S, self.groups)]
        self.scale = [solve_scale(r, len(I), k) for r, I, k in zip(self.ref, self.groups, self.kappa)]
        # c: the next power of two above 8 times the worst ratio of the float64 restatement over these groups
        self.f64_ratio = 0.0
        for S, I, r, sc in zip(self.S, self.groups, self.ref, self.scale):
            f = solve_ref(S, self.alpha[I], self.y[I], self.sn2, dtype=np.float64)
            self.f64_ratio = max([self.f64_ratio] + [worst(f[k].astype(LD) - r[k], sc[k]) for k in SOLVE_OUTPUTS])
        self.c = 2.0 ** (math.floor(math.log2(8 * self.f64_ratio)) + 1)
        # the failing pivots: one diagonal entry lowered to half of what the columns to its left take away from it
        self.S_fail = {}
        for g, col in SOLVE_FAIL.items():
            S = self.S[g].copy()
            R = self.ref[g]["R"]
            S[col, col] = float(0.5 * (R[col, :col] * R[col, :col]).sum())
            assert solve_ref(S, self.alpha[self.groups[g]], self.y[self.groups[g]], self.sn2) is None
            self.S_fail[g] = S

    def bound(self, g, k):
        return self.c * self.scale[g][k]

    def mean_bound(self, g):
        """mean = y - e: e's bound and one more rounding"""
        return self.bound(g, "e") + U * np.abs(self.ref[g]["mean"]).astype(np.float64)

    def c_ref(self, g):
        """C = sn2 S^-1 + e e' in long double: what Q Q' is held to, within c (s + 2) u kappa max|C|"""
        r = self.ref[g]
        C = LD(self.sn2) * dc.mm_ld(np.ascontiguousarray(r["X"].T), np.ascontiguousarray(r["X"].T)) + np.outer(r["e"], r["e"])
        return C, self.c * (len(self.groups[g]) + 2) * U * self.kappa[g] * float(np.abs(C).max())

    def wrong(self, g):
        """two members swapped: alpha of the first and the last member exchanged"""
        I = self.groups[g].copy()
        I[[0, -1]] = I[[-1, 0]]
        return solve_ref(self.S[g], self.alpha[I], self.y[self.groups[g]], self.sn2)


_SOLVE = []


def solve_case():
    if not _SOLVE:
        _SOLVE.append(SolveCase())
    return _SOLVE[0]


def s_buffer(S_list, sent):
    """the S of the groups as the solve reads them, one after the other: the lower triangle of each s x s block, `sent`
    (a NaN) everywhere else -- above the diagonal and on the padding, which the solve must not read"""
    out = []
    for S in S_list:
        s = S.shape[0]
        sp = pad16(s)
        B = np.full((sp, sp), sent)
        low = np.tril(np.ones((s, s), dtype=bool))
        B[:s, :s][low] = S[low]
        out.append(B.T.ravel())                                        # column-major
    return np.concatenate(out)


MIX_NP = 384
MIX_WIDTHS = (1, 15, 16, 17, 127, 128)


class MixCase:
    """bins over scattered and contiguous columns of a 384 x 384 H: the bins of 128 and 16 are runs of consecutive columns
    (0 .. 127, 128 .. 143), the others sorted random picks among the remaining 240 columns, 80 of which stay in no bin"""

    def __init__(self):
        rng = np.random.default_rng(77)
        self.Np = MIX_NP
        self.H = rng.standard_normal((self.Np, self.Np))
        rest = rng.permutation(np.arange(144, self.Np))
        self.cols, at = [], 0
        for w in MIX_WIDTHS:
            if w == 128:
                c = np.arange(128)
            elif w == 16:
                c = 128 + np.arange(16)
            else:
                c, at = np.sort(rest[at:at + w]), at + w
            self.cols.append(c.astype(np.int32))
        self.Q = [rng.standard_normal((w, w)) for w in MIX_WIDTHS]
        self.perm = np.concatenate(self.cols).astype(np.int32)
        self.bstart = np.concatenate([[0], np.cumsum(MIX_WIDTHS)]).astype(np.int32)

    def expect(self, b, cols=None):
        """(ref, bound) of H[:, cols_b] Q_b: width terms per element"""
        Hc = self.H[:, self.cols[b] if cols is None else cols]
        return dc.mm_ld(Hc, np.ascontiguousarray(self.Q[b].T)), (MIX_WIDTHS[b] + 2) * U * (np.abs(Hc) @ np.abs(self.Q[b]))

    def wrong(self, b):
        """two members swapped in the bin's list; a bin of one column: the neighbouring column used"""
        c = self.cols[b].copy()
        if len(c) == 1:
            c[0] += 1
        else:
            c[[0, -1]] = c[[-1, 0]]
        return self.expect(b, c)[0]


_MIX = []


def mix_case():
    if not _MIX:
        _MIX.append(MixCase())
    return _MIX[0]


# ------------------------------------------------------------------------------------------------------------------------
# the stages of a one-at-a-time fold
# ------------------------------------------------------------------------------------------------------------------------
FOLD_M = (129, 257, 300, 640)
FOLD_NP = 768             # the samples the members are drawn from
FOLD_SN2 = 0.21
GATHER_NP = 640           # 512 + a ragged 128-row chunk


class FoldCase:
    """One group of m members (sorted, scattered over 768 samples).  T: upper triangular m x m, `NAN` everywhere else of
    m_p x m_p -- below the diagonal and on the padding, none of which a stage may read.  Every stage has inputs of its own
    (w, e, var are drawn, not chained), so that its reference does not lean on another kernel."""

    def __init__(self, m):
        rng = np.random.default_rng(9000 + m)
        self.m, self.mp, self.sn2 = m, pad128(m), FOLD_SN2
        self.rows = np.sort(rng.choice(FOLD_NP, m, replace=False)).astype(np.int32)
        self.alpha, self.y = rng.standard_normal(FOLD_NP), rng.standard_normal(FOLD_NP)
        self.T = np.full((self.mp, self.mp), NAN)
        up = np.triu(np.ones((m, m), dtype=bool))
        self.T[:m, :m][up] = upper_factor(m, 9100 + m)[up]
        self.Tz = np.where(np.isnan(self.T), 0.0, self.T)[:m, :m]     # T with its structural zeros, for the references
        self.wv, self.ev = rng.standard_normal(m), rng.standard_normal(m)
        self.vv = rng.uniform(0.5, 2.0, m)
        self.rdiag = rng.uniform(0.5, 2.0, m)                        # the diagonal of R; the rest of R is NAN
        self.sc = np.array([math.sqrt(self.sn2), 0.4321])

    # every expect_* returns {output: (ref, bound)}
    def expect_w(self, shift=0):
        """w_j = sum_{i <= j} T_ij alpha_rows[i]: j + 1 terms.  shift: the wrong kernel that reads alpha a row further on"""
        a = self.alpha[np.minimum(self.rows + shift, FOLD_NP - 1)]
        ref = dc.mv_ld(self.Tz.T, a)
        n = np.arange(self.m) + 1
        return {"wv": (ref, (n + 2) * U * (np.abs(self.Tz).T @ np.abs(a)))}

    def expect_ev(self, shift=0):
        """e_i, var_i: m - i terms and the product with sn2; mean = y - e: one more rounding.  shift: w a neighbour on"""
        w = np.roll(self.wv, shift)
        n = self.m - np.arange(self.m)
        e = LD(self.sn2) * dc.mv_ld(self.Tz, w)
        v = LD(self.sn2) * (self.Tz.astype(LD) ** 2).sum(axis=1)
        be = (n + 2) * U * self.sn2 * (np.abs(self.Tz) @ np.abs(w))
        bv = (n + 2) * U * self.sn2 * (self.Tz ** 2).sum(axis=1)
        mean = self.y[self.rows].astype(LD) - e
        return {"ev": (e, be), "vv": (v, bv), "mean": (mean, be + U * np.abs(mean).astype(np.float64)), "var": (v, bv)}

    def expect_sums(self, swap=False):
        """The three sums over m terms: (m + 2) u sum|terms| and, for e^2 / var, two roundings inside every term.  logp: the
        bounds of its parts, 2 ulp = 4 u per evaluation of the device's log (AN ASSUMPTION about that function, the one
        the suite makes of it elsewhere), and four roundings of the final expression on the magnitudes it adds.
        swap: the wrong kernel that takes alpha of two members the other way round"""
        m, sn = self.m, LD(self.sn2)
        e, v, r = self.ev.astype(LD), self.vv.astype(LD), self.rdiag.astype(LD)
        rows = self.rows.copy()
        if swap:
            rows[[0, -1]] = rows[[-1, 0]]
        a = self.alpha[rows].astype(LD)
        sse, ssr, md, ld = (e * e).sum(), (e * e / v).sum(), (a * e).sum(), np.log(r).sum()
        f = (m + 2) * U
        b_sse, b_ssr = f * float(sse), (f + 2 * U) * float(ssr)
        b_md = f * float((np.abs(a) * np.abs(e)).sum())
        b_ld = (f + 4 * U) * float(np.abs(np.log(r)).sum())
        logp = -md / 2 - (m * np.log(sn) - 2 * ld) / 2 - m * LOG2PI_LD / 2
        mag = float(abs(md) / 2 + m * abs(np.log(sn)) / 2 + abs(ld) + m * LOG2PI_LD / 2)
        b_logp = b_md / 2 + b_ld + 4 * U * m * float(abs(np.log(sn))) / 2 + 4 * U * mag
        return {"gsum": (np.array([sse, ssr, md]), np.array([b_sse, b_ssr, b_md])), "logp": (logp, b_logp)}

    def expect_beta(self, drop=False):
        """sc[0] = sqrt(sn2), correctly rounded: exact.  sc[1] = g(|w|^2), |d log g / d log |w|^2| < 1/2, so half the relative
        bound (m + 2) u of |w|^2, and six roundings: the fma, two square roots, the sum and two quotients.
        drop: the wrong kernel that leaves the last w out"""
        w = self.wv.astype(LD)[:-1] if drop else self.wv.astype(LD)
        sn = LD(self.sn2)
        s1 = sn / (1 + np.sqrt(1 + sn * (w * w).sum())) / np.sqrt(sn)
        return {"sc0": (LD(np.sqrt(np.float64(self.sn2))), 0.0), "sc1": (s1, ((self.m + 2) / 2 + 6) * U * float(s1))}

    def expect_q(self, transposed, shift=0):
        """Q_ij = sc0 T_ij + (sc1 e_i) w_j: three roundings -- sc1 e_i, sc0 T_ij and the fused sum -- each on a magnitude below
        |sc0 T_ij| + |sc1 e_i w_j|.  Exact +0 on the rest of m_p x m_p.  shift: the wrong kernel that reads e a row on"""
        m, mp = self.m, self.mp
        e = np.roll(self.ev, shift)
        A, B = LD(self.sc[0]) * self.Tz.astype(LD), LD(self.sc[1]) * np.outer(e.astype(LD), self.wv.astype(LD))
        ref, bnd = np.zeros((mp, mp), dtype=LD), np.zeros((mp, mp))
        ref[:m, :m] = A + B
        bnd[:m, :m] = 3 * U * (np.abs(A) + np.abs(B)).astype(np.float64)
        return {"Q": (ref.T, bnd.T) if transposed else (ref, bnd)}


_FOLD = {}


def fold_case(m):
    if m not in _FOLD:
        _FOLD[m] = FoldCase(m)
    return _FOLD[m]


# ------------------------------------------------------------------------------------------------------------------------
# leave-one-out
# ------------------------------------------------------------------------------------------------------------------------
LOO_NP, LOO_N = 1152, 1100        # chunks of 512 + 512 + 128 columns
LOO_SN2 = 0.29
LOO_CHUNK = 512


def loo_tiles(Np, P, a):
    return [g for g in range(Np // TILE) if g % P == a]


def rowsumsq_ref(G):
    """d_i = sum_{k >= i} G_ik^2 in long double and its bound (n - i + 2) u sum_k G_ik^2"""
    n = G.shape[0]
    T = np.triu(G)
    return (T.astype(LD) ** 2).sum(axis=1), (n - np.arange(n) + 2) * U * (T ** 2).sum(axis=1)


def finish_ref(d, y, alpha, sn2):
    """var = sn2 / d: one rounding.  mean = y - alpha var, fused or not: var's rounding and the product's on |alpha var|,
    the difference's on |mean|.  The kernel then forms r = y - mean (exact in long double: alpha var) with the error of
    mean and one rounding of its own, and adds r^2, r^2 / var and log var over the N rows: per term the propagated
    error (two roundings more for r^2 / var, 4 u for the device's log -- the assumption of the fold stages -- and u for
    its argument), then (N + 2) u sum|terms| for the additions."""
    N = len(d)
    d, y, a, sn = np.asarray(d).astype(LD), np.asarray(y).astype(LD), np.asarray(alpha).astype(LD), LD(sn2)
    var = sn / d
    av = a * var
    mean = y - av
    f64 = lambda x: np.abs(x).astype(np.float64)      # noqa: E731
    b_var = U * f64(var)
    b_mean = 2 * U * f64(av) + U * f64(mean)
    dr = b_mean + U * f64(av)
    t0, t1, t2 = av * av, av * av / var, np.log(var)
    e0 = 2 * f64(av) * dr + U * f64(t0)
    e1 = e0 / f64(var) + 3 * U * f64(t1)
    e2 = U + 4 * U * f64(t2)
    f = (N + 2) * U
    sums = np.array([t0.sum(), t1.sum(), t2.sum()])
    b_sums = np.array([e0.sum() + f * f64(t0).sum(), e1.sum() + f * f64(t1).sum(), e2.sum() + f * f64(t2).sum()])
    return {"var": (var, b_var), "mean": (mean, b_mean), "sums": (sums, b_sums)}


class LooCase:
    def __init__(self):
        rng = np.random.default_rng(4242)
        self.Np, self.N, self.sn2 = LOO_NP, LOO_N, LOO_SN2
        self.G = upper_factor(self.Np, 4243)
        self.alpha, self.y = rng.standard_normal(self.Np), rng.standard_normal(self.Np)
        self.alpha[self.N:] = 0.0                                      # as the library keeps it on the padding
        self.d_ld, self.d_bound = rowsumsq_ref(self.G)
        self.d = self.d_ld.astype(np.float64)                          # the input of the later stages
        B = rng.standard_normal((self.Np, self.Np))
        self.Binv = np.tril(B) + np.tril(B, -1).T                      # symmetric; the device buffer holds its lower tiles
        self.s, self.v = rng.standard_normal(self.Np), rng.standard_normal(self.Np)
        self.s[self.N:] = 0.0
        self.v[self.N:] = 0.0
        self.W = rng.standard_normal((self.Np, self.Np))

    def slab(self, P, a):
        """rows of pass a of P; NAN in every 512-column chunk strictly left of each row block's diagonal block"""
        tiles = loo_tiles(self.Np, P, a)
        out = np.concatenate([self.G[g * TILE:(g + 1) * TILE] for g in tiles])
        for t, g in enumerate(tiles):
            out[t * TILE:(t + 1) * TILE, :g * TILE // LOO_CHUNK * LOO_CHUNK] = NAN
        rows = np.concatenate([np.arange(g * TILE, (g + 1) * TILE) for g in tiles])
        return out, rows

    def d_wrong(self):
        """a neighbouring row used: d of row i + 1 at row i"""
        return np.roll(self.d_ld, -1)

    def expect_finish(self, shift=0):
        """finish_ref on the case's d, y and alpha.  shift: the wrong kernel that reads alpha a row on"""
        N = self.N
        return finish_ref(self.d[:N], self.y[:N], np.roll(self.alpha, -shift)[:N], self.sn2)
    def expect_vectors(self, shift=0):
        """ik = sn2 / d (u), b = alpha ik (2 u), c = (ik + b^2) / 2: both terms positive, b^2 within 5 u fused or not, so c
        within 6 u; its square root 3 u and one more, the quotient by sn2 one more: s within 5 u -- stated as 6 u.  r = b /
        sn2: 3 u.  Zeros from N on.  shift: the wrong kernel that reads alpha a row on"""
        N, Np = self.N, self.Np
        d, a, sn = self.d[:N].astype(LD), np.roll(self.alpha, -shift)[:N].astype(LD), LD(self.sn2)
        ik = sn / d
        b = a * ik
        s, r = np.zeros(Np, dtype=LD), np.zeros(Np, dtype=LD)
        s[:N], r[:N] = np.sqrt((ik + b * b) / 2) / sn, b / sn
        return {"s": (s, 6 * U * np.abs(s).astype(np.float64)), "r": (r, 3 * U * np.abs(r).astype(np.float64))}

    def expect_mirror(self):
        """every entry ONE IEEE product: the bits of s_k * Binv[max(i, k), min(i, k)]; exact zeros from N on"""
        N = self.N
        H = self.Binv * self.s[None, :]
        H[N:, :] = 0.0
        H[:, N:] = 0.0
        return H

    def expect_rank2(self, shift=0):
        """W - (v_i a_j + a_i v_j): the product a_i v_j, the fused sum and the difference, three roundings each below
        |W| + |v_i a_j| + |a_i v_j| (to first order).  shift: the wrong kernel that reads v a row on"""
        v, a = np.roll(self.v, -shift).astype(LD), self.alpha.astype(LD)
        va, av = np.outer(v, a), np.outer(a, v)
        ref = self.W.astype(LD) - (va + av)
        return ref, 3 * U * (np.abs(self.W) + np.abs(va).astype(np.float64) + np.abs(av).astype(np.float64))


_LOO = []


def loo_case():
    if not _LOO:
        _LOO.append(LooCase())
    return _LOO[0]


def lower_tiles(n, tile):
    """n x n boolean: the tile x tile tiles on and below the diagonal tiles"""
    t = np.arange(n) // tile
    return t[:, None] >= t[None, :]
