"""TEST INFRASTRUCTURE: every gpak_dev_* operation (include/gpak_dev.h, the vector pieces of include/gpak_dist.h) ALONE
against a long-double reference -- the cases, independent of the engine that runs them.

A case is a function over an `ops` object whose one method, `call(name, *args)`, takes the arguments of
`gpak_dev_<name>` after the stream (NumPy arrays for pointers) and returns the status.  `HipOps` uploads with torch,
calls libgpak_hip.so through ctypes and downloads; `NumpyOps` runs the same call on the float64 restatements of
tests/np_engine.py / tests/np_dist_engine.py.  A case builds its inputs from a fixed seed, calls ONE operation and
hands back, per output buffer: what came back, a reference in np.longdouble, an elementwise bound, and which elements
must come back bit-identical (everything the operation has no business writing).

Every checked buffer carries a guard band of 256 doubles on either side and every leading dimension is skewed
(ld = rows + 32, 34, 36 ...: never equal to the row count or to each other; the `grad` group's packed panels and slabs
have the leading dimension their interface fixes); guard bands and skew rows hold a
sentinel bit pattern (a NaN with a payload) and belong to the bit-identical set.  Operands are dense standard_normal
unless the case says otherwise: not kernel matrices, so a permuted fragment or a wrong tile is an O(1) error.

Bounds (u = 2^-53):
  * products and sums: (n + 2) u sum|terms| -- holds for ANY order of accumulation, fused or not;
  * logdiag adds 4 u sum|log L_cc| for the device's log;
  * fill / Gram mat-vec: the tolerances of test_gram_matches_oracle against the CPU oracle, scaled by 1/sn2;
  * substitutions (trsv_*, solve_rows, diag_inverse, grad_g_rows) multiply by explicit inverses of 128 x 128 blocks, so no clean
    forward bound exists: 8 x the largest error of NumpyOps (the float64 restatement of the same blocked algorithm, run
    on the same inputs, the device's own factor included) against the long-double solution, elementwise relative to
    |L^-1| |b| in long double.  The 8 covers another accumulation order in an algorithm with the same first-order error.

Long-double products of float64 operands are formed from exact pieces: each operand is cut into 17-bit slices per row
(integers times a power of two), a float64 BLAS product of two slices with K <= 2048 is exact (17 + 17 + 11 < 53 bits)
in any order, and the slice products are summed in long double, smallest first (`mm_ld`; test_dev_ops holds it against
NumPy's own long-double matmul).
"""
import ctypes as C
import os
import re
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TILE = 128
GUARD = 256
U = 2.0 ** -53
LD = np.longdouble
SENTINEL = np.uint64(0x7FF8A5A5DEADBEEF)     # a quiet NaN with a payload: arithmetic on it shows, a copy keeps it
OK, EINVAL = 0, 2
INT_MAX = 0x7FFFFFFF
D4, HYB = 0x10, 0x20
GROUPS = ("gemm", "solve_rows", "trsv", "reduce", "fill", "grad")


def long_double_ok():
    return np.finfo(np.longdouble).eps < 1e-18


def sentinel(n):
    return np.full(int(n), SENTINEL, dtype=np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Mat:
    """rows x cols column-major doubles with leading dimension ld inside a guarded buffer; the skew rows hold the
    sentinel.  `before` is the payload as it went in."""

    def __init__(self, M, ld=None):
        M = np.asarray(M, dtype=np.float64)
        if M.ndim == 1:
            M = M[:, None]
        self.rows, self.cols = M.shape
        self.ld = int(ld) if ld is not None else self.rows
        body = sentinel(self.cols * self.ld).reshape(self.cols, self.ld)
        body[:, :self.rows] = M.T
        self.full = np.concatenate([sentinel(GUARD), body.ravel(), sentinel(GUARD)])
        self.n = self.cols * self.ld
        self.before = self.data.copy()

    @property
    def data(self):
        return self.full[GUARD:GUARD + self.n]

    def get(self):
        return self.data.reshape(self.cols, self.ld).T[:self.rows]          # rows x cols view

    def was(self):
        return self.before.reshape(self.cols, self.ld).T[:self.rows]

    def guards_ok(self):
        f = bits(self.full)
        return bool((f[:GUARD] == SENTINEL).all() and (f[GUARD + self.n:] == SENTINEL).all())

    def lift(self, m2d):
        """rows x cols boolean -> mask over the payload (False in the skew rows)"""
        f = np.zeros((self.cols, self.ld), dtype=bool)
        f[:, :self.rows] = np.broadcast_to(m2d, (self.rows, self.cols)).T
        return f.ravel()


class Check:
    """One output buffer of a case.  cmp: elements held against ref within bound; free: elements the header calls
    scratch / intermediates; every other element of the payload must come back bit-identical."""

    def __init__(self, label, mat, ref=None, bound=None, cmp=None, free=None):
        self.label, self.mat = label, mat
        shape = (mat.rows, mat.cols)
        self.cmp = np.zeros(shape, dtype=bool) if cmp is None else np.broadcast_to(np.asarray(cmp, dtype=bool), shape)
        self.free = np.zeros(shape, dtype=bool) if free is None else np.broadcast_to(np.asarray(free, dtype=bool), shape)
        self.ref = None if ref is None else np.broadcast_to(self._2d(ref, LD), shape)
        self.bound = None if bound is None else np.broadcast_to(self._2d(bound, np.float64), shape)

    @staticmethod
    def _2d(v, dtype):
        v = np.asarray(v, dtype=dtype)
        return v.reshape(-1, 1) if v.ndim < 2 else v

    def ratio(self):
        """worst |out - ref| / bound over the compared elements (inf for a NaN or an error where the bound is 0)"""
        if not self.cmp.any():
            return 0.0
        out = self.mat.get()[self.cmp].astype(LD)
        err = np.abs(out - self.ref[self.cmp]).astype(np.float64)
        b = self.bound[self.cmp]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / b)
        r[~np.isfinite(err)] = np.inf
        return float(r.max())

    def violations(self):
        same = ~(self.mat.lift(self.cmp) | self.mat.lift(self.free))
        return int(np.count_nonzero(bits(self.mat.data)[same] != bits(self.mat.before)[same]))


class Result:
    def __init__(self):
        self.checks, self.rcs, self.info = [], [], {}

    def rc(self, label, got, want=OK):
        self.rcs.append((label, int(got), int(want)))
        return self

    def add(self, *a, **k):
        self.checks.append(Check(*a, **k))
        return self


# ------------------------------------------------------------------------------------------------
# long-double arithmetic on float64 operands
# ------------------------------------------------------------------------------------------------
def _slices(A, ns):
    A = np.asarray(A)
    R = A.astype(LD) if A.dtype == LD else A.astype(np.float64)
    amax = np.abs(R).max(axis=1).astype(np.float64)
    e = np.frexp(np.where(amax > 0, amax, 1.0))[1].astype(np.int64)[:, None] + 1      # |a| < 2^e in every row
    out = []
    for s in range(ns):
        sh = e - 17 * (s + 1)
        q = np.ldexp(np.rint(np.ldexp(R, -sh)), sh)      # the leading bits of R: an integer |.| <= 2^17 times 2^sh
        R = R - q                                        # exact
        out.append(np.ascontiguousarray(q, dtype=np.float64))
    return out


def mm_ld(A, B):
    """A @ B.T in long double (A: m x K, B: n x K, float64 or long double, K <= 2048): see the module docstring.  What
    is left out is below 2^-64 of (row maximum of A) x (row maximum of B) per term."""
    assert A.shape[1] == B.shape[1] and A.shape[1] <= 2048
    ns = 5 if (np.asarray(A).dtype == LD or np.asarray(B).dtype == LD) else 4
    sa, sb = _slices(A, ns), _slices(B, ns)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for lvl in range(ns - 1, -1, -1):
        for i in range(lvl + 1):
            acc += sa[i] @ sb[lvl - i].T
    return acc


def mv_ld(A, x):
    """A @ x in long double, plainly (for the small ones)"""
    return np.asarray(A, dtype=LD) @ np.asarray(x, dtype=LD)


def tri_inv_ld(L):
    """inverse of a lower-triangular float64 matrix in long double, by forward substitution"""
    W = L.shape[0]
    Ll = np.tril(L).astype(LD)
    X = np.zeros((W, W), dtype=LD)
    for i in range(W):
        row = -(Ll[i, :i] @ X[:i, :i + 1]) if i else np.zeros(1, dtype=LD)
        row[i] += 1.0
        X[i, :i + 1] = row / Ll[i, i]
    return X


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------
# the two adaptors
# ------------------------------------------------------------------------------------------------
# arguments of gpak_dev_<name> after the stream: p device pointer, i int, l long, d double, h host double array,
# P host array of device pointers (a list here)
SIG = {
    "transform": "piiihhp", "transform_k": "piiihihp", "fill_b": "piiiiihddipl", "fill_rect": "piiiiiihddipl",
    "factor_panel": "pliiipp", "factor_panel_co": "pliiippi", "update_block": "pliipliii", "update_cyclic": "pliipliiiiiii",
    "update_rect": "plplipliii", "solve_rows": "pliiplp", "trsv_fwd_block": "pliiippp", "coldot": "pliiipp",
    "trsv_bwd_block": "pliippp", "trsv_bwd_packed": "pliiiippppp", "diag_inverse": "pliiipp", "logdiag_block": "pliiip",
    "kmatvec": "piiiiphdipp", "nlz_terms": "ipppdp", "pack": "pliiip", "gemv_n_add": "pliipp", "gemv_t": "pliipp",
    "vec_axpy": "idpp", "vec_scale": "ipdp", "vec_sum": "ipp", "grad_g_rows": "iiiiPPp", "grad_binv_rows": "iiiippp",
}


def precheck(name, a):
    """The argument rules of include/gpak_dev.h, restated for the NumPy side: a status to return without doing
    anything, or None."""
    if name == "pack":
        _src, ld, row0, nrows, ncols, _dst = a
        if nrows <= 0 or ncols <= 0:
            return OK
        return EINVAL if (nrows | row0 | ld) & 1 else None
    if name == "trsv_bwd_packed":
        W = a[5]
        return EINVAL if W <= 0 or W > 512 or W % TILE else None
    if name == "diag_inverse":
        W = a[4]
        return EINVAL if W <= 0 or W > 512 or W % TILE or a[6] is None else None
    if name == "fill_rect":
        nrows, ncols = a[4], a[6]
        if nrows <= 0 or ncols <= 0:
            return OK
        return EINVAL if nrows % TILE or ncols % 64 else None
    if name == "solve_rows":
        nrows, W = a[2], a[3]
        if nrows <= 0:
            return OK
        return EINVAL if nrows % TILE or W <= 0 or W % TILE or W > 512 else None
    if name == "update_rect":
        K, mrows, ncols = a[4], a[7], a[8]
        if mrows <= 0 or ncols <= 0:
            return OK
        return EINVAL if mrows % TILE or ncols % TILE or K % TILE else None
    if name == "gemv_n_add":
        nrows, W = a[2], a[3]
        if nrows <= 0 or W <= 0:
            return OK
        return EINVAL if W > 512 else None
    if name == "gemv_t":
        return OK if a[3] <= 0 else None
    if name == "grad_binv_rows":
        P, ra, rb = a[1], a[2], a[3]
        return EINVAL if ra < 0 or ra >= P or rb < 0 or rb >= P else None
    if name == "update_cyclic":
        nb, lb0, n_local, last_width = a[7], a[10], a[11], a[12]
        return OK if (n_local - 1) * (nb // TILE) + last_width // TILE - lb0 * (nb // TILE) <= 0 else None
    return None


def _buf(x):
    return x.full if isinstance(x, Mat) else x


class NumpyOps:
    """The float64 restatement: the callbacks of NumpyDistEngine (they have the C signatures of gpak_dev_*), and
    NumpyEngine for the two operations the C++ schedules do not use."""
    name = "numpy"

    def __init__(self):
        import torch
        from np_dist_engine import NumpyDistEngine
        self.torch = torch
        self.nde = NumpyDistEngine(poison_upper=False)
        self.eng = self.nde.np

    @staticmethod
    def _ptr(x):
        if x is None:
            return None
        if isinstance(x, Mat):
            return x.full.ctypes.data + 8 * GUARD
        return x.ctypes.data

    def _t(self, x):
        return self.torch.from_numpy(x.data if isinstance(x, Mat) else x)

    def call(self, name, *a):
        assert len(a) == len(SIG[name]), name
        rc = precheck(name, a)
        if rc is not None:
            return rc
        if name == "coldot":
            blk, ld, Np, J, W, x, s = a
            self.eng.coldot(self._t(blk), ld, Np, J, W, self._t(x), self._t(s))
            return OK
        if name == "trsv_bwd_block":
            blk, ld, J, W, inv, x, out = a
            self.eng.trsv_bwd_block(self._t(blk), ld, J, W, self._t(inv), self._t(x), self._t(out))
            return OK
        if name == "factor_panel_co":
            name, a = "factor_panel", a[:-1]
        conv = []
        for kind, v in zip(SIG[name], a):
            if kind == "p":
                conv.append(self._ptr(v))
            elif kind == "P":
                conv.append((C.c_void_p * len(v))(*[self._ptr(x) for x in v]))
            elif kind == "h":
                conv.append((C.c_double * len(v))(*[float(t) for t in v]))
            else:
                conv.append(v)
        return int(self.nde._keep[name](None, *conv))


class HipOps:
    """libgpak_hip.so on the device: HipEngine for the library, the device and the stream; every call uploads its
    arrays, runs, synchronises and downloads them again (guard bands included)."""
    name = "hip"
    _ct = {"p": C.c_void_p, "i": C.c_int, "l": C.c_long, "d": C.c_double, "h": C.POINTER(C.c_double), "P": C.POINTER(C.c_void_p)}

    def __init__(self):
        from py_schedule import HipEngine
        self.eng = HipEngine(0)
        self.lib = self.eng.lib

    def call(self, name, *a):
        assert len(a) == len(SIG[name]), name
        fn = getattr(self.lib, "gpak_dev_" + name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [self._ct[k] for k in SIG[name]]
        dev, conv, keep = {}, [], []

        def ptr(v):
            if id(v) not in dev:
                dev[id(v)] = (v, self.eng.from_numpy(_buf(v)))
            return dev[id(v)][1].data_ptr() + (8 * GUARD if isinstance(v, Mat) else 0)

        for kind, v in zip(SIG[name], a):
            if kind == "p":
                conv.append(None if v is None else ptr(v))
            elif kind == "P":
                keep.append((C.c_void_p * len(v))(*[ptr(x) for x in v]))
                conv.append(keep[-1])
            elif kind == "h":
                keep.append((C.c_double * len(v))(*[float(t) for t in v]))
                conv.append(keep[-1])
            else:
                conv.append(v)
        rc = int(fn(self.eng._st(), *conv))
        self.eng.sync()                     # a fault surfaces here and ends the worker
        for v, t in dev.values():
            _buf(v)[...] = t.cpu().numpy()
        return rc


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
CASES = []          # (group, name, entry points, function of ops -> Result)


def case(group, name, entries, **kw):
    def deco(fn):
        CASES.append((group, name, tuple(entries), (lambda ops, fn=fn, kw=kw, name=name: fn(ops, name, **kw))))
        return fn
    return deco


def covered_entry_points():
    return sorted({e for _g, _n, ents, _f in CASES for e in ents})


def declared_entry_points():
    """every gpak_dev_* function include/gpak_dev.h declares, and the vector pieces of include/gpak_dist.h"""
    names = set()
    for h in ("gpak_dev.h", "gpak_dist.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            names |= set(re.findall(r"^int (gpak_dev_\w+)\(", f.read(), flags=re.M))
    return sorted(names)


_NUMPY = []


def numpy_ops():
    if not _NUMPY:
        _NUMPY.append(NumpyOps())
    return _NUMPY[0]


_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def tile_rows(mask_tiles):
    """tiles (mt x nt boolean) -> elements"""
    return np.kron(mask_tiles, np.ones((TILE, TILE), dtype=bool))


# ---- GEMM family -----------------------------------------------------------------------------------
def gemm_expect(key, A, B, C0, tiles):
    """C0 - A B^T on the tiles that take part: reference, bound (K + 2) u (|A| |B|^T + |C0|), element mask"""
    prod, aprod = memo(("gemm", key), lambda: (mm_ld(A, B), np.abs(A) @ np.abs(B).T))
    K = A.shape[1]
    cmp = tile_rows(tiles)
    return C0.astype(LD) - prod, (K + 2) * U * (aprod + np.abs(C0)), cmp


def _update_block(ops, name, Np, Jc, Wc, W, prow0):
    rng = rng_for(name)
    ld, ldp = Np + 32, Np - prow0 + 34
    panel = Mat(rng.standard_normal((Np - prow0, W)), ldp)
    blk = Mat(rng.standard_normal((Np, Wc)), ld)
    res = Result().rc("update_block", ops.call("update_block", panel, ldp, prow0, W, blk, ld, Np, Jc, Wc))
    a = panel.was()[Jc - prow0:]
    mt, nt = (Np - Jc) // TILE, Wc // TILE
    tiles = np.arange(mt)[:, None] >= np.arange(nt)[None, :]            # lower tiles of the trapezoid
    ref, bound, cmp = gemm_expect(name, a, a[:Wc], blk.was()[Jc:], tiles)
    full = lambda x, fill: np.concatenate([np.full((Jc, Wc), fill, dtype=x.dtype), x])
    res.add("blk", blk, full(ref, 0), full(bound, 0), full(cmp, False))
    return res.add("panel", panel)


for _Np, _Jc, _Wc, _W, _p0 in ((1280, 128, 1152, 128, 128), (1280, 128, 1152, 512, 128), (1280, 1152, 128, 256, 128),
                               (384, 0, 256, 1024, 0)):
    case("gemm", f"update_block[Np={_Np},Jc={_Jc},Wc={_Wc},W={_W}]", ["gpak_dev_update_block"], Np=_Np, Jc=_Jc, Wc=_Wc,
         W=_W, prow0=_p0)(_update_block)


def _update_rect(ops, name, m, n, K, diag_first, want=OK):
    rng = rng_for(f"update_rect[{m},{n},{K}]")          # both diag_first variants share operands and reference
    lda, ldb, ldc = m + 32, n + 34, m + 36
    A, B = Mat(rng.standard_normal((m, K)), lda), Mat(rng.standard_normal((n, K)), ldb)
    Cm = Mat(rng.standard_normal((m, n)), ldc)
    res = Result().rc("update_rect", ops.call("update_rect", A, lda, B, ldb, K, Cm, ldc, m, n, diag_first), want)
    if want == OK and m > 0:
        mt, nt = m // TILE, n // TILE
        tiles = (np.arange(mt)[:, None] >= np.arange(nt)[None, :]) if diag_first else np.ones((mt, nt), dtype=bool)
        ref, bound, cmp = gemm_expect(f"update_rect[{m},{n},{K}]", A.was(), B.was(), Cm.was(), tiles)
        res.add("C", Cm, ref, bound, cmp)
    else:
        res.add("C", Cm)                                  # a refusal or a no-op writes nothing
    return res.add("A", A).add("B", B)


for _m, _n, _K in ((1152, 384, 128), (256, 1152, 512), (640, 384, 2048)):
    for _df in (0, 1):
        case("gemm", f"update_rect[{_m},{_n},{_K},diag_first={_df}]", ["gpak_dev_update_rect"], m=_m, n=_n, K=_K,
             diag_first=_df)(_update_rect)
case("gemm", "update_rect[128,128,128,diag_first=0]", ["gpak_dev_update_rect"], m=128, n=128, K=128, diag_first=0)(_update_rect)
for _m, _n, _K in ((192, 128, 128), (128, 64, 128), (128, 128, 96)):
    case("gemm", f"update_rect[{_m},{_n},{_K}]->EINVAL", ["gpak_dev_update_rect"], m=_m, n=_n, K=_K, diag_first=0,
         want=EINVAL)(_update_rect)
case("gemm", "update_rect[mrows=0]->no-op", ["gpak_dev_update_rect"], m=0, n=128, K=128, diag_first=0)(_update_rect)


def cyclic_layout(Np, nb, P, rank):
    nblocks = (Np + nb - 1) // nb
    owned = [b for b in range(nblocks) if b % P == rank]
    return owned, min(nb, Np - owned[-1] * nb)


def _update_cyclic(ops, name, Np, nb, P, rank, lb0, W=256):
    rng = rng_for(name)
    owned, last_width = cyclic_layout(Np, nb, P, rank)
    n_local = len(owned)
    ncols = (n_local - 1) * nb + last_width
    first = (lb0 * P + rank) * nb if lb0 < n_local else Np
    prow0 = TILE if first >= TILE else 0
    ld, ldp = Np + 32, Np - prow0 + 34
    panel = Mat(rng.standard_normal((Np - prow0, W)), ldp)
    local = Mat(rng.standard_normal((Np, ncols)), ld)
    res = Result().rc("update_cyclic", ops.call("update_cyclic", panel, ldp, prow0, W, local, ld, Np, nb, P, rank, lb0,
                                                n_local, last_width))
    if lb0 >= n_local:
        return res.add("local", local).add("panel", panel)
    Pg = np.zeros((Np, W))
    Pg[prow0:] = panel.was()                                  # by global row
    tpb, T = nb // TILE, Np // TILE
    gct = np.array([(lt // tpb * P + rank) * tpb + lt % tpb for lt in range(ncols // TILE)])
    tiles = (np.arange(T)[:, None] >= gct[None, :]) & (np.arange(ncols // TILE)[None, :] >= lb0 * tpb)
    tiles &= np.arange(T)[:, None] >= (lb0 * P + rank) * tpb
    B = Pg[(gct[:, None] * TILE + np.arange(TILE)[None, :]).ravel()]       # the panel rows of each local column
    ref, bound, cmp = gemm_expect(name, Pg, B, local.was(), tiles)
    return res.add("local", local, ref, bound, cmp).add("panel", panel)


for _Np, _nb, _P, _r, _lb0 in ((1408, 256, 2, 1, 0), (1408, 256, 2, 1, 1), (1408, 256, 3, 0, 1), (1408, 256, 3, 2, 0),
                               (1280, 128, 3, 1, 2), (1408, 256, 2, 1, 3)):
    case("gemm", f"update_cyclic[Np={_Np},nb={_nb},P={_P},rank={_r},lb0={_lb0}]" + ("->no-op" if _lb0 == 3 else ""),
         ["gpak_dev_update_cyclic"], Np=_Np, nb=_nb, P=_P, rank=_r, lb0=_lb0)(_update_cyclic)


# ---- a factored diagonal block, from the engine under test -----------------------------------------
def factored_block(ops, key, W, Np, J, below):
    """Block column [J, J+W) of an Np-row matrix (ld = Np + 32): rows above J hold the sentinel (nothing may read
    them), the diagonal block is G G^T / W + 2 I (condition number of order 10) factored by ONE factor_panel_co call of
    the engine and read back, and the rows below are `below` (untouched by the factorisation: it is told Np = J + W).
    Returns (payload, ld, inv, L).  The factorisation is checked INDIRECTLY here, through the operations that use the
    factor (tests/test_gpu_parity.py::test_block_kernel_directly is its own test); what is checked on the spot is that
    gpak_dev_factor_panel on the same input gives the same bits (it is factor_panel_co(..., 0): csrc/dev_api.hip), the
    run-twice check of the cases for an operation whose result they memoise."""
    def make():
        rng = rng_for(f"factor[{key}]")
        G = rng.standard_normal((W, W))
        ld = Np + 32
        M = np.full((Np, W), np.nan)
        M[:] = sentinel(1)[0]
        M[J:J + W] = G @ G.T / W + 2.0 * np.eye(W)
        if Np > J + W:
            M[J + W:] = below
        blk = Mat(M, ld)
        inv = np.zeros(W // TILE * 2 * TILE * TILE)
        info = np.full(4, INT_MAX, dtype=np.int32)
        blk2, inv2, info2 = Mat(M, ld), np.zeros(inv.size), info.copy()
        rc = ops.call("factor_panel_co", blk, ld, J + W, J, W, inv, info, 0)
        rc2 = ops.call("factor_panel", blk2, ld, J + W, J, W, inv2, info2)
        assert rc == OK and rc2 == OK and info[0] == INT_MAX and info2[0] == INT_MAX, (rc, rc2, info, info2)
        assert blk.guards_ok() and blk2.guards_ok()
        assert np.array_equal(bits(blk.full), bits(blk2.full)) and np.array_equal(bits(inv), bits(inv2)), \
            f"factor_panel and factor_panel_co(..., 0) differ on {key}"
        return blk.data.copy(), ld, inv, np.tril(blk.get()[J:J + W]).copy()
    return memo(("factor", ops.name, key), make)


def subst_bound(res, label, num, ref, scale):
    """The substitution tolerance: 8 x the worst error of the float64 restatement against the long-double solution,
    relative to `scale` = |L^-1| |b|; recorded with the case."""
    scale = np.asarray(scale, dtype=np.float64)
    err = np.abs(np.asarray(num, dtype=LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):      # a structural zero (scale 0) is exact or the case fails
        ratio = float(np.where(err == 0, 0.0, err / scale).max())
    res.info[f"numpy_vs_longdouble[{label}]"] = ratio
    return 8.0 * ratio * scale


# ---- panel solve -------------------------------------------------------------------------------------
def numpy_solve_rows(P, L, inv, W):
    """dev_api.hip's steps in float64: P_s := P_s inv(D_s)^T, P[:, s+1..] -= P_s L[s+1.., s]^T"""
    P = P.copy()
    iv = inv.reshape(W // TILE, 2, TILE, TILE)
    for s in range(W // TILE):
        c = slice(s * TILE, (s + 1) * TILE)
        P[:, c] = P[:, c] @ iv[s, 0]          # memory [c][r] of D^-1 = (D^-1)^T as a C-ordered array
        if (s + 1) * TILE < W:
            P[:, (s + 1) * TILE:] -= P[:, c] @ L[(s + 1) * TILE:, c].T
    return P


def _solve_rows(ops, name, W, nrows, want=OK):
    rng = rng_for(name)
    Wf = W if (W % TILE == 0 and 0 < W <= 512) else 128          # a refused call still gets valid operands
    payload, ldl, inv, L = factored_block(ops, f"W={Wf}", Wf, Wf, 0, None)
    ld = nrows + 32
    P = Mat(rng.standard_normal((nrows, max(W, Wf))), ld)
    Lbb, invm = Mat(payload.reshape(Wf, ldl).T[:Wf], ldl), Mat(inv)
    res = Result().rc("solve_rows", ops.call("solve_rows", P, ld, nrows, W, Lbb, ldl, invm), want)
    res.add("Lbb", Lbb).add("inv", invm)
    if want != OK:
        return res.add("P", P)
    Li = memo(("tri_inv", ops.name, Wf), lambda: tri_inv_ld(L))
    ref = mm_ld(P.was(), Li)                                       # P L^-T
    scale = np.abs(P.was()) @ np.abs(Li).astype(np.float64).T
    # the tolerance comes from the device's blocked algorithm restated in float64 (numpy_solve_rows); NumpyOps itself
    # runs NumpyDistEngine's solve_rows (plain substitution), so the CPU run holds that callback to this tolerance too
    num = numpy_solve_rows(P.was(), L, inv, W)
    bound = subst_bound(res, "P", num, ref, scale)
    res.info["elements_differing_from_blocked_float64[P]"] = int(np.count_nonzero(bits(P.get()[:, :W].copy()) != bits(num[:, :W].copy())))
    return res.add("P", P, ref, bound, True)


for _W in (128, 256, 384, 512):
    for _n in (128, 640):
        case("solve_rows", f"solve_rows[W={_W},nrows={_n}]", ["gpak_dev_solve_rows", "gpak_dev_factor_panel_co", "gpak_dev_factor_panel"], W=_W,
             nrows=_n)(_solve_rows)
case("solve_rows", "solve_rows[W=256,nrows=20736]", ["gpak_dev_solve_rows"], W=256, nrows=20736)(_solve_rows)
for _W, _n in ((640, 128), (64, 128), (128, 192)):
    case("solve_rows", f"solve_rows[W={_W},nrows={_n}]->EINVAL", ["gpak_dev_solve_rows"], W=_W, nrows=_n, want=EINVAL)(_solve_rows)


# ---- triangular-solve pieces on one synthetic panel ---------------------------------------------------
TRSV_SHAPES = ((1408, 256, 512), (1408, 1280, 128), (1408, 1024, 384), (4992, 0, 512))


class Panel:
    """One block column (Np, J, W) as a full column (ld) and as a packed panel from its diagonal block (ldp), with the
    long-double quantities the cases share."""

    def __init__(self, ops, Np, J, W):
        rng = rng_for(f"panel[{Np},{J},{W}]")
        self.Np, self.J, self.W, self.rows = Np, J, W, Np - J - W
        below = rng.standard_normal((self.rows, W)) / np.sqrt(Np)
        self.payload, self.ld, self.inv, self.L = factored_block(ops, f"panel[{Np},{J},{W}]", W, Np, J, below)
        self.col = self.payload.reshape(W, self.ld).T[:Np]           # Np x W, sentinel above J
        self.below = self.col[J + W:]
        self.ldp = Np - J + 34
        self.Li = tri_inv_ld(self.L)
        self.aLi = np.abs(self.Li).astype(np.float64)

    def blk(self):
        return Mat(self.col, self.ld)

    def packed(self):
        return Mat(self.col[self.J:], self.ldp)


def panel_for(ops, shape):
    return memo(("panel", ops.name) + tuple(shape), lambda: Panel(ops, *shape))


def _trsv_fwd(ops, name, shape):
    p, rng = panel_for(ops, shape), rng_for(name)
    Np, J, W = shape
    blk, inv = p.blk(), Mat(p.inv)
    x, out = Mat(rng.standard_normal(Np)), Mat(rng.standard_normal(Np))
    res = Result().rc("trsv_fwd_block", ops.call("trsv_fwd_block", blk, p.ld, Np, J, W, inv, x, out))
    x0 = x.was()[:, 0]
    xn, on = x0.copy(), np.zeros(Np)                       # the float64 restatement, on the same factor
    numpy_ops().eng.trsv_fwd_block(numpy_ops()._t(p.payload.copy()), p.ld, Np, J, W, numpy_ops()._t(p.inv.copy()),
                                   numpy_ops()._t(xn), numpy_ops()._t(on))
    sol = mv_ld(p.Li, x0[J:J + W])
    tail = x0[J + W:].astype(LD) - mv_ld(p.below, sol)
    s_out = p.aLi @ np.abs(x0[J:J + W])
    s_tail = np.abs(x0[J + W:]) + np.abs(p.below) @ s_out
    ref = np.concatenate([sol, tail])
    bound = subst_bound(res, "out,x", np.concatenate([on[J:J + W], xn[J + W:]]), ref, np.concatenate([s_out, s_tail]))
    idx = np.arange(Np)[:, None]
    pad = lambda v, lo: np.concatenate([np.zeros(lo, dtype=v.dtype), v, np.zeros(Np - lo - len(v), dtype=v.dtype)])
    res.add("out", out, pad(ref[:W], J), pad(bound[:W], J), (idx >= J) & (idx < J + W))
    # x: every row from J + W on is updated; rows of the block itself hold intermediates; rows above J are not touched
    res.add("x", x, pad(ref[W:], J + W), pad(bound[W:], J + W), idx >= J + W, free=(idx >= J) & (idx < J + W))
    return res.add("blk", blk).add("inv", inv)


def _coldot(ops, name, shape):
    p, rng = panel_for(ops, shape), rng_for(name)
    Np, J, W = shape
    blk, x, s = p.blk(), Mat(rng.standard_normal(Np)), Mat(rng.standard_normal(W))
    res = Result().rc("coldot", ops.call("coldot", blk, p.ld, Np, J, W, x, s))
    xt = x.was()[J + W:, 0]
    ref = mv_ld(p.below.T, xt) if p.rows else np.zeros(W, dtype=LD)
    bound = (p.rows + 2) * U * (np.abs(p.below).T @ np.abs(xt)) if p.rows else np.zeros(W)
    return res.add("s", s, ref, bound, True).add("x", x).add("blk", blk)


def _trsv_bwd_block(ops, name, shape):
    p, rng = panel_for(ops, shape), rng_for(name)
    Np, J, W = shape
    blk, inv = p.blk(), Mat(p.inv)
    x, out = Mat(rng.standard_normal(Np)), Mat(rng.standard_normal(Np))
    res = Result().rc("trsv_bwd_block", ops.call("trsv_bwd_block", blk, p.ld, J, W, inv, x, out))
    x0 = x.was()[:, 0]
    xn, on = x0.copy(), np.zeros(Np)
    numpy_ops().eng.trsv_bwd_block(numpy_ops()._t(p.payload.copy()), p.ld, J, W, numpy_ops()._t(p.inv.copy()),
                                   numpy_ops()._t(xn), numpy_ops()._t(on))
    ref = mv_ld(p.Li.T, x0[J:J + W])
    bound = subst_bound(res, "out", on[J:J + W], ref, p.aLi.T @ np.abs(x0[J:J + W]))
    idx = np.arange(Np)[:, None]
    inside = (idx >= J) & (idx < J + W)
    pad = lambda v: np.concatenate([np.zeros(J, dtype=v.dtype), v, np.zeros(Np - J - W, dtype=v.dtype)])
    res.add("out", out, pad(ref), pad(bound), inside)
    return res.add("x", x, free=inside).add("blk", blk).add("inv", inv)      # x above J (and below the block): untouched


def _diag_inverse(ops, p):
    """rinv from gpak_dev_diag_inverse on the packed panel (a 512 x 512 buffer, leading dimension 512)"""
    rng = rng_for(f"rinv[{p.Np},{p.J},{p.W}]")
    panel, inv, rinv = p.packed(), Mat(p.inv), Mat(rng.standard_normal((512, 512)))
    rc = ops.call("diag_inverse", panel, p.ldp, p.J, p.J, p.W, inv, rinv)
    return rc, panel, inv, rinv


def _diag_inverse_case(ops, name, shape):
    p = panel_for(ops, shape)
    W = p.W
    rc, panel, inv, rinv = _diag_inverse(ops, p)
    res = Result().rc("diag_inverse", rc)
    ref = np.zeros((512, 512), dtype=LD)
    ref[:W, :W] = p.Li.T
    scale = np.full((512, 512), 1.0)
    scale[:W, :W] = (p.aLi @ np.abs(p.L) @ p.aLi).T          # the forward bound of an inversion: |X| |L| |X|
    # np.linalg.inv is also what NumpyDistEngine's diag_inverse runs: on the float64 restatement this case compares it
    # with itself (ratio 1/8 by construction) and proves the reference and the masks only; on the device it is a test
    num = np.linalg.inv(p.L).T
    bound = np.zeros((512, 512))
    bound[:W, :W] = subst_bound(res, "rinv", num, ref[:W, :W], scale[:W, :W])
    cmp, free = np.zeros((512, 512), dtype=bool), np.zeros((512, 512), dtype=bool)
    cmp[:W, :W] = True
    free[W:, :W] = True                                      # the header promises the W x W block; columns from W on are not the call's
    res.add("rinv", rinv, ref, bound, cmp, free=free).add("panel", panel).add("inv", inv)
    for Wbad in (640, 64):
        r2 = Mat(np.zeros((8, 8)))
        res.rc(f"diag_inverse[W={Wbad}]", ops.call("diag_inverse", panel, p.ldp, p.J, p.J, Wbad, inv, r2), EINVAL).add("r2", r2)
    return res


def _trsv_bwd_packed(ops, name, shape, with_rinv):
    p, rng = panel_for(ops, shape), rng_for(f"trsv_bwd_packed[{shape}]")     # both variants share inputs
    Np, J, W = shape
    panel, inv = p.packed(), Mat(p.inv)
    z, out, scratch = Mat(rng.standard_normal(Np)), Mat(rng.standard_normal(Np)), Mat(np.zeros(24 * 512))
    rinv = None
    res = Result()
    if with_rinv:
        rc, _pn, _iv, rinv = _diag_inverse(ops, p)
        res.rc("diag_inverse", rc)
        rinv = Mat(rinv.get())
    res.rc("trsv_bwd_packed", ops.call("trsv_bwd_packed", panel, p.ldp, J, Np, J, W, inv, z, scratch, out, rinv))
    z0, o0 = z.was()[:, 0], out.was()[:, 0]
    zn, on = z0.copy(), o0.copy()
    nrinv = np.zeros((512, 512))
    nrinv[:W, :W] = np.linalg.inv(p.L).T
    nrinv = Mat(nrinv) if with_rinv else None
    numpy_ops().call("trsv_bwd_packed", Mat(p.col[J:], p.ldp), p.ldp, J, Np, J, W, p.inv.copy(), zn, np.zeros(24 * 512), on, nrinv)
    s = mv_ld(p.below.T, o0[J + W:]) if p.rows else np.zeros(W, dtype=LD)
    ref = mv_ld(p.Li.T, z0[J:J + W].astype(LD) - s)
    sabs = np.abs(p.below).T @ np.abs(o0[J + W:]) if p.rows else np.zeros(W)
    bound = subst_bound(res, "out", on[J:J + W], ref, p.aLi.T @ (np.abs(z0[J:J + W]) + sabs))
    idx = np.arange(Np)[:, None]
    pad = lambda v: np.concatenate([np.zeros(J, dtype=v.dtype), v, np.zeros(Np - J - W, dtype=v.dtype)])
    res.add("out", out, pad(ref), pad(bound), (idx >= J) & (idx < J + W))
    res.add("z", z).add("panel", panel).add("inv", inv)               # z is read-only
    res.add("scratch", scratch, free=True)
    if rinv is not None:
        res.add("rinv", rinv)
    if not with_rinv:
        for Wbad in (640, 64):
            res.rc(f"trsv_bwd_packed[W={Wbad}]", ops.call("trsv_bwd_packed", panel, p.ldp, J, Np, J, Wbad, inv, z, scratch,
                                                          out, None), EINVAL)
    return res


def _logdiag(ops, name, shape, N):
    p = panel_for(ops, shape)
    Np, J, W = shape
    blk, out = p.blk(), Mat(np.array([123.0]))
    res = Result().rc("logdiag_block", ops.call("logdiag_block", blk, p.ld, J, W, N, out))
    nc = max(0, min(W, N - J))
    lg = np.log(np.diag(p.L)[:nc].astype(LD))
    ref, sabs = lg.sum(), float(np.abs(lg).sum())
    return res.add("out", out, [ref], [(nc + 2) * U * sabs + 4 * U * sabs], True).add("blk", blk)


def _pack(ops, name, shape):
    p = panel_for(ops, shape)
    row0, nrows, ncols = 128, 258, 3
    M = np.nan_to_num(p.col, nan=7.0)          # finite everywhere: a bound of zero then asks for the exact copy
    src, dst = Mat(M, p.ld), Mat(np.zeros(nrows * ncols))
    res = Result().rc("pack", ops.call("pack", src, p.ld, row0, nrows, ncols, dst))
    ref = M[row0:row0 + nrows, :ncols].T.ravel()
    res.add("dst", dst, ref, np.zeros(nrows * ncols), True).add("src", src)
    d2 = Mat(np.zeros(nrows * ncols))
    res.rc("pack[nrows odd]", ops.call("pack", src, p.ld, row0, nrows + 1, ncols, d2), EINVAL)
    res.rc("pack[row0 odd]", ops.call("pack", src, p.ld, row0 + 1, nrows, ncols, d2), EINVAL)
    res.rc("pack[ld odd]", ops.call("pack", src, p.ld + 1, row0, nrows, ncols, d2), EINVAL)
    res.rc("pack[ncols=0]", ops.call("pack", src, p.ld, row0, nrows, 0, d2), OK)
    return res.add("d2", d2)


for _s in TRSV_SHAPES:
    _t = f"[Np={_s[0]},J={_s[1]},W={_s[2]}]"
    case("trsv", "trsv_fwd_block" + _t, ["gpak_dev_trsv_fwd_block", "gpak_dev_factor_panel_co"], shape=_s)(_trsv_fwd)
    case("trsv", "coldot" + _t, ["gpak_dev_coldot"], shape=_s)(_coldot)
    case("trsv", "trsv_bwd_block" + _t, ["gpak_dev_trsv_bwd_block"], shape=_s)(_trsv_bwd_block)
    case("trsv", "diag_inverse" + _t, ["gpak_dev_diag_inverse"], shape=_s)(_diag_inverse_case)
    case("trsv", "trsv_bwd_packed" + _t + "[rinv=None]", ["gpak_dev_trsv_bwd_packed"], shape=_s, with_rinv=False)(_trsv_bwd_packed)
    case("trsv", "trsv_bwd_packed" + _t + "[rinv]", ["gpak_dev_trsv_bwd_packed", "gpak_dev_diag_inverse"], shape=_s,
         with_rinv=True)(_trsv_bwd_packed)
    for _N in (_s[0] - 5, _s[1] + 70, _s[1]):
        case("trsv", "logdiag_block" + _t + f"[N={_N}]", ["gpak_dev_logdiag_block"], shape=_s, N=_N)(_logdiag)
    case("trsv", "pack" + _t, ["gpak_dev_pack"], shape=_s)(_pack)


# ---- the two linear-algebra operations of the distributed gradient ----------------------------------------
# (gpak_dev_grad_pairs_rows / _consts / _finish stay under the distributed-gradient tests: no bound of this file's kind
# exists for the pair sums.)  The interface fixes every leading dimension here (a packed panel has Np - J, a slab and
# binv have rows_a), so these buffers have guard bands but no skew rows.
def grad_tiles(Np, P, a):
    T = Np // TILE
    return (T - a + P - 1) // P if T > a else 0


def grad_rows(Np, P, a):
    """global rows of the 128-row blocks g = t P + a, in slab order"""
    return (np.arange(grad_tiles(Np, P, a))[:, None] * P * TILE + a * TILE + np.arange(TILE)[None, :]).ravel()


class Factor:
    """A whole lower-triangular factor of order Np as block columns of nb: each the Panel of the trsv cases (diagonal
    block factored by the engine under test, dense rows below), with L^-1 in long double."""

    def __init__(self, ops, Np, nb):
        self.Np, self.nb = Np, nb
        self.cols = [Panel(ops, Np, J, min(nb, Np - J)) for J in range(0, Np, nb)]
        self.L = np.zeros((Np, Np))
        for p in self.cols:
            self.L[p.J:p.J + p.W, p.J:p.J + p.W] = p.L
            self.L[p.J + p.W:, p.J:p.J + p.W] = p.below
        self.Li = tri_inv_ld(self.L)

    def panels(self):
        return [Mat(p.col[p.J:]) for p in self.cols]        # packed: leading dimension Np - J

    def invs(self):
        return [Mat(p.inv) for p in self.cols]


def factor_for(ops, Np, nb):
    return memo(("factor_full", ops.name, Np, nb), lambda: Factor(ops, Np, nb))


def numpy_g_rows(f, P, a):
    """csrc/grad.hip's blocked forward substitution on identity rows in float64: per block column, 128-column steps
    W_j := W_j inv(D_j)^T, W[:, j+1..] -= W_j L[j+1.., j]^T inside it, then one update of everything to the right; a row
    block takes part from the step of its own diagonal block on."""
    Np, nb, Ta, rows = f.Np, f.nb, grad_tiles(f.Np, P, a), grad_rows(f.Np, P, a)
    S = np.zeros((len(rows), Np))
    S[np.arange(len(rows)), rows] = 1.0
    upto = lambda g: min(Ta, (g - a) // P + 1) * TILE if g >= a else 0
    for p in f.cols:
        J, W = p.J, p.W
        iv = p.inv.reshape(W // TILE, 2, TILE, TILE)
        for j0 in range(J, J + W, TILE):
            m, c = upto(j0 // TILE), slice(j0, j0 + TILE)
            if m:
                S[:m, c] = S[:m, c] @ iv[(j0 - J) // TILE, 0]
                S[:m, j0 + TILE:J + W] -= S[:m, c] @ f.L[j0 + TILE:J + W, c].T
        m = upto((J + W) // TILE - 1)
        if m and J + W < Np:
            S[:m, J + W:] -= S[:m, J:J + W] @ f.L[J + W:, J:J + W].T
    return S


def _grad_g_rows(ops, name, Np, nb, P, a):
    f = factor_for(ops, Np, nb)
    rows = grad_rows(Np, P, a)
    panels, invs = f.panels(), f.invs()
    slab = Mat(rng_for(name).standard_normal((max(len(rows), TILE), Np)))
    res = Result().rc("grad_g_rows", ops.call("grad_g_rows", Np, nb, P, a, panels, invs, slab))
    for k, (pn, iv) in enumerate(zip(panels, invs)):
        res.add(f"panel{k}", pn).add(f"inv{k}", iv)
    if not len(rows):
        return res.add("slab", slab)                          # no tiles: nothing is written
    # rows of L^-T = columns of L^-1; |L^-1| |e_i| = |L^-1|: exact zeros left of the diagonal, so the bound is 0 there
    ref = f.Li[:, rows].T
    bound = subst_bound(res, "slab", numpy_g_rows(f, P, a), ref, np.abs(ref).astype(np.float64))
    return res.add("slab", slab, ref, bound, True)


for _a in (0, 1, 2):
    case("grad", f"grad_g_rows[Np=640,nb=256,P=3,a={_a}]", ["gpak_dev_grad_g_rows", "gpak_dev_factor_panel_co"], Np=640, nb=256,
         P=3, a=_a)(_grad_g_rows)
case("grad", "grad_g_rows[Np=640,nb=512,P=1,a=0]", ["gpak_dev_grad_g_rows"], Np=640, nb=512, P=1, a=0)(_grad_g_rows)
case("grad", "grad_g_rows[Np=128,nb=128,P=2,a=1]->no-op", ["gpak_dev_grad_g_rows"], Np=128, nb=128, P=2, a=1)(_grad_g_rows)


def grad_slab(ops, Np, nb, P, a):
    """rank a's rows of L^-T from the engine under test (checked by the cases above)"""
    def make():
        f = factor_for(ops, Np, nb)
        slab = Mat(np.zeros((grad_tiles(Np, P, a) * TILE, Np)))
        assert ops.call("grad_g_rows", Np, nb, P, a, f.panels(), f.invs(), slab) == OK and slab.guards_ok()
        return slab.get().copy()
    return memo(("grad_slab", ops.name, Np, nb, P, a), make)


def _grad_binv_rows(ops, name, a, b, want=OK, Np=640, nb=256, P=3):
    Tmax, Ta = grad_tiles(Np, P, 0), grad_tiles(Np, P, a)
    Sa = Mat(grad_slab(ops, Np, nb, P, a))
    Sb = Sa if b == a else Mat(grad_slab(ops, Np, nb, P, b % P))      # the same pointer when b == a (gpak_dev.h)
    binv = Mat(rng_for(name).standard_normal((Ta * TILE, P * Tmax * TILE)))
    res = Result().rc("grad_binv_rows", ops.call("grad_binv_rows", Np, P, a, b, Sa, Sb, binv), want)
    res.add("slab_a", Sa)
    if Sb is not Sa:
        res.add("slab_b", Sb)
    if want != OK:
        return res.add("binv", binv)
    # tile (t, u) of column group b Tmax + u <- rows t of slab_a times rows u of slab_b, where u P + b <= t P + a
    Tb = grad_tiles(Np, P, b)
    need = np.zeros((Ta, P * Tmax), dtype=bool)
    mine = np.zeros((Ta, P * Tmax), dtype=bool)
    for u in range(Tb):
        mine[:, b * Tmax + u] = True
        need[:, b * Tmax + u] = u * P + b <= np.arange(Ta) * P + a
    ref, bound = np.zeros(binv.get().shape, dtype=LD), np.zeros(binv.get().shape)
    cols = slice(b * Tmax * TILE, (b * Tmax + Tb) * TILE)
    ref[:, cols] = mm_ld(Sa.was(), Sb.was())
    bound[:, cols] = (Np + 2) * U * (np.abs(Sa.was()) @ np.abs(Sb.was()).T)
    # the tiles of rank b that are NOT needed come back bit-identical from the device; the float64 restatement
    # (np_dist_engine.py) writes the whole product there, so they are free on that engine and on that engine only
    free = tile_rows(mine & ~need) if ops.name == "numpy" else None
    return res.add("binv", binv, ref, bound, tile_rows(need), free=free)


for _a, _b in ((0, 0), (0, 2), (2, 0), (1, 1)):
    case("grad", f"grad_binv_rows[Np=640,P=3,a={_a},b={_b}]", ["gpak_dev_grad_binv_rows", "gpak_dev_grad_g_rows"], a=_a,
         b=_b)(_grad_binv_rows)
case("grad", "grad_binv_rows[Np=640,P=3,a=1,b=3]->EINVAL", ["gpak_dev_grad_binv_rows"], a=1, b=3, want=EINVAL)(_grad_binv_rows)


# ---- matrix-vector products and reductions ---------------------------------------------------------------
def _gemv_n_add(ops, name, nrows, W, want=OK):
    rng = rng_for(name)
    ld = nrows + 33
    A, x, y = Mat(rng.standard_normal((nrows, W)), ld), Mat(rng.standard_normal(W)), Mat(rng.standard_normal(nrows))
    res = Result().rc("gemv_n_add", ops.call("gemv_n_add", A, ld, nrows, W, x, y), want)
    if want != OK:
        return res.add("y", y).add("A", A).add("x", x)
    y0, xv = y.was()[:, 0], x.was()[:, 0]
    ref = y0.astype(LD) + mv_ld(A.was(), xv)
    bound = (W + 2) * U * (np.abs(A.was()) @ np.abs(xv) + np.abs(y0))
    return res.add("y", y, ref, bound, True).add("A", A).add("x", x)


def _gemv_t(ops, name, nrows, W):
    rng = rng_for(name)
    ld = max(nrows, 1) + 33
    A = Mat(rng.standard_normal((max(nrows, 1), W)), ld)
    x, y = Mat(rng.standard_normal(max(nrows, 1))), Mat(rng.standard_normal(W))
    res = Result().rc("gemv_t", ops.call("gemv_t", A, ld, nrows, W, x, y))
    Av, xv = A.was()[:nrows], x.was()[:nrows, 0]
    ref = mv_ld(Av.T, xv) if nrows else np.zeros(W, dtype=LD)              # nrows = 0: y = 0
    bound = (nrows + 2) * U * (np.abs(Av).T @ np.abs(xv)) if nrows else np.zeros(W)
    return res.add("y", y, ref, bound, True).add("A", A).add("x", x)


def _vec_ops(ops, name, n):
    """vec_axpy, vec_scale, vec_sum, nlz_terms on n entries (buffers one longer: the entry after the end is not theirs)"""
    rng = rng_for(name)
    res = Result()
    idx = np.arange(n + 1)[:, None] < n
    pad = lambda v: np.concatenate([np.asarray(v), np.zeros(1, dtype=np.asarray(v).dtype)])
    a = 0.37
    x, y = Mat(rng.standard_normal(n + 1)), Mat(rng.standard_normal(n + 1))
    res.rc("vec_axpy", ops.call("vec_axpy", n, a, x, y))
    x0, y0 = x.was()[:n, 0], y.was()[:n, 0]
    res.add("axpy.y", y, pad(y0.astype(LD) + LD(a) * x0), pad(3 * U * (np.abs(a * x0) + np.abs(y0))), idx).add("axpy.x", x)
    s = -1.7
    vin, vout = Mat(rng.standard_normal(n + 1)), Mat(rng.standard_normal(n + 1))
    res.rc("vec_scale", ops.call("vec_scale", n, vin, s, vout))
    v0 = vin.was()[:n, 0]
    res.add("scale.out", vout, pad(v0.astype(LD) * LD(s)), pad(3 * U * np.abs(v0 * s)), idx).add("scale.in", vin)
    tot = Mat(np.array([5.0, 6.0]))
    res.rc("vec_sum", ops.call("vec_sum", n, vin, tot))
    res.add("sum.out", tot, [v0.astype(LD).sum(), 0], [(n + 2) * U * np.abs(v0).sum(), 0], [[True], [False]])
    # nlz_terms: out[0] = sum alpha_i (f_i / 2), out[1] = sum -(y_i - f_i)^2 / (2 sn2) - log(2 pi sn2) / 2; both held to
    # (n + 2) u sum|terms|, the terms of out[1] being (y_i - f_i)^2 / (2 sn2) and log(2 pi sn2) / 2 for every i
    sn2 = 0.016
    yv, f, al = (Mat(rng.standard_normal(n + 1)) for _ in range(3))
    out = Mat(np.array([5.0, 6.0, 7.0]))
    res.rc("nlz_terms", ops.call("nlz_terms", n, yv, f, al, sn2, out))
    y1, f1, a1 = (m.was()[:n, 0].astype(LD) for m in (yv, f, al))
    q = a1 * (f1 / 2)
    c = np.log(2 * LD(np.pi) * LD(sn2)) / 2
    lp = (y1 - f1) ** 2 / (2 * LD(sn2))
    ref = [q.sum(), (-lp - c).sum(), 0]
    bound = [(n + 2) * U * float(np.abs(q).sum()), (n + 2) * U * float((lp + abs(c)).sum()), 0]
    res.add("nlz.out[0]", out, ref, bound, [[True], [False], [False]], free=[[False], [True], [False]])      # per entry, so that
    res.add("nlz.out[1]", out, ref, bound, [[False], [True], [False]], free=[[True], [False], [False]])      # each ratio is printed
    res.add("nlz.y", yv).add("nlz.f", f).add("nlz.alpha", al)
    return res


for _n in (1, 255, 256, 700):
    for _W in (1, 127, 512):
        case("reduce", f"gemv_n_add[nrows={_n},W={_W}]", ["gpak_dev_gemv_n_add"], nrows=_n, W=_W)(_gemv_n_add)
        case("reduce", f"gemv_t[nrows={_n},W={_W}]", ["gpak_dev_gemv_t"], nrows=_n, W=_W)(_gemv_t)
    case("reduce", f"vec_axpy,vec_scale,vec_sum,nlz_terms[n={_n}]",
         ["gpak_dev_vec_axpy", "gpak_dev_vec_scale", "gpak_dev_vec_sum", "gpak_dev_nlz_terms"], n=_n)(_vec_ops)
case("reduce", "gemv_n_add[nrows=256,W=513]->EINVAL", ["gpak_dev_gemv_n_add"], nrows=256, W=513, want=EINVAL)(_gemv_n_add)
case("reduce", "gemv_t[nrows=0,W=127]", ["gpak_dev_gemv_t"], nrows=0, W=127)(_gemv_t)


# ---- fill and Gram mat-vec against the CPU oracle -------------------------------------------------------
FILL_N, FILL_NP = 300, 384
FILL_TOL = {1: 1e-13, 0: 2e-7}        # test_gram_matches_oracle: relative to max |K|, DIST_DIRECT = 1, DIST_EXPANSION = 0
HYB_TERMS = [(0, None), (2, [0.5, 0.9, 0.5])]       # ExpAns (the default parameters) + RBF
HYB_WHITE = 0.10


class Points:
    """300 drill-hole points transformed by the engine under test, and the oracle's B = I + K / sn2"""

    def __init__(self, ops, kind, mode):
        from gp_ss_ak_amd import synth
        from oracle import oracle as orc
        self.E = np.array(synth.DEFAULT_EXPANS, dtype=np.float64)
        self.bias, self.sn2 = synth.DEFAULT_BIAS, synth.DEFAULT_SN2
        n, cap = FILL_N, FILL_NP
        X, _y = synth.drillholes4(n) if kind == "d4" else synth.drillholes(n)
        X = np.asarray(X, dtype=np.float64)
        xs = np.zeros((4, cap))
        xs[:X.shape[1], :n] = X.T
        mu = np.zeros(4)
        mu[:X.shape[1]] = X.sum(axis=0) / n                      # pooled mean of X u X (Kernel.cpp:1391-1392)
        self.u = np.zeros(15 * cap)
        self.mode = mode | (D4 if kind == "d4" else 0) | (HYB if kind == "hyb" else 0)
        if kind == "hyb":
            terms = [(k, list(self.E) if p is None else p) for k, p in HYB_TERMS]
            kern = [len(terms)] + [k for k, _ in terms] + [0] * (3 - len(terms)) + [HYB_WHITE]
            for _k, p in terms:
                kern += list(p)
            self.kern = kern + [0.0] * (32 - len(kern))
            rc = ops.call("transform_k", xs.ravel(), cap, n, cap, self.kern, self.mode, mu, self.u)
            K = orc.gram_hyb(X, X, terms, self.bias, HYB_WHITE, mode)
        else:
            self.kern = list(self.E)
            rc = ops.call("transform", xs.ravel(), cap, n, cap, self.kern, mu, self.u)
            K = orc.gram(X, X, self.E, self.bias, mode)
        assert rc == OK
        # checked INDIRECTLY, through fill and kmatvec; on the spot: a second call gives the same bits (the cases memoise it)
        u2 = np.zeros(15 * cap)
        if kind == "hyb":
            ops.call("transform_k", xs.ravel(), cap, n, cap, self.kern, self.mode, mu, u2)
        else:
            ops.call("transform", xs.ravel(), cap, n, cap, self.kern, mu, u2)
        assert np.array_equal(bits(self.u), bits(u2)), "two transforms of the same points differ"
        self.K = K
        self.B = np.eye(cap)
        self.B[:n, :n] += K / self.sn2
        self.tol = FILL_TOL[mode] * np.abs(K).max() / self.sn2
        self.transform_entry = "gpak_dev_transform_k" if kind == "hyb" else "gpak_dev_transform"


def points_for(ops, kind, mode):
    return memo(("points", ops.name, kind, mode), lambda: Points(ops, kind, mode))


def fill_expect(pt, rows, cols, written):
    """reference, bound and mask for B[rows, cols]: the oracle's value within the fill tolerance where both points
    exist, EXACTLY 0 (1 on the diagonal) in padded rows and columns"""
    ref = pt.B[rows][:, cols]
    valid = (np.arange(FILL_NP)[rows] < FILL_N)[:, None] & (np.arange(FILL_NP)[cols] < FILL_N)[None, :]
    return ref, np.where(valid, pt.tol, 0.0), written


def _fill_b(ops, name, J, W, kind, mode):
    pt = points_for(ops, kind, mode)
    Np, ld = FILL_NP, FILL_NP + 32
    blk = Mat(rng_for(name).standard_normal((Np, W)), ld)
    res = Result().rc("fill_b", ops.call("fill_b", pt.u, Np, FILL_N, Np, J, W, pt.kern, pt.bias, pt.sn2, pt.mode, blk, ld))
    lower = tile_rows(np.arange(Np // TILE)[:, None] >= (J // TILE + np.arange(W // TILE))[None, :])
    ref, bound, cmp = fill_expect(pt, slice(0, Np), slice(J, J + W), lower)   # tiles strictly above the diagonal: untouched
    return res.add("blk", blk, ref, bound, cmp)


def _fill_rect(ops, name, row0, nrows, col0, ncols, kind, mode, want=OK):
    pt = points_for(ops, kind, mode)
    ld = nrows + 32
    dst = Mat(rng_for(name).standard_normal((nrows, ncols)), ld)
    res = Result().rc("fill_rect", ops.call("fill_rect", pt.u, FILL_NP, FILL_N, row0, nrows, col0, ncols, pt.kern, pt.bias,
                                            pt.sn2, pt.mode, dst, ld), want)
    if want != OK:
        return res.add("dst", dst)
    written = np.ones((nrows, ncols), dtype=bool)               # row0 != col0: filled whole
    if row0 == col0:                                            # a diagonal piece: its lower 128-tiles
        written = (np.arange(nrows)[:, None] // TILE) >= (np.arange(ncols)[None, :] // TILE)
    ref, bound, cmp = fill_expect(pt, slice(row0, row0 + nrows), slice(col0, col0 + ncols), written)
    return res.add("dst", dst, ref, bound, cmp)


def _kmatvec(ops, name, i0, i1, mode):
    pt = points_for(ops, "3d", mode)
    rng = rng_for(name)
    cap, n = FILL_NP, FILL_N
    w, out, scratch = Mat(rng.standard_normal(cap)), Mat(rng.standard_normal(cap)), Mat(np.zeros(64 * cap))
    res = Result().rc("kmatvec", ops.call("kmatvec", pt.u, cap, n, i0, i1, w, pt.kern, pt.bias, pt.mode, scratch, out))
    wv = w.was()[i0:i1, 0]
    Ks = pt.K[i0:i1]
    ref = np.zeros(cap, dtype=LD)
    ref[:n] = mv_ld(Ks.T, wv)
    bound = np.zeros(cap)
    bound[:n] = (i1 - i0 + 2) * U * (np.abs(Ks).T @ np.abs(wv)) + FILL_TOL[mode] * np.abs(pt.K).max() * np.abs(wv).sum()
    return res.add("out", out, ref, bound, np.arange(cap)[:, None] < n).add("w", w).add("scratch", scratch, free=True)


for _mode, _mn in ((1, "direct"), (0, "expansion")):
    for _J, _W in ((0, 384), (128, 256), (256, 128)):
        case("fill", f"fill_b[J={_J},W={_W},{_mn}]", ["gpak_dev_fill_b", "gpak_dev_transform"], J=_J, W=_W, kind="3d",
             mode=_mode)(_fill_b)
    for _r in ((0, 128, 0, 128), (128, 256, 0, 128), (256, 128, 128, 256), (0, 128, 128, 128), (0, 128, 64, 64),
               (256, 128, 256, 128)):
        case("fill", f"fill_rect[{_r[0]},{_r[1]},{_r[2]},{_r[3]},{_mn}]", ["gpak_dev_fill_rect"], row0=_r[0], nrows=_r[1],
             col0=_r[2], ncols=_r[3], kind="3d", mode=_mode)(_fill_rect)
    for _i0, _i1 in ((0, 300), (0, 128), (130, 300), (299, 300)):
        case("fill", f"kmatvec[{_i0},{_i1},{_mn}]", ["gpak_dev_kmatvec"], i0=_i0, i1=_i1, mode=_mode)(_kmatvec)
for _kind, _ent in (("d4", "gpak_dev_transform"), ("hyb", "gpak_dev_transform_k")):
    case("fill", f"fill_b[J=0,W=384,direct,{_kind}]", ["gpak_dev_fill_b", _ent], J=0, W=384, kind=_kind, mode=1)(_fill_b)
    case("fill", f"fill_rect[128,256,0,128,direct,{_kind}]", ["gpak_dev_fill_rect", _ent], row0=128, nrows=256, col0=0,
         ncols=128, kind=_kind, mode=1)(_fill_rect)
case("fill", "fill_rect[nrows=64]->EINVAL", ["gpak_dev_fill_rect"], row0=0, nrows=64, col0=0, ncols=128, kind="3d", mode=1,
     want=EINVAL)(_fill_rect)
case("fill", "fill_rect[ncols=32]->EINVAL", ["gpak_dev_fill_rect"], row0=0, nrows=128, col0=0, ncols=32, kind="3d", mode=1,
     want=EINVAL)(_fill_rect)


# ------------------------------------------------------------------------------------------------
# running a case
# ------------------------------------------------------------------------------------------------
def summarise(name, first, second):
    """One JSON-able record of a case that ran twice."""
    ratios = {c.label: c.ratio() for c in first.checks}
    viol = {c.label: c.violations() for c in first.checks if c.violations()}
    guards = all(c.mat.guards_ok() for r in (first, second) for c in r.checks)
    rcs = [list(t) for t in first.rcs]
    same = len(first.checks) == len(second.checks) and all(
        np.array_equal(bits(a.mat.full), bits(b.mat.full)) for a, b in zip(first.checks, second.checks))
    worst = max(ratios.values()) if ratios else 0.0
    ok = (worst <= 1.0 and not viol and guards and same and all(g == w for _l, g, w in first.rcs)
          and first.rcs == second.rcs)
    return {"case": name, "ok": bool(ok), "ratio": worst if np.isfinite(worst) else "inf", "violations": viol,
            "guards_ok": guards, "rc": rcs, "deterministic": bool(same),
            "info": {k: float(v) for k, v in first.info.items()}, "ratios": {k: (v if np.isfinite(v) else "inf") for k, v in ratios.items()}}


def run_group(ops, group):
    for g, name, _ents, fn in CASES:
        if g == group:
            yield summarise(name, fn(ops), fn(ops))
