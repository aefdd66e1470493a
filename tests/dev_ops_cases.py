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

The pair passes of the gradients (group `pairs`: gpak_dev_grad_pair_sums, either pass of csrc/grad.hip on caller-owned
buffers).  Inputs: 515 drill-hole points (odd: the last row tile holds 3 valid rows and the double2 of lane 1 straddles
the edge, the column blocks 576..639 are empty, block column 512 has 3 valid columns) transformed by the engine under
test, Np = cap = 640, alpha standard_normal, B^-1 standard_normal on i >= j, i, j < n -- not symmetric, not a kernel
matrix, not an inverse -- and the sentinel NaN in every other element of every buffer (i < j inside diagonal tiles, tiles
above the diagonal, rows and columns >= n, rows >= n of u, x_soa, alpha): a read that is used shows as a NaN sum.  In
DIRECT mode points 77 and 300 coincide (sd == 0 off the diagonal, in different tiles: dk = 0 there by definition).  The
reference is each of the 16 sums elementwise over the pairs in np.longdouble, written from the comments above RefPass /
ExactPass, on the u the engine produced, with M_p and m2 from gpak_dev_grad_consts (held to the oracle's independent
S % S_p by the case `grad_consts via the oracle`).  Bound per sum, u = 2^-53:
    (pairs + 2) u sum|t~|  +  sum (c0 + c1 s) u |t~|
  * the first part holds for any order of accumulation (the fma of the accumulation rounds once per pair);
  * t~ is the term with every cancelling sub-expression replaced by the sum of magnitudes: |q|/sn2 + |alpha_i alpha_j| for
    qw, |a_i| + |a_j| + 4 |x|^T |M_p| |x| for Di2; products of differences of raw columns are products already;
  * c0 + c1 s is the relative error of evaluating one term, from the operation count, with 1 ulp <= 2u and the documented
    2 ulp (4u) of gpak_sqrt_nonneg / gpak_exp_nonpos (gpak_internal.h).  qw: 1/sn2, two products, one difference: 3u of
    its magnitude.  d2 by differences: 4 differences, 4 squares, 3 additions of non-negative terms: 6u; a sum of up to
    three of them: 8u.  sd = sqrt(d2): 3u (4u of a summed d2) + 4u.  exp(-sd): an absolute error of 7u sd (8u sd) in the
    argument becomes a relative one of the result, + 4u: this is c1 s with s = sd.  The RBF argument iw d2 / 2 carries
    8u + 2u, so s = iw d2 / 2 there and c1 >= 10.  dk = e (-0.5 / sd): 7u sd + 4u + 8u + 1u.  The worst slots: as written
    0..5, var2 qw dk Di2: 3 + 13 + 2 products + Di2 (two three-term dots 6u, two additions 2u, each a_i 4u of |a_i| when its
    three terms have one sign) = 34u + 7u sd; as written 9+2t of an Exp child, qw dk(d2s) d2s: 3 + 14 + 2 + 8 = 27u + 8u sd;
    10+2t of an Exp child, qw kd kd, has the exponential twice: 13u + 16u sd; exact 8..13, 2 qw e (-0.5 / sd) D_a D_b:
    3 + 4 + 8 + 2 + 2 + 2 = 21u + 7u sd.  Hence c0 = 40 and c1 = 16 for every slot (PAIR_C0, PAIR_C1);
  * a_i = sum_k x_ik^2 m2_pk has mixed signs, so its rounding is no multiple of |a_i|: 4u sum_k x_ik^2 |m2_pk| per a is
    charged on its own, through the term's other factors;
  * expansion mode (as-written pass): d2 = ps + qs - 2 dot carries delta = 8u (ps + qs + 2 sum|p_c q_c|) against the true
    |u_i - u_j|^2 that the reference uses; off the diagonal its first-order effect |dt/dd2| delta is added (|dk| delta for
    exp(-sd), e (1 + sd) / (4 sd^3) delta for dk), and the case asserts d2 >= 1e6 delta for every such pair (the smallest
    ratio of these inputs is 7e8); ON the diagonal the true d2 is 0 and the computed one is noise <= delta, where no first
    order exists: 1 - exp(-sqrt(z)) <= sqrt(z), so sqrt(delta) of the term's other factors is added for the slots that
    use exp(-sd) there (6 and 7; dk is 0 on the diagonal by definition, and x4_i - x4_i is 0).
One dropped, doubled, misplaced or mis-weighted pair is 10^7 or more bounds (test_the_checks_bite).  A slot a pass does
not use must be +0.0; u, x_soa, alpha, binv and every guard band come back bit-identical; `part` is scratch.  The sums of
the ranks of a P, added in long double, are held to the P = 0 reference within the sum of the ranks' bounds.
gpak_dev_grad_pairs_rows must give the bits of gpak_dev_grad_pair_sums on the same buffers, and out[16] within
(n + 2) u sum((y - f)^2 / sn2 + 1).  gpak_dev_grad_finish[_d]: the formulas of gpak_grad_assemble in long double, 4u of
each entry's magnitude (of |red_7| / sn2 + |red_16| for the sn2 entry).  The oracle case: g[10] assembled from the
long-double sums against orc.grad_ref_q on the symmetric Q of the same lower triangle: twice the case's own bound through
the linear assembly (the oracle is a float64 sum of the same terms in another order), the rounding of M_p itself on
either side (derived in the case), and, for the sn2 entry, the oracle's own f = K alpha.

The panel factorisation alone (group `panel`: gpak_dev_factor_panel_co).  Operands G G^T / W + 2 I on the diagonal block
(a junk upper triangle: only the lower one is read) and standard_normal rows below; W = 128 .. 1024, J = 0 / 384, 0 / 128 /
640 rows below, either build.  Reference in long double: chol_ld (128-column steps, products through mm_ld), P L^-T for
the rows below, the inverse of each 128-block.  Bound, the substitutions' house rule: 8 x the worst error of the float64
restatement of the device's blocked algorithm (np_engine.blocked_factor_panel) against long double on the same input,
relative to s_L = |L| tril(|L^-1| |L||L^T| |L^-T|) for L, |P||L^-T| (I + s_L^T |L^-T|) for the rows below and
|X| (|L_kk| + s_L,kk) |X| for a block inverse X; the residual |A - L L^T| of what came back, in long double, within
(W + 2) u |L||L^T| times 8 x the restatement's own residual ratio.  The second image of `inv` is the transpose of the
first in bits; the diagonal 16-tiles come back with exact zeros above the diagonal; 128-tiles above the diagonal, rows
above J, skew rows and guard bands keep their bits (the 16-tiles above the diagonal inside a diagonal 128-block are
scratch).  `info`: matrices built to fail at a chosen column (tests/failcol_ref.py: D[k] = -1, an exact zero pivot, a
NaN; two failing blocks; pre-set values on either side), the fixture's own rules asserted on the CPU first.

The fp32 prediction kernels alone (group `f32`: include/gpak_dev_f32.h, thin wrappers over the launchers of
csrc/gemm_f32.hip and the ladder of csrc/predict.hip that a GPAK_F32 context runs).  Buffers of floats carry float guard
bands and a float sentinel NaN (`Mat(..., dtype=F32)`); leading dimensions are skewed by multiples of 4 floats (16-byte
loads); a build of the product is selected as the product selects it, through GPAK_F32_ACC / GPAK_F32_RSD / GPAK_F32_TILE
and gpak_reload_tuning (`ops.f32_build`), and the environment is put back afterwards.  u32 = 2^-24, u64 = 2^-53;
references are long double on the float operands taken exactly.
  * gemm_nt_f32: six builds x seven shapes (F32_BUILDS, F32_SHAPES: one tile, an even and an odd number of row tiles,
    one to five chunks of K, the 8 x 8 super-tile crossed in both directions, three super-rows on one super-column) x
    (alpha, beta) = (1, 0) on a C of NaN, (-1, 1), (0.75, -0.5), and in place (A == C) where nt = 1 and K = 128; A carries
    row scales 10^-3 .. 10^3.  Bounds per element, for any order of summation.  Plain builds: a float32 sum of K products
    is at most K roundings deep, alpha and the fused beta c add two: (K + 2) u32 (|alpha| sum|a||b| + |beta||c|).  Wide
    builds: a chunk of 128 summed in float32, 128 u32 sum|a||b| (130 with the second order and, at K = 128 where the plain
    kernel runs, the rounding of alpha * sum); conversions to float64 are exact; K / 128 additions, alpha * total and the
    fused beta c in float64, (K / 128 + 3) u64 of the magnitudes; ONE rounding to float, u32 |exact result|.
    The four wide builds differ in the prefetch ring and the occupancy only, so they must give the same bits (asserted).
  * That the wide build is wide: (2, 1, 4096), operands uniform on [0.5, 1.5).  Tolerance, the house rule: 8 x the worst
    error, relative to sum|terms|, of the float32 restatement of the chunked scheme (f32_product, products rounded and
    added one k at a time) against long double, measured in the case; the case first asserts that the restatement of
    plain accumulation over all K is at least 2 tolerances out (measured: chunked 2.5 u32, plain 63 u32, margin 3.1).
  * fill_f32: nP = 131 of 256 rows, nQ = 70 of 128 columns, drill-hole points, P[130] == Q[33], rows from n on of every
    transformed array the sentinel; six compositions, a White child that must change no bit; rows >= nP and columns >= nQ
    +0.0f.  Bound per element: sum_m var2_m e^(-s_m) (c0 + c1 s_m) u32 + (terms + 2) u32 |k|, s_m the exponential's
    argument.  The operation count of gpak_fill_f32 per term: the distance in float64 (4 differences, 4 squares, 3
    additions: 6 u64, nothing beside u32) and ONE conversion to float; ExpSqrt: sqrtf, a negation, __expf = v_exp_f32 of
    the argument times log2(e) (one product, one rounded constant); RBF: the conversion of iw, an exact halving, one
    product with d, then the same __expf; the conversion of var2 and one product (or fused multiply-add) into k; the
    conversion of the bias and one addition per term.  The MI355X guides state no accuracy for v_exp_f32, v_sqrt_f32 or
    the float conversions (they say only that hipcc keeps f32 subnormals), so each of those is taken as 2 ulp = 4 u32;
    a float product or sum is one rounding, u32, by the format.  A relative error in the argument is s times that in
    the result.  ExpSqrt: the conversion of d is 4 u32 of d = 2 u32 of s, sqrtf 4, the product with log2(e) and the
    constant 2: c1 = 8.  RBF: conversions of d and iw 4 + 4, the product 1, log2(e) 2: c1 = 11.  On the result: v_exp_f32
    4, the conversion of var2 4, the product 1: c0 = 9.  Hence FILL32_C0 = 10, FILL32_C1 = 12 for every term.  The sum:
    `terms` additions of positive numbers, u32 |k| each, and the bias's conversion, for which the form leaves 2 u32 |k|.
  * lower_to_f32 / vec_to_f32: the bits of np.float32(.) (round to nearest even: halfway cases, results in and below
    the float denormals, signed zeros, 3e38), +0.0f above the diagonal, the factor's upper triangle the sentinel.
  * rowsumsq_f32: every partial to (columns of the split + 2) u64 sum v^2, their sum on the host to (cols + 2) u64 sum v^2;
    rows = 1 .. 300, splits with a shorter last one, of one column, of odd length (cols = 639 is this module's addition).
  * fwd_subst_f32: the 640-row factor of the group `grad`, imaged by the two conversions; levels 128 / 512, 128 / 256, 128,
    128 / 256 / 1024 (the last child of a block clipped at one or two levels), under the default and the plain build.
    Tolerance as for solve_rows: 8 x the error of f32_ladder (the same recursion on f32_product, one k at a time) against
    W Lf^-T in long double, relative to |W||Lf^-T|.
The eleven wrong engines of test_the_checks_bite each fail a named case of this group.

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
SENTINEL32 = np.uint32(0x7FC5BEEF)           # the same for float buffers (group `f32`)
F32 = np.float32
U32 = 2.0 ** -24
OK, EINVAL = 0, 2
INT_MAX = 0x7FFFFFFF
D4, HYB = 0x10, 0x20
GROUPS = ("gemm", "solve_rows", "trsv", "reduce", "fill", "grad", "pairs", "panel", "f32")


def long_double_ok():
    return np.finfo(np.longdouble).eps < 1e-18


def sentinel(n, dtype=np.float64):
    if np.dtype(dtype) == np.float32:
        return np.full(int(n), SENTINEL32, dtype=np.uint32).view(np.float32)
    return np.full(int(n), SENTINEL, dtype=np.uint64).view(np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Mat:
    """rows x cols column-major doubles (or floats: dtype) with leading dimension ld inside a guarded buffer; the skew
    rows hold the sentinel.  `before` is the payload as it went in."""

    def __init__(self, M, ld=None, dtype=np.float64):
        M = np.asarray(M, dtype=dtype)
        if M.ndim == 1:
            M = M[:, None]
        self.rows, self.cols = M.shape
        self.ld = int(ld) if ld is not None else self.rows
        self.sent = SENTINEL32 if M.dtype == np.float32 else SENTINEL
        body = sentinel(self.cols * self.ld, dtype).reshape(self.cols, self.ld)
        body[:, :self.rows] = M.T
        self.full = np.concatenate([sentinel(GUARD, dtype), body.ravel(), sentinel(GUARD, dtype)])
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
        return bool((f[:GUARD] == self.sent).all() and (f[GUARD + self.n:] == self.sent).all())

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
# arguments of gpak_dev_<name> after the stream: p device pointer, i int, l long, d double, h host double array (a list,
# read only), H host double array (an array or a Mat, passed as it is), P host array of device pointers (a list here)
SIG = {
    "transform": "piiihhp", "transform_k": "piiihihp", "fill_b": "piiiiihddipl", "fill_rect": "piiiiiihddipl",
    "factor_panel": "pliiipp", "factor_panel_co": "pliiippi", "update_block": "pliipliii", "update_cyclic": "pliipliiiiiii",
    "update_rect": "plplipliii", "solve_rows": "pliiplp", "trsv_fwd_block": "pliiippp", "coldot": "pliiipp",
    "trsv_bwd_block": "pliippp", "trsv_bwd_packed": "pliiiippppp", "diag_inverse": "pliiipp", "logdiag_block": "pliiip",
    "kmatvec": "piiiiphdipp", "nlz_terms": "ipppdp", "pack": "pliiip", "gemv_n_add": "pliipp", "gemv_t": "pliipp",
    "vec_axpy": "idpp", "vec_scale": "ipdp", "vec_sum": "ipp", "grad_g_rows": "iiiiPPp", "grad_binv_rows": "iiiippp",
    "grad_pair_sums": "ipipiiippliihddipp", "grad_pairs_rows": "pipiiippppiihddipp",
    "grad_finish": "hddiHH", "grad_finish_d": "hddiiHH", "grad_consts": "hHH",
    # include/gpak_dev_f32.h (group `f32`): f float, I host int array (a list)
    "gemm_nt_f32": "iiifplplfpl", "fill_f32": "piipiiiihdipl", "lower_to_f32": "plipl", "vec_to_f32": "plp",
    "rowsumsq_f32": "pliiipi", "fwd_subst_f32": "pliiplpIi",
}
F32_OPS = ("gemm_nt_f32", "fill_f32", "lower_to_f32", "vec_to_f32", "rowsumsq_f32", "fwd_subst_f32")
F32_ENV = ("GPAK_F32_ACC", "GPAK_F32_RSD", "GPAK_F32_TILE")


class Off:
    """a pointer `elems` elements into a Mat's payload (a misaligned operand for a refusal)"""

    def __init__(self, mat, elems):
        self.mat, self.elems = mat, int(elems)
HOST_ONLY = ("grad_finish", "grad_finish_d", "grad_consts")       # no stream argument; H: a host array, read or written


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
    if name == "grad_pairs_rows":
        return EINVAL if a[10] < 1 or a[11] < 0 or a[11] >= a[10] else None
    if name == "grad_pair_sums":
        passno, ld, P, ra, kern, mode = a[0], a[9], a[10], a[11], a[12], a[15]
        if passno not in (0, 1) or P < 0 or (P > 0 and (ra < 0 or ra >= P)) or (P == 0 and ld & 1):
            return EINVAL
        if mode & HYB:
            nt, kinds = int(kern[0]), [int(k) for k in kern[1:4]]
            if nt < 1 or nt > 3 or any(k not in (0, 1, 2) for k in kinds[:nt]) or kern[4] != 0.0 or kinds[:nt].count(0) > 1:
                return EINVAL
        return None
    if name == "update_cyclic":
        nb, lb0, n_local, last_width = a[7], a[10], a[11], a[12]
        return OK if (n_local - 1) * (nb // TILE) + last_width // TILE - lb0 * (nb // TILE) <= 0 else None
    # include/gpak_dev_f32.h; a Mat's payload is 16-byte aligned, an Off by a multiple of 4 floats keeps that
    odd = lambda x, per: isinstance(x, Off) and x.elems % per != 0
    same = lambda x, y: (x.mat if isinstance(x, Off) else x) is (y.mat if isinstance(y, Off) else y)
    if name == "gemm_nt_f32":
        mt, nt, K, _al, A, lda, B, ldb, _be, Cm, ldc = a
        if mt <= 0 or nt <= 0:
            return OK
        if K < TILE or K % TILE or lda < mt * TILE or ldb < nt * TILE or ldc < mt * TILE or (lda | ldb | ldc) & 3:
            return EINVAL
        if odd(A, 4) or odd(B, 4) or odd(Cm, 4) or (same(A, Cm) and (nt != 1 or K != TILE)):
            return EINVAL
        return None
    if name == "fill_f32":
        _uP, capP, nP, _uQ, capQ, nQ, rows_p, cols_p, kern, _bias, mode, _C, ld = a
        if rows_p <= 0 or rows_p % TILE or cols_p <= 0 or cols_p % 64 or capP < rows_p or capP & 1:
            return EINVAL
        if nP < 0 or nP > rows_p or nQ < 0 or nQ > cols_p or nQ > capQ or ld < rows_p or ld & 1:
            return EINVAL
        if mode & HYB:
            nt, kinds = int(kern[0]), [int(k) for k in kern[1:4]]
            if nt < 1 or nt > 3 or any(k not in (0, 1, 2) for k in kinds[:nt]):
                return EINVAL
        return None
    if name == "lower_to_f32":
        _L, ld, Np, _out, ldo = a
        return EINVAL if Np <= 0 or ld < Np or ldo < Np else None
    if name == "vec_to_f32":
        return None if a[1] > 0 else (OK if a[1] == 0 else EINVAL)
    if name == "rowsumsq_f32":
        _V, ldv, rows, cols, splits, _part, part_ld = a
        return EINVAL if rows <= 0 or cols <= 0 or splits < 1 or splits > cols or ldv < rows or part_ld < rows else None
    if name == "fwd_subst_f32":
        Wt, ldw, mrows, Np, Lf, ldLf, invf, levels, nlevels = a
        if mrows <= 0 or mrows % TILE or Np <= 0 or Np % TILE or ldw < mrows or ldLf < Np or (ldw | ldLf) & 3:
            return EINVAL
        if odd(Wt, 4) or odd(Lf, 4) or odd(invf, 4) or nlevels < 0 or nlevels > 8:
            return EINVAL
        lv = list(levels)[:nlevels]
        if any((v != TILE) if k == 0 else (v <= lv[k - 1] or v % lv[k - 1]) for k, v in enumerate(lv)):
            return EINVAL
        return None
    return None


def _buf(x):
    return x.full if isinstance(x, Mat) else x


def pay(x):
    """the payload of a Mat (from `elems` on for an Off), or the array itself"""
    if isinstance(x, Off):
        return x.mat.data[x.elems:]
    return x.data if isinstance(x, Mat) else x


class NumpyOps:
    """The float64 restatement: the callbacks of NumpyDistEngine (they have the C signatures of gpak_dev_*), and
    NumpyEngine for the two operations the C++ schedules do not use."""
    name = "numpy"

    def __init__(self, mut=()):
        """mut: deliberate faults of the pair pass (np_dist_engine.pair_sums) or of the float32 restatements (F32Restated),
        for test_the_checks_bite"""
        import torch
        from np_dist_engine import NumpyDistEngine
        self.torch = torch
        self.nde = NumpyDistEngine(poison_upper=False)
        self.eng = self.nde.np
        self.mut = tuple(mut)
        self.f32 = F32Restated(mut=self.mut)

    def f32_build(self, env=None):
        """the build of the fp32 product the calls that follow run under: the GPAK_F32_* variables of the library"""
        self.f32.wide = (env or {}).get("GPAK_F32_ACC") != "plain"

    @staticmethod
    def _ptr(x):
        if x is None:
            return None
        if isinstance(x, Mat):
            return x.full.ctypes.data + x.full.itemsize * GUARD
        return x.ctypes.data

    def _t(self, x):
        return self.torch.from_numpy(x.data if isinstance(x, Mat) else x)

    def call(self, name, *a):
        assert len(a) == len(SIG[name]), name
        rc = precheck(name, a)
        if rc is not None:
            return rc
        if name in F32_OPS:
            return getattr(self.f32, name)(*a)
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
        if name == "grad_pair_sums":
            import np_dist_engine as nd
            pay = lambda x: x.data if isinstance(x, Mat) else x
            passno, u, cap, xs, xst, n, Np, alpha, binv, ld, P, ra, kern, bias, sn2, mode, _part, out = a
            nd.pair_sums(passno, pay(u), cap, pay(xs), xst, n, Np, pay(alpha), pay(binv), ld, P, ra, kern, bias, sn2, mode, pay(out),
                         mut=self.mut)
            if "store" in self.mut:
                pay(binv)[0] = 1.0
            return OK
        if name in ("grad_finish", "grad_finish_d"):
            E, bias, sn2, n = a[:4]
            red, g = (x.data if isinstance(x, Mat) else x for x in a[-2:])
            d = a[4] if name == "grad_finish_d" else 3
            g[:6] = red[:6]
            g[6] = 2.0 * red[6] * E[6]
            g[7] = -4.0 * red[15] / n if d == 4 else 0.0
            g[8] = red[8]
            g[9] = -1.0 * (0.5 * red[7]) * (2.0 / sn2) - red[16]
            return OK
        if name == "grad_consts":              # host code of the library under either engine: its check is the oracle
            return host_call(name, a)
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


def host_call(name, a):
    """a host-only entry point of libgpak_hip.so (no stream, no device)"""
    from gp_ss_ak_amd import _lib
    fn = getattr(_lib.load(), "gpak_dev_" + name)
    fn.restype = C.c_int
    fn.argtypes = [HipOps._ct[k] for k in SIG[name]]
    conv, keep = [], []
    for kind, v in zip(SIG[name], a):
        if kind == "h":
            keep.append((C.c_double * len(v))(*[float(t) for t in v]))
            conv.append(keep[-1])
        elif kind == "H":
            arr = v.data if isinstance(v, Mat) else v
            assert arr.dtype == np.float64 and arr.flags.c_contiguous
            conv.append(arr.ctypes.data_as(C.POINTER(C.c_double)))
        else:
            conv.append(v)
    return int(fn(*conv))


class HipOps:
    """libgpak_hip.so on the device: HipEngine for the library, the device and the stream; every call uploads its
    arrays, runs, synchronises and downloads them again (guard bands included)."""
    name = "hip"
    _ct = {"p": C.c_void_p, "i": C.c_int, "l": C.c_long, "d": C.c_double, "h": C.POINTER(C.c_double), "P": C.POINTER(C.c_void_p),
           "H": C.POINTER(C.c_double), "f": C.c_float, "I": C.POINTER(C.c_int)}

    def __init__(self):
        from py_schedule import HipEngine
        self.eng = HipEngine(0)
        self.lib = self.eng.lib

    def f32_build(self, env=None):
        """Select the build of the fp32 product as the product does: the GPAK_F32_* variables and gpak_reload_tuning.
        No argument: the environment as the process found it."""
        if not hasattr(self, "_env0"):
            self._env0 = {k: os.environ.get(k) for k in F32_ENV}
        for k in F32_ENV:
            v = (env or {}).get(k) if env is not None else self._env0[k]
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        self.lib.gpak_reload_tuning()

    def call(self, name, *a):
        assert len(a) == len(SIG[name]), name
        if name in HOST_ONLY:
            return host_call(name, a)
        fn = getattr(self.lib, "gpak_dev_" + name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [self._ct[k] for k in SIG[name]]
        dev, conv, keep = {}, [], []

        def ptr(v):
            if isinstance(v, Off):
                return ptr(v.mat) + v.elems * v.mat.full.itemsize
            if id(v) not in dev:
                dev[id(v)] = (v, self.eng.from_numpy(_buf(v)))
            return dev[id(v)][1].data_ptr() + (_buf(v).itemsize * GUARD if isinstance(v, Mat) else 0)

        for kind, v in zip(SIG[name], a):
            if kind == "p":
                conv.append(None if v is None else ptr(v))
            elif kind == "P":
                keep.append((C.c_void_p * len(v))(*[ptr(x) for x in v]))
                conv.append(keep[-1])
            elif kind == "h":
                keep.append((C.c_double * len(v))(*[float(t) for t in v]))
                conv.append(keep[-1])
            elif kind == "I":
                keep.append((C.c_int * max(len(v), 1))(*[int(t) for t in v]))
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
    """every gpak_dev_* function include/gpak_dev.h and include/gpak_dev_f32.h declare, and the vector pieces of
    include/gpak_dist.h"""
    names = set()
    for h in ("gpak_dev.h", "gpak_dev_f32.h", "gpak_dist.h"):
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
    Returns (payload, ld, inv, L).  The factorisation itself is held to long double by the group `panel`; what is checked
    on the spot here is that
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
# (the pair pass and the host ends of the chain are the group `pairs`, further down.)  The interface fixes every leading
# dimension here (a packed panel has Np - J, a slab and
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


# ---- the pair passes of the gradients alone ---------------------------------------------------------------
# gpak_dev_grad_pair_sums (either pass of csrc/grad.hip on caller-owned buffers), gpak_dev_grad_pairs_rows, and the host
# ends of the chain (gpak_dev_grad_consts, gpak_dev_grad_finish / _finish_d).  The bound is derived in the module docstring.
PAIR_C0, PAIR_C1 = 40.0, 16.0
PAIR_N, PAIR_NP, PAIR_LD = 515, 640, 672
PAIR_TWINS = (77, 300)                 # two coincident points, off the diagonal and in different tiles (DIRECT mode only)
EXP_P, RBF_P = [0.7, 0.8], [0.5, 0.9, 0.5]
PAIR_COMPS = {                         # name -> (terms, input columns); None = the default ExpAns parameters
    "expans+bias": ([(0, None)], 3), "expans d4": ([(0, None)], 4), "expans+rbf": (HYB_TERMS, 3),
    "exp+rbf": ([(1, EXP_P), (2, RBF_P)], 3), "expans+exp+rbf": ([(0, None), (1, EXP_P), (2, RBF_P)], 3),
}
PAIR_SLOTS = 16


def serialise(terms, white):
    kern = [len(terms)] + [k for k, _ in terms] + [0] * (3 - len(terms)) + [white]
    for _k, p in terms:
        kern += list(p)
    return kern + [0.0] * (32 - len(kern))


class PairData:
    """The inputs of a pair pass: n drill-hole points (two of them coincident in DIRECT mode) transformed by the engine
    under test, alpha and the elements i >= j of B^-1 standard_normal, the sentinel everywhere else; and, per pass, the
    long-double sums, row by row."""

    def __init__(self, ops, comp, mode, n, Np):
        from gp_ss_ak_amd import synth
        terms, cols = PAIR_COMPS[comp]
        self.E = np.array(synth.DEFAULT_EXPANS, dtype=np.float64)
        self.terms = [(k, list(self.E) if p is None else list(p)) for k, p in terms]
        self.bias, self.sn2, self.n, self.Np, self.cap, self.d = synth.DEFAULT_BIAS, synth.DEFAULT_SN2, n, Np, Np, cols
        self.hyb = not (len(terms) == 1 and terms[0][0] == 0)
        self.mode = mode | (D4 if cols == 4 else 0) | (HYB if self.hyb else 0)
        self.kern = serialise(self.terms, 0.0) if self.hyb else list(self.E)
        rng = rng_for(f"pairs[{comp},{mode},{n}]")
        X, _y = synth.drillholes4(n) if cols == 4 else synth.drillholes(n)
        X = np.array(X, dtype=np.float64)
        if mode == 1 and n > PAIR_TWINS[1]:
            X[PAIR_TWINS[1]] = X[PAIR_TWINS[0]]
        self.X = X
        cap = self.cap
        xs = np.zeros((4, cap))
        xs[:cols, :n] = X.T
        mu = np.zeros(4)
        mu[:cols] = X.sum(axis=0) / n
        call = (lambda u: ops.call("transform_k", xs.ravel(), cap, n, cap, self.kern, self.mode, mu, u)) if self.hyb else \
               (lambda u: ops.call("transform", xs.ravel(), cap, n, cap, self.kern, mu, u))
        u, u2 = np.zeros(15 * cap), np.zeros(15 * cap)
        assert call(u) == OK and call(u2) == OK
        assert np.array_equal(bits(u), bits(u2)), "two transforms of the same points differ"
        nt = len(self.terms)
        poison = lambda M: np.where((np.arange(cap) < n)[:, None], M, sentinel(1)[0])         # rows from n on: the sentinel
        self.u = poison(u.reshape(15, cap).T[:, :5 * nt])                                     # cap x 5 nterms
        self.xs = poison(xs.T)
        self.alpha = poison(np.concatenate([rng.standard_normal(n), np.zeros(cap - n)])[:, None])
        self.B = np.tril(rng.standard_normal((n, n)))
        self.y, self.f = rng.standard_normal(n), rng.standard_normal(n)
        self.un = u.reshape(15, cap)[:5 * nt, :n].reshape(nt, 5, n).copy()
        self.te = [k for k, _ in self.terms].index(0) if 0 in [k for k, _ in self.terms] else -1
        if self.te >= 0:
            from np_dist_engine import grad_consts
            self.Mp, self.m2 = grad_consts(self.terms[self.te][1])
        self._sums = {}

    def binv(self, P, a):
        """B^-1 as rank a of P holds it (P == 0: Np x Np, leading dimension PAIR_LD): the sentinel wherever the pass has
        no business reading"""
        n, Np = self.n, self.Np
        low = np.tril(np.ones((n, n), dtype=bool))
        vals = np.where(low, self.B, sentinel(1)[0])
        if P == 0:
            M = sentinel(Np * Np).reshape(Np, Np)
            M[:n, :n] = vals
            return Mat(M, PAIR_LD if Np + 32 <= PAIR_LD else Np + 32)
        rows, Tmax = grad_rows(Np, P, a), grad_tiles(Np, P, 0)
        M = sentinel(max(len(rows), TILE) * P * Tmax * TILE).reshape(max(len(rows), TILE), P * Tmax * TILE)
        cols = np.arange(n)
        cperm = ((cols // TILE % P) * Tmax + cols // TILE // P) * TILE + cols % TILE
        loc = np.arange(len(rows))[rows < n]
        if len(loc):
            M[np.ix_(loc, cperm)] = vals[rows[rows < n]]
        return Mat(M)

    def sums(self, passno):
        """per row i and slot: the long-double sum over j <= i, sum |t~|, and the evaluation part of the bound"""
        if passno not in self._sums:
            self._sums[passno] = pair_reference(self, passno)
        return self._sums[passno]

    def expect(self, passno, P, a):
        """reference and bound of the 16 sums over the rows of rank a of P"""
        ref, tb, ev = self.sums(passno)
        rows = grad_rows(self.Np, P, a) if P else np.arange(self.n)
        rows = rows[rows < self.n]
        pairs = float((rows + 1).sum())
        return ref[:, rows].sum(axis=1), (pairs + 2) * U * tb[:, rows].sum(axis=1) + ev[:, rows].sum(axis=1)


def pair_reference(d, passno):
    """The 16 sums of a pass elementwise over the pairs in np.longdouble, from the formulas in the comments above RefPass
    and ExactPass (csrc/grad.hip), with the true distance |u_i - u_j|^2 of the transformed points in either dist_mode."""
    n, sn2, bias = d.n, LD(d.sn2), LD(d.bias)
    ii, jj = np.arange(n)[:, None], np.arange(n)[None, :]
    low, diag = ii >= jj, ii == jj
    w = np.where(diag, 1.0, 2.0) * low
    q = d.B.astype(LD)
    al = d.alpha[:n, 0].astype(LD)
    aa = al[:, None] * al[None, :]
    qw, qwb = (q / sn2 - aa) * low, ((np.abs(q) / sn2 + np.abs(aa)) * low).astype(np.float64)
    X4 = np.zeros((n, 4), dtype=LD)
    X4[:, :d.d] = d.X
    expansion = passno == 0 and (d.mode & 0xF) == 0
    assert not expansion or len(d.terms) == 1, "the expansion-mode part of the bound is written for one ExpAns term"
    d2, dd = [], []
    for m in range(len(d.terms)):
        c = d.un[m][[0, 1, 2, 4]].astype(LD)
        d2.append(((c[:, :, None] - c[:, None, :]) ** 2).sum(axis=0))
        if expansion:         # delta d2 = 8u (ps + qs + 2 sum |p_c q_c|): the rounding of |u|^2 and of the expansion itself
            cf, ps = np.abs(d.un[m][[0, 1, 2, 4]]), d.un[m][3]
            dd.append(8 * U * (ps[:, None] + ps[None, :] + 2 * np.einsum("ci,cj->ij", cf, cf)))
            off = low & ~diag
            d.cond = float((d2[m][off].astype(np.float64) / dd[m][off]).min())
            assert d.cond >= 1e6, f"an off-diagonal pair has d2 = {d.cond:.3g} x its own cancellation noise"
    T, TB, EV = {}, {}, {}        # slot -> term, |t~|, evaluation bound (all n x n)

    def put(k, t, tbar, amp, extra=None):
        T[k], TB[k] = t, tbar
        EV[k] = U * (PAIR_C0 + PAIR_C1 * amp) * tbar + (0.0 if extra is None else extra)

    def expsqrt(D2):
        sd = np.sqrt(D2)
        ek = np.exp(-sd)
        with np.errstate(divide="ignore", invalid="ignore"):
            dk = np.where((sd == 0) | diag, LD(0), ek * (LD(-0.5) / sd))
        return sd, ek, dk

    f = lambda a: np.asarray(a, dtype=np.float64)
    var2 = [LD(np.float64(p[2]) * np.float64(p[2])) if k == 2 else LD(np.float64(p[6 if k == 0 else 1]) ** 2) for k, p in d.terms]
    if passno == 0:
        prof, amps = [], []
        for m, (k, p) in enumerate(d.terms):
            if k == 2:
                arg = LD(0.5) * LD(p[1]) * d2[m]
                prof.append(np.exp(-arg)); amps.append(f(arg))
            else:
                sd, ek, _dk = expsqrt(d2[m])
                prof.append(ek); amps.append(f(sd))
        kfull = bias + sum(v * e for v, e in zip(var2, prof))
        kbar = f(w * np.abs(q)) * (abs(d.bias) * PAIR_C0 + sum(f(v * e) * (PAIR_C0 + PAIR_C1 * s) for v, e, s in zip(var2, prof, amps)))
        T[7], TB[7] = w * q * kfull, f(w * np.abs(q) * (abs(bias) + sum(v * e for v, e in zip(var2, prof))))
        EV[7] = U * kbar
        put(8, qw * diag, qwb * diag, 0.0)
        if d.te >= 0:
            te = d.te
            sd, ek, dk = expsqrt(d2[te])
            sdf, ekf, dkf = f(sd), f(ek), np.abs(f(dk))
            off = low & ~diag
            x = X4[:, :3]
            xa = np.abs(f(x))
            dx4 = X4[:, 3][:, None] - X4[:, 3][None, :]
            if expansion:     # first order in delta d2 off the diagonal; on it d2 is noise <= delta d2 and 1 - exp(-sqrt(z)) <= sqrt(z)
                de = np.where(diag, np.sqrt(dd[te]), dkf * dd[te]) * low
                with np.errstate(divide="ignore", invalid="ignore"):
                    ddk = np.where(off, ekf * (1.0 + sdf) / (4.0 * sdf ** 3) * dd[te], 0.0)
                EV[7] = EV[7] + f(w * np.abs(q)) * float(var2[te]) * de
            # what an error of e in every entry of M_p (m2 = 2 x its column sums: 6 e) does to sums 0..5, per unit of e
            x2, x1 = (xa * xa).sum(axis=1), xa.sum(axis=1)
            d.mp_sens = float((f(w) * float(var2[te]) * qwb * dkf * (6 * (x2[:, None] + x2[None, :]) + 4 * x1[:, None] * x1[None, :])).sum())
            for p in range(6):
                Mp, m2 = d.Mp[p].astype(LD), d.m2[p].astype(LD)
                ai = (x * x) @ m2
                di2 = ai[:, None] + ai[None, :] - 4 * (x @ Mp @ x.T)
                di2b = np.abs(f(ai))[:, None] + np.abs(f(ai))[None, :] + 4.0 * (xa @ np.abs(d.Mp[p]) @ xa.T)
                # a_i is itself a three-term sum with mixed signs: its rounding, 4u sum_k x_ik^2 |m2_pk|, is no multiple of
                # |a_i| and is charged on its own
                ab = (xa * xa) @ np.abs(d.m2[p])
                rb = f(w) * float(var2[te]) * qwb
                put(p, w * var2[te] * qw * dk * di2, rb * dkf * di2b, sdf,
                    rb * dkf * 4 * U * (ab[:, None] + ab[None, :]) + (rb * di2b * ddk if expansion else 0.0))
            put(6, w * qw * ek, f(w) * qwb * ekf, sdf, f(w) * qwb * de if expansion else None)
            put(15, w * ek * dx4 * dx4, f(w * ek * dx4 * dx4), sdf, f(w * dx4 * dx4) * de * (~diag) if expansion else None)
        d2s = sum(d2)
        for m, (k, p) in enumerate(d.terms):
            if k == 1:
                sd, kd, dk = expsqrt(d2s)
                put(9 + 2 * m, w * qw * dk * d2s, f(w) * qwb * np.abs(f(dk)) * f(d2s), f(sd))
                put(10 + 2 * m, w * qw * kd * kd, f(w) * qwb * f(kd * kd), f(sd))
            elif k == 2:
                arg = LD(0.5) * LD(p[1]) * d2s
                kd = np.exp(-arg)
                put(9 + 2 * m, w * qw * kd * d2s, f(w) * qwb * f(kd * d2s), f(arg))
                put(10 + 2 * m, w * qw * kd, f(w) * qwb * f(kd), f(arg))
    else:
        put(0, w * qw, f(w) * qwb, 0.0)
        put(1, qw * diag, qwb * diag, 0.0)
        for m, (k, p) in enumerate(d.terms):
            if k == 2:
                arg = LD(0.5) * LD(p[1]) * d2[m]
                e = np.exp(-arg)
                put(2 + m, w * qw * e, f(w) * qwb * f(e), f(arg))
                put(5 + m, w * qw * e * d2[m], f(w) * qwb * f(e * d2[m]), f(arg))
                continue
            sd, ek, dk = expsqrt(d2[m])
            put(2 + m, w * qw * ek, f(w) * qwb * f(ek), f(sd))
            if m == d.te:
                D = [X4[:, c][:, None] - X4[:, c][None, :] for c in range(4)]
                for s, (ca, cb) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                    put(8 + s, w * qw * dk * D[ca] * D[cb], f(w) * qwb * np.abs(f(dk * D[ca] * D[cb])), f(sd))
                put(14, w * qw * dk * D[3] * D[3], f(w) * qwb * np.abs(f(dk * D[3] * D[3])), f(sd))
            else:
                put(5 + m, w * qw * dk * d2[m], f(w) * qwb * np.abs(f(dk)) * f(d2[m]), f(sd))
    ref, tb, ev = np.zeros((PAIR_SLOTS, n), dtype=LD), np.zeros((PAIR_SLOTS, n)), np.zeros((PAIR_SLOTS, n))
    for k in T:
        ref[k], tb[k], ev[k] = T[k].sum(axis=1), np.asarray(TB[k]).sum(axis=1), np.asarray(EV[k]).sum(axis=1)
    return ref, tb, ev


def pair_data(ops, comp, mode, n=PAIR_N, Np=PAIR_NP):
    return memo(("pairs", ops.name, comp, mode, n, Np), lambda: PairData(ops, comp, mode, n, Np))


def pair_buffers(d, P, a, name):
    Ta = grad_tiles(d.Np, P, a) if P else d.Np // TILE
    part = Mat(rng_for(name + "part").standard_normal(max(Ta, 1) * (d.Np // 64) * PAIR_SLOTS))
    return Mat(d.u), Mat(d.xs), Mat(d.alpha), d.binv(P, a), part


def add_sums(res, out, ref, bound, nout=PAIR_SLOTS):
    """one check per slot, so that each slot's ratio is printed; a slot the pass does not use (reference and bound 0) must
    be +0.0 exactly"""
    got = out.get()[:, 0]
    unused = [k for k in range(PAIR_SLOTS) if ref[k] == 0 and bound[k] == 0]
    res.rc("unused slots that are not +0.0", int(np.count_nonzero(bits(got[unused].copy()))))
    idx = np.arange(nout)[:, None]
    for k in range(nout):
        res.add(f"out[{k}]", out, ref, bound, idx == k, free=idx != k)


def _pair_sums(ops, name, passno, P, a, comp, mode, n=PAIR_N, Np=PAIR_NP):
    d = pair_data(ops, comp, mode, n, Np)
    u, xs, alpha, binv, part = pair_buffers(d, P, a, name)
    out = Mat(rng_for(name + "out").standard_normal(PAIR_SLOTS))
    res = Result().rc("grad_pair_sums", ops.call("grad_pair_sums", passno, u, d.cap, xs, d.cap, n, Np, alpha, binv, binv.ld, P, a,
                                                 d.kern, d.bias, d.sn2, d.mode, part, out))
    ref, bound = d.expect(passno, P, a)
    add_sums(res, out, ref, bound)
    if hasattr(d, "cond") and (d.mode & 0xF) == 0:
        res.info["smallest d2 / its cancellation noise"] = d.cond
    owns = P == 0 or grad_tiles(Np, P, a) > 0
    res.add("part", part, free=owns)                         # a rank without tiles leaves it alone
    return res.add("u", u).add("x_soa", xs).add("alpha", alpha).add("binv", binv)


def _pair_rank_sum(ops, name, passno, P, comp, mode):
    """the ranks' sums added in long double against the P = 0 reference, within the sum of the ranks' bounds"""
    d = pair_data(ops, comp, mode)
    res, tot, btot = Result(), np.zeros(PAIR_SLOTS, dtype=LD), np.zeros(PAIR_SLOTS)
    for a in range(P):
        u, xs, alpha, binv, part = pair_buffers(d, P, a, f"{name}{a}")
        out = Mat(np.zeros(PAIR_SLOTS))
        res.rc(f"grad_pair_sums[a={a}]", ops.call("grad_pair_sums", passno, u, d.cap, xs, d.cap, d.n, d.Np, alpha, binv, binv.ld,
                                                  P, a, d.kern, d.bias, d.sn2, d.mode, part, out))
        tot += out.get()[:, 0].astype(LD)
        btot += d.expect(passno, P, a)[1]
        res.add(f"binv{a}", binv)
    ref = d.expect(passno, 0, 0)[0]
    err = np.abs(tot - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / btot)
    r[~np.isfinite(err)] = np.inf
    res.info["ranks' sum: worst error / bound"] = float(r.max())
    return res.rc("slots of the ranks' sum outside the bound", int(np.count_nonzero(~(r <= 1.0))))


def _pair_refused(ops, name, what):
    d = pair_data(ops, "expans+rbf" if what in ("two expans", "white") else "expans+bias", 1)
    passno, P, a, kern, mode = 0, 0, 0, d.kern, d.mode
    if what == "pass":
        passno = 2
    if what == "a":
        P, a = 3, 3
    if what == "two expans":
        kern = serialise([(0, list(d.E)), (0, list(d.E))], 0.0)
    if what == "white":
        kern = serialise(d.terms, HYB_WHITE)
    u, xs, alpha, binv, part = pair_buffers(d, P, min(a, max(P - 1, 0)), name)
    out = Mat(rng_for(name).standard_normal(PAIR_SLOTS))
    ld = binv.ld + 1 if what == "ld" else binv.ld
    res = Result().rc("grad_pair_sums", ops.call("grad_pair_sums", passno, u, d.cap, xs, d.cap, d.n, d.Np, alpha, binv, ld, P, a,
                                                 kern, d.bias, d.sn2, mode, part, out), EINVAL)
    return res.add("out", out).add("part", part).add("u", u).add("x_soa", xs).add("alpha", alpha).add("binv", binv)


def _pairs_rows(ops, name, comp):
    """gpak_dev_grad_pairs_rows: the same bits as gpak_dev_grad_pair_sums on the same buffers, and the lp_dhyp sum"""
    P, a = 3, 1
    d = pair_data(ops, comp, 1)
    n, cap = d.n, d.cap
    u, xs, alpha, binv, part = pair_buffers(d, P, a, name)
    poison = lambda v: Mat(np.concatenate([v, sentinel(cap - n)]))
    y, f = poison(d.y), poison(d.f)
    out, o16 = Mat(rng_for(name + "out").standard_normal(PAIR_SLOTS + 1)), Mat(np.zeros(PAIR_SLOTS))
    res = Result().rc("grad_pairs_rows", ops.call("grad_pairs_rows", u, cap, xs, cap, n, d.Np, y, f, alpha, binv, P, a, d.kern,
                                                  d.bias, d.sn2, d.mode, part, out))
    res.rc("grad_pair_sums", ops.call("grad_pair_sums", 0, u, cap, xs, cap, n, d.Np, alpha, binv, 0, P, a, d.kern, d.bias, d.sn2,
                                      d.mode, Mat(part.was()), o16))
    res.rc("sums that differ from gpak_dev_grad_pair_sums", int(np.count_nonzero(bits(out.get()[:16, 0].copy()) != bits(o16.get()[:, 0].copy()))))
    ref, bound = d.expect(0, P, a)
    dl = (d.y.astype(LD) - d.f.astype(LD)) ** 2 / LD(d.sn2)
    ref = np.concatenate([ref, [(dl - 1).sum()]])
    bound = np.concatenate([bound, [(n + 2) * U * float((dl + 1).sum())]])
    add_sums(res, out, ref, bound, PAIR_SLOTS + 1)
    o2 = Mat(np.zeros(PAIR_SLOTS + 1))
    res.rc("grad_pairs_rows[a=P]", ops.call("grad_pairs_rows", u, cap, xs, cap, n, d.Np, y, f, alpha, binv, P, P, d.kern, d.bias,
                                            d.sn2, d.mode, part, o2), EINVAL).add("o2", o2)
    return res.add("part", part, free=True).add("u", u).add("x_soa", xs).add("alpha", alpha).add("binv", binv).add("y", y).add("f", f)


def finish_ld(E, bias, sn2, n, d, red):
    """gpak_grad_assemble for ExpAns + Bias in long double: the ten entries and the magnitudes their rounding scales with"""
    r = np.asarray(red, dtype=LD)
    g, mag = np.zeros(10, dtype=LD), np.zeros(10)
    g[:6] = r[:6]
    g[6] = 2 * r[6] * LD(E[6])
    g[7] = -4 * r[15] / LD(n) if d == 4 else 0
    g[8] = r[8]
    g[9] = -(LD(0.5) * r[7]) * (2 / LD(sn2)) - r[16]
    mag[:9] = np.abs(g[:9]).astype(np.float64)
    mag[9] = float(np.abs(r[7]) / LD(sn2) + np.abs(r[16]))
    return g, mag


def _finish(ops, name, d):
    from gp_ss_ak_amd import synth
    E, bias, sn2, n = np.array(synth.DEFAULT_EXPANS), synth.DEFAULT_BIAS, synth.DEFAULT_SN2, PAIR_N
    red, g = Mat(rng_for(name).standard_normal(17)), Mat(rng_for(name + "g").standard_normal(10))
    res = Result()
    if d == 3:                 # gpak_dev_grad_finish is _finish_d(..., 3, ...)
        g3 = Mat(g.was())
        res.rc("grad_finish", ops.call("grad_finish", list(E), bias, sn2, n, red, g3))
        res.rc("grad_finish_d", ops.call("grad_finish_d", list(E), bias, sn2, n, 3, red, g))
        res.rc("entries of grad_finish that differ from grad_finish_d(3)", int(np.count_nonzero(bits(g3.data) != bits(g.data))))
        res.rc("g[7] is not +0.0", int(bits(g.get()[7:8, 0].copy())[0] != 0))
    else:
        res.rc("grad_finish_d", ops.call("grad_finish_d", list(E), bias, sn2, n, d, red, g))
    ref, mag = finish_ld(E, bias, sn2, n, d, red.was()[:, 0])
    return res.add("g", g, ref, 4 * U * mag, True).add("red", red)


def _consts_vs_oracle(ops, name, comp):
    """gpak_dev_grad_consts through the oracle, which restates S % S_p on its own (expans_S_matrices): the ten gradient
    entries from the long-double pair sums (they carry M_p and m2 of gpak_dev_grad_consts) against orc.grad_ref_q on the
    symmetric Q of the same lower triangle."""
    from oracle import oracle as orc
    d = pair_data(ops, comp, 1)
    n, E = d.n, d.E
    M36, m2 = Mat(np.zeros(36)), Mat(np.zeros(18))
    res = Result().rc("grad_consts", ops.call("grad_consts", list(E), M36, m2))
    same = np.array_equal(bits(m2.data), bits(d.m2.ravel().copy())) and all(
        np.array_equal(M36.data[6 * p:6 * p + 6], d.Mp[p][[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]) for p in range(6))
    res.rc("constants differ from those the reference sums were made with", int(not same))
    ref16, b16 = d.expect(0, 0, 0)
    # the oracle's lp_dhyp sum is made from its own f = K alpha: the same in long double, from the true distances
    c = d.un[0][[0, 1, 2, 4]].astype(LD)
    K = LD(E[6]) ** 2 * np.exp(-np.sqrt(((c[:, :, None] - c[:, None, :]) ** 2).sum(axis=0))) + LD(d.bias)
    al = d.alpha[:n, 0].astype(LD)
    fl = K @ al
    dl = d.y.astype(LD) - fl
    red = np.concatenate([ref16, [(dl * dl / LD(d.sn2) - 1).sum()]])
    g = Mat(np.zeros(10))
    res.rc("grad_finish_d", ops.call("grad_finish_d", list(E), d.bias, d.sn2, n, d.d, red.astype(np.float64), g))
    Q = np.asfortranarray(d.B + np.tril(d.B, -1).T)
    go = orc.grad_ref_q(d.X, d.y, Q, d.alpha[:n, 0].copy(), E, d.bias, d.sn2, orc.DIST_DIRECT)
    # the oracle sums the same terms in float64 in another order: twice the case's own bound through the linear assembly
    # (4u of it for the assembly itself); its f carries (n + 2 + c0 + c1 sd) u |K| |alpha| per entry, and the lp_dhyp sum
    # (n + 2) u sum (d^2 / sn2 + 1) of its own
    df = (n + 2 + PAIR_C0 + PAIR_C1 * 4.0) * U * (np.abs(K) @ np.abs(al)).astype(np.float64)
    lp = float((2 * np.abs(dl).astype(np.float64) / d.sn2 * df).sum() + (n + 2) * U * float((dl * dl / LD(d.sn2) + 1).sum()))
    # M_p = S % S_p itself is rounded, in the library and in the oracle: |S| <= w, |S_p| <= 2 w (w = the largest inverse
    # width; the rows of Rot are unit vectors), S carries 8u w and S_p 16u w (three-term sums of products of rounded sines
    # and cosines), so M_p carries (16 + 16 + 2) u w^2 on either side: 68 u w^2 between the two
    eM = 68 * U * float(np.abs(E[[1, 3, 5]]).max()) ** 2
    bound = np.zeros(10)
    bound[:6] = 2 * b16[:6] + eM * d.mp_sens
    bound[6] = 2 * abs(2 * E[6]) * b16[6]
    bound[7] = 2 * 4 * b16[15] / n
    bound[8] = 2 * b16[8]
    bound[9] = 2 * b16[7] / d.sn2 + lp
    bound += 4 * U * finish_ld(E, d.bias, d.sn2, n, d.d, red)[1]
    return res.add("g", g, go.astype(LD), bound, True).add("M36", M36, free=True).add("m2", m2, free=True)


_AW, _EX = "as written", "exact"
for _mode, _mn in ((1, "direct"), (0, "expansion")):
    case("pairs", f"pair_sums[{_AW},P=0,expans+bias,{_mn}]", ["gpak_dev_grad_pair_sums", "gpak_dev_transform"], passno=0, P=0, a=0,
         comp="expans+bias", mode=_mode)(_pair_sums)
for _P in (1, 2, 3):
    for _a in range(_P):
        case("pairs", f"pair_sums[{_AW},P={_P},a={_a},expans+bias,direct]", ["gpak_dev_grad_pair_sums"], passno=0, P=_P, a=_a,
             comp="expans+bias", mode=1)(_pair_sums)
    if _P > 1:
        case("pairs", f"pair_sums[{_AW},P={_P},all ranks,expans+bias,direct]", ["gpak_dev_grad_pair_sums"], passno=0, P=_P,
             comp="expans+bias", mode=1)(_pair_rank_sum)
case("pairs", f"pair_sums[{_AW},P=3,a=1,expans+bias,expansion]", ["gpak_dev_grad_pair_sums"], passno=0, P=3, a=1,
     comp="expans+bias", mode=0)(_pair_sums)
for _c in ("expans d4", "expans+rbf", "exp+rbf", "expans+exp+rbf"):
    case("pairs", f"pair_sums[{_AW},P=0,{_c},direct]", ["gpak_dev_grad_pair_sums", "gpak_dev_transform_k"], passno=0, P=0, a=0,
         comp=_c, mode=1)(_pair_sums)
for _c in PAIR_COMPS:
    case("pairs", f"pair_sums[{_EX},P=0,{_c},direct]", ["gpak_dev_grad_pair_sums"], passno=1, P=0, a=0, comp=_c, mode=1)(_pair_sums)
case("pairs", f"pair_sums[{_EX},P=2,a=1,expans+rbf,direct]", ["gpak_dev_grad_pair_sums"], passno=1, P=2, a=1, comp="expans+rbf",
     mode=1)(_pair_sums)
case("pairs", f"pair_sums[{_EX},P=2,all ranks,expans+rbf,direct]", ["gpak_dev_grad_pair_sums"], passno=1, P=2, comp="expans+rbf",
     mode=1)(_pair_rank_sum)
for _ps, _pn in ((0, _AW), (1, _EX)):
    case("pairs", f"pair_sums[{_pn},P=3,a=2,n=129,Np=256]->no tile", ["gpak_dev_grad_pair_sums"], passno=_ps, P=3, a=2,
         comp="expans+bias", mode=1, n=129, Np=256)(_pair_sums)
    case("pairs", f"pair_sums[{_pn},P=0,n=640=Np]", ["gpak_dev_grad_pair_sums"], passno=_ps, P=0, a=0, comp="expans+bias", mode=1,
         n=640, Np=640)(_pair_sums)
for _w in ("pass", "a", "ld", "two expans", "white"):
    case("pairs", f"pair_sums[bad {_w}]->EINVAL", ["gpak_dev_grad_pair_sums"], what=_w)(_pair_refused)
for _c in ("expans+bias", "expans d4"):
    case("pairs", f"pairs_rows[P=3,a=1,{_c}]", ["gpak_dev_grad_pairs_rows", "gpak_dev_grad_pair_sums"], comp=_c)(_pairs_rows)
    case("pairs", f"grad_consts via the oracle[{_c}]", ["gpak_dev_grad_consts", "gpak_dev_grad_finish_d"], comp=_c)(_consts_vs_oracle)
for _d in (3, 4):
    case("pairs", f"grad_finish[d={_d}]", ["gpak_dev_grad_finish", "gpak_dev_grad_finish_d"] if _d == 3 else ["gpak_dev_grad_finish_d"],
         d=_d)(_finish)


# ---- the panel factorisation alone (group `panel`: gpak_dev_factor_panel_co) ------------------------------------------
def chol_ld(A):
    """lower Cholesky factor of a symmetric float64 matrix (its lower triangle is read) in long double: 128-column steps,
    the products through mm_ld.  Returns (L, [inverse of each 128 x 128 diagonal block of L])."""
    W = A.shape[0]
    L = (np.tril(A) + np.tril(A, -1).T).astype(LD)
    invs = []
    for j in range(0, W, TILE):
        D = L[j:j + TILE, j:j + TILE]
        for c in range(TILE):
            D[c, c] = np.sqrt(D[c, c] - D[c, :c] @ D[c, :c])
            D[c + 1:, c] = (D[c + 1:, c] - D[c + 1:, :c] @ D[c, :c]) / D[c, c]
            D[c, c + 1:] = 0
        invs.append(tri_inv_ld(D))
        if j + TILE < W:
            P = mm_ld(L[j + TILE:, j:j + TILE], invs[-1])
            L[j + TILE:, j:j + TILE] = P
            L[j + TILE:, j + TILE:] -= mm_ld(P, P)
    return np.tril(L), invs


def rows_ld(P, L, invs):
    """P L^-T in long double by block forward substitution with the 128-block inverses of chol_ld"""
    X = P.astype(LD)
    W = L.shape[0]
    for j in range(0, W, TILE):
        X[:, j:j + TILE] = mm_ld(X[:, j:j + TILE], invs[j // TILE])
        if j + TILE < W:
            X[:, j + TILE:] -= mm_ld(X[:, j:j + TILE], L[j + TILE:, j:j + TILE])
    return X


def panel_operands(W, below):
    """(A = G G^T / W + 2 I, the rows below: standard_normal, a junk upper triangle) -- functions of W (and `below`) alone,
    so that every J and either build share one reference"""
    def make():
        rng = rng_for(f"panel-group[W={W}]")
        G = rng.standard_normal((W, W))
        A = G @ G.T / W + 2.0 * np.eye(W)
        A = np.tril(A) + np.tril(A, -1).T
        junk = 1e3 * rng.standard_normal((W, W))
        return A, junk
    A, junk = memo(("panel-A", W), make)
    P = memo(("panel-P", W, below), lambda: rng_for(f"panel-group[W={W},below={below}]").standard_normal((below, W)))
    return A, P, junk


def panel_reference(W, below):
    """long double: L, P L^-T, the inverses of the 128-blocks; the scales the errors are relative to (|L^-1|-type, as
    subst_bound's); and the float64 restatement of the device's blocked algorithm (np_engine.blocked_factor_panel) on the
    same input, whose error against long double sets the tolerance"""
    def make():
        from np_engine import blocked_factor_panel
        A, P, _junk = panel_operands(W, below)
        L, invs = memo(("panel-chol", W), lambda: chol_ld(A))
        X = rows_ld(P, L, invs) if below else np.zeros((0, W), dtype=LD)
        L64 = L.astype(np.float64)
        aL = np.abs(L64)
        aLi = np.abs(np.linalg.inv(L64))
        # first-order error of a Cholesky factor: dL = L tril(L^-1 dA L^-T) with |dA| <= c u |L| |L^T|
        sL = np.tril(aL @ np.tril(aLi @ (aL @ aL.T) @ aLi.T))
        # the rows below carry their own substitution error and the factor's: P L^-T dL^T L^-T
        pl = np.abs(P) @ aLi.T
        sP = pl + pl @ sL.T @ aLi.T
        sI = []
        for k in range(W // TILE):
            c = slice(k * TILE, (k + 1) * TILE)
            Xk = np.abs(invs[k]).astype(np.float64)
            sI.append(Xk @ (aL[c, c] + sL[c, c]) @ Xk)       # the inversion's own |X| |L| |X| and the factor's error through it
        M = np.vstack([A, P])
        inv = np.zeros((W // TILE, 2, TILE, TILE))
        assert blocked_factor_panel(M, W, inv, 0) == []
        return dict(L=L, X=X, invs=invs, sL=sL, sP=sP, sI=sI, numL=np.tril(M[:W]), numP=M[W:], numI=inv)
    return memo(("panel-ref", W, below), make)


def _ratio(num, ref, scale):
    err = np.abs(np.asarray(num, dtype=LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / scale)
    return float(r.max()) if r.size else 0.0


def panel_input(A_upper, A, P, J, Np, ld):
    """the block column as it goes in: the sentinel above row J, the lower triangle of A with `A_upper` above the diagonal,
    the rows below"""
    W = A.shape[0]
    M = np.empty((Np, W))
    M[:] = sentinel(1)[0]
    M[J:J + W] = np.tril(A) + np.triu(A_upper, 1)
    M[J + W:] = P
    return Mat(M, ld)


def upper16(W):
    """elements of the W x W block above the diagonal: inside the diagonal 16 x 16 tiles (exact zeros come back); in the
    16-tiles above the diagonal of a diagonal 128-block (the block kernel neither reads nor writes them, but the in-panel
    update of a later diagonal 128-tile is a whole-tile product and does: scratch); in the 128-tiles strictly above the
    diagonal (never written: they keep their bits)"""
    i, j = np.arange(W)[:, None], np.arange(W)[None, :]
    return (i < j) & (i // 16 == j // 16), (i // 16 < j // 16) & (i // TILE == j // TILE), i // TILE < j // TILE


def _panel(ops, name, W, J, below, mirror=False):
    """gpak_dev_factor_panel_co alone: accuracy against long double, what it writes, either build, a junk upper triangle"""
    A, P, junk = panel_operands(W, below)
    ref = panel_reference(W, below)
    Np, nblk = J + W + below, W // TILE
    ld = Np + 32
    res = Result()

    def run(upper, co, label):
        blk, inv = panel_input(upper, A, P, J, Np, ld), Mat(sentinel(nblk * 2 * TILE * TILE))
        info = np.full(4, INT_MAX, dtype=np.int32)
        res.rc(label, ops.call("factor_panel_co", blk, ld, Np, J, W, inv, info, co))
        res.rc(label + ": info stays INT_MAX", int(info[0] != INT_MAX or (info[1:] != INT_MAX).any()))
        return blk, inv

    blk, inv = run(junk, 0, "factor_panel_co")
    blk1, inv1 = run(junk, 1, "factor_panel_co[coresident]")
    res.rc("coresident: the same bits", int(not (np.array_equal(bits(blk.full), bits(blk1.full))
                                                  and np.array_equal(bits(inv.full), bits(inv1.full)))))
    zero16, scratch16, keep128 = upper16(W)
    pad = lambda m, fill: np.vstack([np.full((J, W), fill, dtype=bool), m, np.full((below, W), not fill, dtype=bool)])
    if mirror:                # only the lower triangle is read: a symmetric input gives the same bits where the call writes
        blk2, inv2 = run(A, 0, "factor_panel_co[symmetric input]")
        wr = pad(~(scratch16 | keep128), False)
        res.rc("junk above the diagonal: the same bits", int(not (np.array_equal(bits(blk.get()[wr]), bits(blk2.get()[wr]))
                                                                 and np.array_equal(bits(inv.full), bits(inv2.full)))))
    # ---- the tolerance: 8 x the restatement's worst error against long double, relative to the scales
    rL = _ratio(ref["numL"], ref["L"], ref["sL"])
    rP = _ratio(ref["numP"], ref["X"], ref["sP"])
    rI = max(_ratio(ref["numI"][k, 1], ref["invs"][k], ref["sI"][k]) for k in range(nblk))
    res.info["numpy_vs_longdouble[L]"], res.info["numpy_vs_longdouble[P]"], res.info["numpy_vs_longdouble[inv]"] = rL, rP, rI
    full_ref = np.zeros((Np, W), dtype=LD)
    full_ref[J:J + W], full_ref[J + W:] = ref["L"], ref["X"]
    bound = np.zeros((Np, W))
    bound[J:J + W], bound[J + W:] = 8.0 * rL * ref["sL"], 8.0 * rP * ref["sP"]
    # rows above J and the 128-tiles above the diagonal: bit-identical
    res.add("blk", blk, full_ref, bound, pad(~(scratch16 | keep128), False), free=np.vstack([np.zeros((J, W), dtype=bool), scratch16, np.zeros((below, W), dtype=bool)]))
    iref, ibound = np.zeros((nblk, 2, TILE, TILE), dtype=LD), np.zeros((nblk, 2, TILE, TILE))
    for k in range(nblk):
        iref[k, 0], iref[k, 1] = ref["invs"][k].T, ref["invs"][k]          # memory [c][r] of L^-1, then of L^-T
        ibound[k, 0], ibound[k, 1] = 8.0 * rI * ref["sI"][k].T, 8.0 * rI * ref["sI"][k]
    res.add("inv", inv, iref.reshape(-1, 1), ibound.reshape(-1, 1), True)
    iv = inv.data.reshape(nblk, 2, TILE, TILE)
    res.rc("inv: the second image is the transpose of the first, in bits",
           int(not all(np.array_equal(bits(iv[k, 1]), bits(iv[k, 0].T.copy())) for k in range(nblk))))
    out = blk.get()[J:J + W]
    res.rc("exact zeros above the diagonal of the diagonal 16-tiles", int(bits(out[zero16].copy()).any()))
    # ---- the residual on the diagonal block, in long double
    Lh = np.tril(out)
    rb = (W + 2) * U * (np.abs(Lh) @ np.abs(Lh).T)
    low = np.tril(np.ones((W, W), dtype=bool))

    def resid(Lx):
        return np.abs(A.astype(LD) - mm_ld(Lx, Lx)).astype(np.float64)
    rR = float((memo(("panel-resid", W), lambda: resid(ref["numL"]))[low] / ((W + 2) * U * (np.abs(ref["numL"]) @ np.abs(ref["numL"]).T))[low]).max())
    res.info["numpy_residual_ratio"] = rR
    res.add("residual", Mat(np.where(low, resid(Lh), 0.0)), 0.0, 8.0 * rR * rb, low)
    return res


for _W in (128, 256, 512):
    for _J in (0, 384):
        for _b in (0, 128, 640):
            case("panel", f"factor_panel[W={_W},J={_J},below={_b}]", ["gpak_dev_factor_panel_co"], W=_W, J=_J, below=_b,
                 mirror=(_b == 128))(_panel)
for _J, _b in ((0, 128), (384, 640), (384, 0)):
    case("panel", f"factor_panel[W=1024,J={_J},below={_b}]", ["gpak_dev_factor_panel_co"], W=1024, J=_J, below=_b,
         mirror=(_b == 128))(_panel)


PANEL_INFO_W, PANEL_INFO_J, PANEL_INFO_BELOW = 512, 384, 128
PANEL_INFO_K = (0, 15, 16, 127, 128, 300, 511)


def _panel_info(ops, name, what):
    """*info of gpak_dev_factor_panel_co: pre-set by the caller, gets the MINIMUM failing global column (1-based); the
    status travels in it, the return code is GPAK_OK."""
    import failcol_ref as fr
    W, J, below = PANEL_INFO_W, PANEL_INFO_J, PANEL_INFO_BELOW
    Np = J + W + below
    ld = Np + 32
    L = memo(("panel-info-L", W), lambda: fr.ldl_factor(W, 20260305))
    P = memo(("panel-info-P", W), lambda: rng_for("panel-info").standard_normal((below, W)))
    res = Result()

    def run(A, preset, co=0):
        blk, inv = panel_input(A, A, P, J, Np, ld), Mat(sentinel(W // TILE * 2 * TILE * TILE))
        info = np.full(4, INT_MAX, dtype=np.int32)
        info[0] = preset
        res.rc(f"{name}: return code", ops.call("factor_panel_co", blk, ld, Np, J, W, inv, info, co))
        res.rc(f"{name}: the ints beside info", int((info[1:] != INT_MAX).any()))
        res.add("blk", blk, free=np.arange(Np)[:, None] >= J).add("inv", inv, free=True)     # guards, skew rows, rows above J
        return int(info[0]), blk

    def want(label, got, expected):
        res.rc(f"{name}: {label}", got, expected)

    good = L @ L.T
    if what == "success":
        want("a success leaves INT_MAX", run(good, INT_MAX)[0], INT_MAX)
        want("a success leaves a pre-set 5", run(good, 5)[0], 5)
        want("a success leaves INT_MAX [coresident]", run(good, INT_MAX, 1)[0], INT_MAX)
        return res
    if what in ("-1", "0", "nan"):
        d = {"-1": -1.0, "0": 0.0, "nan": np.nan}[what]
        for k in PANEL_INFO_K:
            A = fr.ldl_panel(L, k, d)
            fr.assert_ldl_discriminates(A, k, d)                   # the fixture first, on the CPU
            for co in (0, 1):
                want(f"D[{k}] = {what}, coresident {co}", run(A, INT_MAX, co)[0], J + k + 1)
        return res
    if what == "two failures":
        # blockdiag of two L D L^T blocks: the first fails at k1 (in the first 128-block), the second at k2 (in the third)
        k1, k2, h = 70, 40, W // 2
        La, Lb = fr.ldl_factor(h, 11), fr.ldl_factor(h, 12)
        A = np.zeros((W, W))
        A[:h, :h], A[h:, h:] = fr.ldl_panel(La, k1), fr.ldl_panel(Lb, k2)
        assert fr.reference_info(A) == k1 + 1 and fr.reference_info(A[h:, h:]) == k2 + 1
        for co in (0, 1):
            want(f"the first of two failures, coresident {co}", run(A, INT_MAX, co)[0], J + k1 + 1)
        want("the second alone", run(np.block([[La @ La.T, np.zeros((h, h))], [np.zeros((h, h)), A[h:, h:]]]), INT_MAX)[0], J + h + k2 + 1)
        return res
    if what == "pre-set":
        k = 300
        A = fr.ldl_panel(L, k)
        fr.assert_ldl_discriminates(A, k, -1.0)
        want("a pre-set value below the failing column survives", run(A, J + k - 2)[0], J + k - 2)
        want("a pre-set value above it is replaced", run(A, J + k + 50)[0], J + k + 1)
        want("a pre-set value equal to it stays", run(A, J + k + 1)[0], J + k + 1)
        return res
    assert what == "flip"
    # a 1 -> -1 flip of one D entry changes nothing left of column k: columns [0, k) of the block column (the rows below
    # included) come back with the bits of the successful factorisation of the same L
    _i, ok = run(good, INT_MAX)
    for k in (15, 16, 127, 128, 300, 511):
        A = fr.ldl_panel(L, k)
        assert np.array_equal(bits(np.tril(A)[:, :k].copy()), bits(np.tril(good)[:, :k].copy()))
        got, bad = run(A, INT_MAX)
        want(f"flip at {k}: info", got, J + k + 1)
        a, b = ok.get()[J:, :k], bad.get()[J:, :k]
        low = np.arange(Np - J)[:, None] >= np.arange(k)[None, :]
        diff = (bits(a.copy()) != bits(b.copy())) & low
        res.info[f"first column that differs, flip at {k}"] = float(np.argmax(diff.any(axis=0)) if diff.any() else k)
        want(f"flip at {k}: columns [0, {k}) keep their bits", int(diff.any()), 0)
    return res


for _what in ("success", "-1", "0", "nan", "two failures", "pre-set", "flip"):
    case("panel", f"factor_panel info[{_what}]", ["gpak_dev_factor_panel_co"], what=_what)(_panel_info)


# ---- the fp32 prediction kernels alone (group `f32`: include/gpak_dev_f32.h) ---------------------------------------
# u32 = 2^-24, u64 = 2^-53; references in long double on the float operands taken exactly.  Derivations: the module
# docstring, "The fp32 prediction kernels alone".
F32_BUILDS = {       # the GPAK_F32_* environment of each build the launcher of csrc/gemm_f32.hip can pick
    "wide,rsd=2": {"GPAK_F32_RSD": "2"}, "wide,rsd=4": {}, "wide,rsd=8": {"GPAK_F32_RSD": "8"},
    "wide,rsd=16": {"GPAK_F32_RSD": "16"}, "plain": {"GPAK_F32_ACC": "plain"},
    "plain,tile=64": {"GPAK_F32_ACC": "plain", "GPAK_F32_TILE": "64"},
}
F32_WIDE = tuple(b for b in F32_BUILDS if b.startswith("wide"))
F32_SHAPES = ((1, 1, 128), (2, 1, 128), (3, 2, 128), (1, 1, 256), (2, 3, 384), (9, 9, 256), (17, 1, 640))
F32_AB = ((1.0, 0.0), (-1.0, 1.0), (0.75, -0.5))
F32_POS_K = 4096


def f32_sum_k(A, B, k0, k1, sequential):
    """sum over k in [k0, k1) of A[:, k] B[:, k] in float32: each product rounded, then added, one k at a time
    (sequential), or in the order of the host's float32 BLAS"""
    if not sequential:
        return np.asarray(A[:, k0:k1] @ B[:, k0:k1].T, dtype=F32)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=F32)
    for k in range(k0, k1):
        acc += np.multiply.outer(A[:, k], B[:, k])
    return acc


def f32_product(A, B, alpha, beta, C0, wide, sequential=False):
    """beta C0 + alpha A B^T as csrc/gemm_f32.hip forms it.  wide (and K > 128): chunks of 128 accumulated in float32 from
    zero, the chunk sums added in float64, alpha * total + beta * C0 in float64, rounded once.  Otherwise one float32 sum
    over all of K, alpha * sum rounded, then the fused beta * C0 + that.  beta == 0 never reads C0."""
    A, B = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(B, dtype=F32)
    K = A.shape[1]
    if wide and K > TILE:
        tot = np.zeros((A.shape[0], B.shape[0]))
        for c in range(0, K, TILE):
            tot += f32_sum_k(A, B, c, min(K, c + TILE), sequential).astype(np.float64)
        v = float(alpha) * tot
        if beta != 0:
            v = v + float(beta) * np.asarray(C0, dtype=np.float64)
        return v.astype(F32)
    v = F32(alpha) * f32_sum_k(A, B, 0, K, sequential)
    if beta != 0:
        v = (float(beta) * np.asarray(C0, dtype=np.float64) + v.astype(np.float64)).astype(F32)
    return v


def f32_ladder(W, Lf, iv, levels, wide, sequential=False, mut=()):
    """fs_block_f32 (csrc/predict.hip) in float32 on W (mrows x Np), in place: a block of width lv[k] child by child of
    width lv[k-1] (the last one clipped), W_j := W_j inv(D_j)^T at 128 columns, after each child ONE update of the rest of
    the block.  iv: (Np / 128, 2, 128, 128), the pairs of inverse blocks as they lie in memory."""
    lv = list(levels) or [TILE, 512]
    Np = W.shape[1]
    lv.append(Np if Np > lv[-1] else lv[-1] + 1)

    def block(J0, Wd, k):
        if k == 0:
            c = slice(J0, J0 + TILE)
            Binv = iv[J0 // TILE, 1 if "f32 inv transposed" in mut else 0].T      # B[n, k] = memory[n + 128 k]
            W[:, c] = f32_product(W[:, c], Binv, 1.0, 0.0, None, wide, sequential)
            return
        cw = lv[k - 1]
        for j0 in range(J0, J0 + Wd, cw):
            w = min(cw, J0 + Wd - j0)
            if not ("f32 clip skipped" in mut and w < cw):
                block(j0, w, k - 1)
            if J0 + Wd - j0 - w > 0:
                rest = slice(j0 + w, J0 + Wd)
                W[:, rest] = f32_product(W[:, j0:j0 + w], Lf[rest, j0:j0 + w], -1.0, 1.0, W[:, rest], wide, sequential)
    block(0, Np, len(lv) - 1)
    return W


class F32Restated:
    """The operations of include/gpak_dev_f32.h restated in NumPy float32 / float64 on the cases' buffers.  mut: deliberate
    faults (test_the_checks_bite)."""

    def __init__(self, mut=()):
        self.mut, self.wide = tuple(mut), True

    @staticmethod
    def _view(x, rows, cols, ld):
        return pay(x)[:cols * ld].reshape(cols, ld).T[:rows]

    def gemm_nt_f32(self, mt, nt, K, alpha, A, lda, B, ldb, beta, Cm, ldc):
        m, n = mt * TILE, nt * TILE
        a, b = self._view(A, m, K, lda).copy(), self._view(B, n, K, ldb).copy()
        Cv = self._view(Cm, m, n, ldc)
        c0 = Cv.copy()
        if "f32 short k" in self.mut and K > TILE:
            K -= TILE
        plain = "f32 plain" in self.mut
        v = f32_product(a[:, :K], b[:, :K], alpha, beta, c0, self.wide and not plain, sequential=plain)
        if "f32 beta0" in self.mut and beta == 0:
            v = v + F32(0) * c0
        if "f32 unpermuted" in self.mut:      # MFMA tile i of a wave's 64 rows holds the rows 4 j + i
            v = v.reshape(m // 64, 16, 4, n).transpose(0, 2, 1, 3).reshape(m, n)
        Cv[...] = v
        return OK

    def fill_f32(self, uP, capP, nP, uQ, capQ, nQ, rows_p, cols_p, kern, bias, mode, Cm, ld):
        from np_engine import NumpyEngine
        terms, white = NumpyEngine.decode_kern(kern) if mode & HYB else ([(0, [float(t) for t in kern[:8]])], 0.0)
        up, uq = pay(uP)[:15 * capP].reshape(15, capP), pay(uQ)[:15 * capQ].reshape(15, capQ)
        keep = nP + 1 if ("f32 pair kept" in self.mut and nP & 1 and nP < rows_p) else nP
        sel = [0, 1, 2] if "f32 no col4" in self.mut else [0, 1, 2, 4]
        k = np.full((keep, nQ), F32(bias), dtype=F32)
        with np.errstate(invalid="ignore"):
            for t, (kind, p) in enumerate(terms):
                P, Q = up[5 * t:5 * t + 5][sel][:, :keep], uq[5 * t:5 * t + 5][sel][:, :nQ]
                d = ((P[:, :, None] - Q[:, None, :]) ** 2).sum(axis=0).astype(F32)      # the distance in float64, rounded once
                if kind == 2 and "f32 rbf as exp" not in self.mut:
                    k += F32(p[2] * p[2]) * np.exp((F32(-0.5) * F32(p[1])) * d)
                else:
                    k += F32((p[6] if kind == 0 else p[2] if kind == 2 else p[1]) ** 2) * np.exp(-np.sqrt(d))
                if "f32 white" in self.mut and t == 0:
                    k += np.where(d == 0, F32(white), F32(0))
        out = np.zeros((rows_p, cols_p), dtype=F32)
        out[:keep, :nQ] = k
        self._view(Cm, rows_p, cols_p, ld)[...] = out
        return OK

    def lower_to_f32(self, L, ld, Np, out, ldo):
        Lv = self._view(L, Np, Np, ld)
        low = np.arange(Np)[:, None] >= np.arange(Np)[None, :]
        with np.errstate(all="ignore"):
            self._view(out, Np, Np, ldo)[...] = np.where(low, np.where(low, Lv, 0.0).astype(F32), F32(0))
        return OK

    def vec_to_f32(self, vin, n, out):
        with np.errstate(all="ignore"):
            pay(out)[:n] = pay(vin)[:n].astype(F32)
        return OK

    def rowsumsq_f32(self, V, ldv, rows, cols, splits, part, part_ld):
        Vv = self._view(V, rows, cols, ldv).astype(np.float64)
        cps = (cols + splits - 1) // splits
        pv = pay(part)[:splits * part_ld].reshape(splits, part_ld)
        for s in range(splits):
            c0, c1 = s * cps, min(cols, (s + 1) * cps)
            if "f32 odd tail" in self.mut and (c1 - c0) & 1:
                c1 -= 1
            pv[s, :rows] = (Vv[:, c0:c1] ** 2).sum(axis=1) if c1 > c0 else 0.0
        return OK

    def fwd_subst_f32(self, Wt, ldw, mrows, Np, Lf, ldLf, invf, levels, nlevels):
        Wv = self._view(Wt, mrows, Np, ldw)
        iv = pay(invf)[:Np // TILE * 2 * TILE * TILE].reshape(Np // TILE, 2, TILE, TILE)
        Wv[...] = f32_ladder(Wv.copy(), self._view(Lf, Np, Np, ldLf).copy(), iv, list(levels)[:nlevels], self.wide, mut=self.mut)
        return OK


# -- the product -------------------------------------------------------------------------------------
def f32_operands(mt, nt, K):
    """A with row scales 10^-3 .. 10^3 (a permuted row shows), B and C standard_normal, all float32; A B^T in long double"""
    def make():
        rng = rng_for(f"gemm_nt_f32[{mt},{nt},{K}]")
        A = (rng.standard_normal((mt * TILE, K)) * 10.0 ** rng.integers(-3, 4, (mt * TILE, 1))).astype(F32)
        B, C0 = rng.standard_normal((nt * TILE, K)).astype(F32), rng.standard_normal((mt * TILE, nt * TILE)).astype(F32)
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        return A, B, C0, mm_ld(A64, B64), np.abs(A64) @ np.abs(B64).T
    return memo(("f32 operands", mt, nt, K), make)


def f32_bound(wide, K, alpha, beta, aprod, C0, exact):
    mag = abs(alpha) * aprod + abs(beta) * np.abs(C0)
    if wide:
        return 130 * U32 * abs(alpha) * aprod + U32 * np.abs(exact).astype(np.float64) + (K // TILE + 3) * U * mag
    return (K + 2) * U32 * mag


def _gemm_f32(ops, name, build, mt, nt, K):
    env = F32_BUILDS[build]
    wide = build in F32_WIDE
    A0, B0, C00, prod, aprod = f32_operands(mt, nt, K)
    m, n = mt * TILE, nt * TILE
    lda, ldb, ldc = m + 36, n + 40, m + 44
    res = Result()
    ops.f32_build(env)
    try:
        for alpha, beta in F32_AB:
            A, B = Mat(A0, lda, F32), Mat(B0, ldb, F32)
            Cm = Mat(np.full((m, n), np.nan) if beta == 0 else C00, ldc, F32)      # beta == 0: C is never read
            res.rc(f"gemm_nt_f32[{alpha},{beta}]", ops.call("gemm_nt_f32", mt, nt, K, alpha, A, lda, B, ldb, beta, Cm, ldc))
            c0 = np.zeros((m, n)) if beta == 0 else C00.astype(np.float64)
            exact = LD(alpha) * prod + LD(beta) * c0
            res.add(f"C[{alpha},{beta}]", Cm, exact, f32_bound(wide, K, alpha, beta, aprod, c0, exact), True)
            res.add(f"A[{alpha},{beta}]", A).add(f"B[{alpha},{beta}]", B)
        if nt == 1 and K == TILE:              # the inverse product of the ladder: A == C, alpha = 1, beta = 0
            A, B = Mat(A0, lda, F32), Mat(B0, ldb, F32)
            res.rc("gemm_nt_f32[in place]", ops.call("gemm_nt_f32", mt, 1, K, 1.0, A, lda, B, ldb, 0.0, A, lda))
            res.add("A=C[in place]", A, prod, f32_bound(wide, K, 1.0, 0.0, aprod, np.zeros((m, n)), prod), True).add("B[in place]", B)
    finally:
        ops.f32_build()
    return res


for _b in F32_BUILDS:
    for _mt, _nt, _K in F32_SHAPES:
        case("f32", f"gemm_nt_f32[{_b}][{_mt},{_nt},{_K}]", ["gpak_dev_gemm_nt_f32"], build=_b, mt=_mt, nt=_nt, K=_K)(_gemm_f32)


def _gemm_f32_agree(ops, name, mt, nt, K):
    """The four wide builds differ in the prefetch ring and the occupancy only: per accumulator the same MFMAs in the
    same order, the same float64 additions, the same epilogue -- the same bits."""
    A0, B0, C00, _prod, _aprod = f32_operands(mt, nt, K)
    m, n = mt * TILE, nt * TILE
    lda, ldb, ldc = m + 36, n + 40, m + 44
    res, first = Result(), None
    try:
        for b in F32_WIDE:
            ops.f32_build(F32_BUILDS[b])
            A, B, Cm = Mat(A0, lda, F32), Mat(B0, ldb, F32), Mat(C00, ldc, F32)
            res.rc(b, ops.call("gemm_nt_f32", mt, nt, K, 0.75, A, lda, B, ldb, -0.5, Cm, ldc))
            first = Cm if first is None else first
            res.rc(f"elements of {b} that differ from {F32_WIDE[0]}", int(np.count_nonzero(bits(Cm.full) != bits(first.full))))
            res.add(b, Cm, free=True)
    finally:
        ops.f32_build()
    return res


for _mt, _nt, _K in ((2, 3, 384), (9, 9, 256)):
    case("f32", f"gemm_nt_f32[the wide builds agree][{_mt},{_nt},{_K}]", ["gpak_dev_gemm_nt_f32"], mt=_mt, nt=_nt, K=_K)(_gemm_f32_agree)


def f32_positive():
    """(2, 1, F32_POS_K) with both operands uniform on [0.5, 1.5): every term positive, a running float32 sum grows
    linearly.  The worst error relative to sum|terms| of the chunked and of the plain restatement against long double."""
    def make():
        rng, K = rng_for("gemm_nt_f32[positive]"), F32_POS_K
        A, B = rng.uniform(0.5, 1.5, (2 * TILE, K)).astype(F32), rng.uniform(0.5, 1.5, (TILE, K)).astype(F32)
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        exact = sum(mm_ld(A64[:, c:c + 2048], B64[:, c:c + 2048]) for c in range(0, K, 2048))
        s = exact.astype(np.float64)                                    # = sum|terms|
        err = lambda v: float((np.abs(v.astype(LD) - exact).astype(np.float64) / s).max())
        chunked = err(f32_product(A, B, 1.0, 0.0, None, True, sequential=True))
        plain = err(f32_product(A, B, 1.0, 0.0, None, False, sequential=True))
        return A, B, exact, s, chunked, plain
    return memo(("f32 positive",), make)


def _gemm_f32_is_wide(ops, name, build):
    A0, B0, exact, s, chunked, plain = f32_positive()
    tol = 8.0 * chunked                                                 # the house rule, relative to sum|terms|
    K, lda, ldb, ldc = F32_POS_K, 2 * TILE + 36, TILE + 40, 2 * TILE + 44
    res = Result()
    res.info["chunked restatement: error / (u32 sum|terms|)"] = chunked / U32
    res.info["plain restatement: error / (u32 sum|terms|)"] = plain / U32
    res.info["plain / tolerance"] = plain / tol
    res.rc("the plain restatement is within 2 x the tolerance: the input does not discriminate", int(plain < 2 * tol))
    ops.f32_build(F32_BUILDS[build])
    try:
        A, B, Cm = Mat(A0, lda, F32), Mat(B0, ldb, F32), Mat(np.full((2 * TILE, TILE), np.nan), ldc, F32)
        res.rc("gemm_nt_f32", ops.call("gemm_nt_f32", 2, 1, K, 1.0, A, lda, B, ldb, 0.0, Cm, ldc))
    finally:
        ops.f32_build()
    return res.add("C", Cm, exact, tol * s, True).add("A", A).add("B", B)


for _b in F32_WIDE:
    case("f32", f"gemm_nt_f32[{_b}][accumulates wide]", ["gpak_dev_gemm_nt_f32"], build=_b)(_gemm_f32_is_wide)


def _gemm_f32_refused(ops, name):
    rng = rng_for(name)
    m, K = TILE, 2 * TILE
    lda = m + 36
    A, B, Cm = (Mat(rng.standard_normal((m, K)).astype(F32), lda, F32) for _ in range(3))
    res = Result()
    call = lambda label, want, *a: res.rc(label, ops.call("gemm_nt_f32", *a), want)
    call("K=64", EINVAL, 1, 1, 64, 1.0, A, lda, B, lda, 0.0, Cm, lda)
    call("K=192", EINVAL, 1, 1, 192, 1.0, A, lda, B, lda, 0.0, Cm, lda)
    call("K=0", EINVAL, 1, 1, 0, 1.0, A, lda, B, lda, 0.0, Cm, lda)
    call("lda no multiple of 4", EINVAL, 1, 1, TILE, 1.0, A, lda + 2, B, lda, 0.0, Cm, lda)
    call("ldb below the rows", EINVAL, 1, 1, TILE, 1.0, A, lda, B, TILE - 4, 0.0, Cm, lda)
    call("ldc below the rows", EINVAL, 1, 2, TILE, 1.0, A, lda, B, lda, 0.0, Cm, TILE - 4)
    call("A misaligned", EINVAL, 1, 1, TILE, 1.0, Off(A, 1), lda, B, lda, 0.0, Cm, lda)
    call("C misaligned", EINVAL, 1, 1, TILE, 1.0, A, lda, B, lda, 0.0, Off(Cm, 2), lda)
    call("A == C, nt=2", EINVAL, 1, 2, TILE, 1.0, A, lda, B, lda, 0.0, A, lda)
    call("A == C, K=256", EINVAL, 1, 1, K, 1.0, A, lda, B, lda, 0.0, A, lda)
    call("mt=0", OK, 0, 1, TILE, 1.0, A, lda, B, lda, 0.0, Cm, lda)
    call("nt=0", OK, 1, 0, TILE, 1.0, A, lda, B, lda, 0.0, Cm, lda)
    return res.add("A", A).add("B", B).add("C", Cm)


case("f32", "gemm_nt_f32->EINVAL / no-op", ["gpak_dev_gemm_nt_f32"])(_gemm_f32_refused)


# -- the cross-kernel fill ----------------------------------------------------------------------------
FILL32_NP, FILL32_ROWS, FILL32_NQ, FILL32_COLS = 131, 256, 70, 128
FILL32_TWIN = (130, 33)                # P[130] (the last valid row: a lane's first element) == Q[33]
FILL32_C0, FILL32_C1 = 10.0, 12.0      # the module docstring derives them
FILL32_COMPS = {                       # name -> (terms, input columns, Sigma_White)
    "expans": ([(0, None)], 3, 0.0), "expans+exp": ([(0, None), (1, EXP_P)], 3, 0.0), "rbf": ([(2, RBF_P)], 3, 0.0),
    "expans+rbf+bias,white=0.1": (HYB_TERMS, 3, HYB_WHITE), "expans+exp+rbf": ([(0, None), (1, EXP_P), (2, RBF_P)], 3, 0.0),
    "expans d4": ([(0, None)], 4, 0.0),
}


class Fill32Data:
    """nP test-side and nQ train-side drill-hole points, one pair coincident, transformed by the engine under test; rows
    from n on of every transformed array hold the sentinel.  The cross-kernel in long double and its bound."""

    def __init__(self, ops, comp):
        from gp_ss_ak_amd import synth
        terms, cols, white = FILL32_COMPS[comp]
        E = np.array(synth.DEFAULT_EXPANS, dtype=np.float64)
        self.terms = [(k, list(E) if p is None else list(p)) for k, p in terms]
        self.bias, self.white = synth.DEFAULT_BIAS, white
        nP, nQ, capP, capQ = FILL32_NP, FILL32_NQ, FILL32_ROWS, FILL32_COLS
        self.hyb = not (len(terms) == 1 and terms[0][0] == 0)
        self.mode = 1 | (D4 if cols == 4 else 0) | (HYB if self.hyb else 0)
        self.kern = serialise(self.terms, white) if self.hyb else list(E)
        self.kern_no_white = serialise(self.terms, 0.0) if self.hyb else list(E)
        X, _y = synth.drillholes4(nP + nQ) if cols == 4 else synth.drillholes(nP + nQ)
        X = np.array(X, dtype=np.float64)
        X[nP + FILL32_TWIN[1]] = X[FILL32_TWIN[0]]
        mu = np.zeros(4)
        mu[:cols] = X.sum(axis=0) / len(X)

        def transformed(Xs, cap):
            n = len(Xs)
            xs = np.zeros((4, cap))
            xs[:cols, :n] = Xs.T
            u, u2 = np.zeros(15 * cap), np.zeros(15 * cap)
            for v in (u, u2):
                assert ops.call("transform_k", xs.ravel(), cap, n, cap, self.kern, self.mode, mu, v) == OK
            assert np.array_equal(bits(u), bits(u2)), "two transforms of the same points differ"
            u = u.reshape(15, cap).copy()
            u[:, n:] = sentinel(1)[0]
            return u
        self.uP, self.uQ = transformed(X[:nP], capP), transformed(X[nP:], capQ)
        nt = len(self.terms)
        k, k3, ev = LD(self.bias), LD(self.bias), 0.0
        for t, (kind, p) in enumerate(self.terms):
            P, Q = self.uP[5 * t:5 * t + 5, :nP].astype(LD), self.uQ[5 * t:5 * t + 5, :nQ].astype(LD)
            d3 = sum((P[c][:, None] - Q[c][None, :]) ** 2 for c in (0, 1, 2))
            d2 = d3 + (P[4][:, None] - Q[4][None, :]) ** 2
            var2 = LD(np.float64(p[6 if kind == 0 else 2 if kind == 2 else 1]) ** 2)
            arg = (lambda d: LD(0.5) * LD(p[1]) * d) if kind == 2 else np.sqrt
            k, k3 = k + var2 * np.exp(-arg(d2)), k3 + var2 * np.exp(-arg(d3))
            ev = ev + (var2 * np.exp(-arg(d2))).astype(np.float64) * (FILL32_C0 + FILL32_C1 * arg(d2).astype(np.float64)) * U32
        self.k, self.k3 = k, k3
        self.bound = ev + (nt + 2) * U32 * np.abs(k).astype(np.float64)
        self.twin_exact = float(self.bias + sum(np.float64(p[6 if kd == 0 else 2 if kd == 2 else 1]) ** 2 for kd, p in self.terms))


def fill32_data(ops, comp):
    return memo(("fill32", ops.name, comp), lambda: Fill32Data(ops, comp))


def _fill_f32(ops, name, comp):
    d = fill32_data(ops, comp)
    nP, nQ, rows_p, cols_p = FILL32_NP, FILL32_NQ, FILL32_ROWS, FILL32_COLS
    ld = rows_p + 34
    uP, uQ = Mat(d.uP.ravel()), Mat(d.uQ.ravel())
    Cm = Mat(rng_for(name).standard_normal((rows_p, cols_p)), ld, F32)
    res = Result().rc("fill_f32", ops.call("fill_f32", uP, rows_p, nP, uQ, cols_p, nQ, rows_p, cols_p, d.kern, d.bias, d.mode, Cm, ld))
    ref, bound = np.zeros((rows_p, cols_p), dtype=LD), np.zeros((rows_p, cols_p))
    ref[:nP, :nQ], bound[:nP, :nQ] = d.k, d.bound
    res.add("C", Cm, ref, bound, True).add("uP", uP).add("uQ", uQ)
    pad = np.ones((rows_p, cols_p), dtype=bool)
    pad[:nP, :nQ] = False
    res.rc("rows >= nP or columns >= nQ that are not +0.0f", int(np.count_nonzero(bits(Cm.get()[pad].copy()))))
    i, j = FILL32_TWIN
    res.info["coincident pair: |k - (bias + sum var2)| / u32"] = abs(float(Cm.get()[i, j]) - d.twin_exact) / U32
    if comp == "expans d4":
        res.rc("the 4th column moves no element by 100 bounds", int(not (np.abs(d.k - d.k3).astype(np.float64) > 100 * d.bound).any()))
    if d.white:                          # Kern_White contributes nothing to a train x test block: the same bits without it
        C2 = Mat(Cm.was(), ld, F32)
        res.rc("fill_f32[white=0]", ops.call("fill_f32", uP, rows_p, nP, uQ, cols_p, nQ, rows_p, cols_p, d.kern_no_white, d.bias,
                                            d.mode, C2, ld))
        res.rc("elements Sigma_White changes", int(np.count_nonzero(bits(C2.full) != bits(Cm.full)))).add("C[white=0]", C2, free=True)
    return res


for _c in FILL32_COMPS:
    case("f32", f"fill_f32[{_c}]", ["gpak_dev_fill_f32", "gpak_dev_transform_k"], comp=_c)(_fill_f32)


def _fill_f32_refused(ops, name):
    d = fill32_data(ops, "expans+exp")
    rows_p, cols_p, ld = FILL32_ROWS, FILL32_COLS, FILL32_ROWS + 34
    uP, uQ = Mat(d.uP.ravel()), Mat(d.uQ.ravel())
    Cm = Mat(rng_for(name).standard_normal((rows_p, cols_p)), ld, F32)
    res = Result()
    good = dict(capP=rows_p, nP=FILL32_NP, capQ=cols_p, nQ=FILL32_NQ, rows_p=rows_p, cols_p=cols_p, kern=d.kern, ld=ld)
    four = list(d.kern)
    four[0] = 4
    for label, ch in (("rows_p=192", dict(rows_p=192)), ("cols_p=96", dict(cols_p=96)), ("capP below rows_p", dict(capP=rows_p - 2)),
                      ("nP above rows_p", dict(nP=rows_p + 1)), ("nQ above cols_p", dict(nQ=cols_p + 1)), ("ld odd", dict(ld=ld + 1)),
                      ("ld below rows_p", dict(ld=rows_p - 2)), ("four children", dict(kern=four))):
        a = dict(good, **ch)
        res.rc(label, ops.call("fill_f32", uP, a["capP"], a["nP"], uQ, a["capQ"], a["nQ"], a["rows_p"], a["cols_p"], a["kern"], d.bias,
                               d.mode, Cm, a["ld"]), EINVAL)
    return res.add("C", Cm).add("uP", uP).add("uQ", uQ)


case("f32", "fill_f32->EINVAL", ["gpak_dev_fill_f32"])(_fill_f32_refused)


# -- the conversions ------------------------------------------------------------------------------------
F32_EDGE_VALUES = (          # halfway cases between two floats, float denormals and below, signed zeros, the largest magnitudes
    1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -24 - 2.0 ** -53, -(1.0 + 2.0 ** -24),
    2.0 ** -126, 2.0 ** -127, 2.0 ** -140, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52),
    -(2.0 ** -150), 1e-40, 1e-46, -1e-46, 1e-300, 0.0, -0.0, 3e38, -3e38, 16777217.0)


def _convert_f32(ops, name):
    rng = rng_for(name)
    Np = 256
    ld, ldo = Np + 34, Np + 68
    L = rng.standard_normal((Np, Np))
    low = np.arange(Np)[:, None] >= np.arange(Np)[None, :]
    pos = np.argwhere(low)
    pick = pos[rng.permutation(len(pos))[:4 * len(F32_EDGE_VALUES)]]
    for q, (r, c) in enumerate(pick):
        L[r, c] = F32_EDGE_VALUES[q % len(F32_EDGE_VALUES)]
    for q, v in enumerate(F32_EDGE_VALUES[:Np]):         # and on the diagonal
        L[q + 3, q + 3] = v
    L[~low] = sentinel(1)[0]                                 # above the diagonal nothing is read
    Lm, out = Mat(L, ld), Mat(rng.standard_normal((Np, Np)), ldo, F32)
    res = Result().rc("lower_to_f32", ops.call("lower_to_f32", Lm, ld, Np, out, ldo))
    with np.errstate(all="ignore"):
        want = np.where(low, np.where(low, L, 0.0).astype(F32), F32(0))
    res.rc("lower_to_f32: elements whose bits are not np.float32(L) / +0.0f", int(np.count_nonzero(bits(out.get().copy()) != bits(want))))
    res.add("out", out, want.astype(LD), np.zeros((Np, Np)), True).add("L", Lm)
    for n in (1, 255, 256, 2 * TILE * TILE + 1):
        v = rng.standard_normal(n + 1)
        v[:min(n, len(F32_EDGE_VALUES))] = F32_EDGE_VALUES[:n]
        vin, vout = Mat(v), Mat(rng.standard_normal(n + 1), dtype=F32)
        res.rc(f"vec_to_f32[n={n}]", ops.call("vec_to_f32", vin, n, vout))
        with np.errstate(all="ignore"):
            w = v[:n].astype(F32)
        res.rc(f"vec_to_f32[n={n}]: elements whose bits are not np.float32(in)", int(np.count_nonzero(bits(vout.get()[:n, 0].copy()) != bits(w))))
        idx = np.arange(n + 1)[:, None] < n
        res.add(f"out[n={n}]", vout, np.concatenate([w, [0]]).astype(LD), np.zeros(n + 1), idx).add(f"in[n={n}]", vin)
    o2 = Mat(np.zeros((8, 8)), dtype=F32)
    res.rc("lower_to_f32[ldo below Np]", ops.call("lower_to_f32", Lm, ld, Np, o2, Np - 4), EINVAL)
    res.rc("lower_to_f32[Np=0]", ops.call("lower_to_f32", Lm, ld, 0, o2, ldo), EINVAL)
    res.rc("vec_to_f32[n=0]", ops.call("vec_to_f32", Lm, 0, o2), OK)
    return res.add("o2", o2)


case("f32", "lower_to_f32,vec_to_f32[Np=256]", ["gpak_dev_lower_to_f32", "gpak_dev_vec_to_f32"])(_convert_f32)


# -- the row sums of squares -----------------------------------------------------------------------------
def _rowsumsq_f32(ops, name, rows, cols, splits):
    rng = rng_for(name)
    ldv, part_ld = rows + 36, rows + 7
    V = Mat(rng.standard_normal((rows, cols)).astype(F32), ldv, F32)
    part = Mat(rng.standard_normal((part_ld, splits)), part_ld)
    res = Result().rc("rowsumsq_f32", ops.call("rowsumsq_f32", V, ldv, rows, cols, splits, part, part_ld))
    v2 = V.was().astype(LD) ** 2
    cps = (cols + splits - 1) // splits
    ref, bound = np.zeros((part_ld, splits), dtype=LD), np.zeros((part_ld, splits))
    for s in range(splits):
        c0, c1 = s * cps, min(cols, (s + 1) * cps)
        ref[:rows, s] = v2[:, c0:c1].sum(axis=1)
        bound[:rows, s] = (max(c1 - c0, 0) + 2) * U * ref[:rows, s].astype(np.float64)
    res.add("part", part, ref, bound, np.arange(part_ld)[:, None] < rows).add("V", V)
    tot, tref = part.get()[:rows].astype(LD).sum(axis=1), v2.sum(axis=1)
    err = np.abs(tot - tref).astype(np.float64)
    r = np.where(err == 0, 0.0, err / ((cols + 2) * U * tref.astype(np.float64)))
    r[~np.isfinite(err)] = np.inf
    res.info["sum over the splits: worst error / bound"] = float(r.max())
    return res.rc("rows whose sum over the splits is outside (cols + 2) u64 sum v^2", int(np.count_nonzero(~(r <= 1.0))))


for _rows in (1, 255, 256, 300):
    for _cols, _sp in ((640, 1), (640, 3), (640, 64), (5, 5), (639, 3)):
        case("f32", f"rowsumsq_f32[rows={_rows},cols={_cols},splits={_sp}]", ["gpak_dev_rowsumsq_f32"], rows=_rows, cols=_cols,
             splits=_sp)(_rowsumsq_f32)


def _rowsumsq_f32_refused(ops, name):
    rng = rng_for(name)
    V, part = Mat(rng.standard_normal((8, 5)), 12, F32), Mat(rng.standard_normal((9, 5)), 9)
    res = Result()
    for label, a in (("splits=0", (12, 8, 5, 0, 9)), ("splits above cols", (12, 8, 5, 6, 9)), ("rows=0", (12, 0, 5, 1, 9)),
                     ("ldv below rows", (7, 8, 5, 1, 9)), ("part_ld below rows", (12, 8, 5, 1, 7))):
        res.rc(label, ops.call("rowsumsq_f32", V, a[0], a[1], a[2], a[3], part, a[4]), EINVAL)
    return res.add("V", V).add("part", part)


case("f32", "rowsumsq_f32->EINVAL", ["gpak_dev_rowsumsq_f32"])(_rowsumsq_f32_refused)


# -- the ladder of the forward substitution -------------------------------------------------------------
LADDER_NP = 640
LADDER_LEVELS = ((128, 512), (128, 256), (128,), (128, 256, 1024))


class Ladder32:
    """The 640-row factor of the group `grad`, its fp32 image through gpak_dev_lower_to_f32 and its inverse blocks through
    gpak_dev_vec_to_f32 (the conversions feed the substitution as in the product), and Lf^-1 in long double."""

    def __init__(self, ops):
        f = factor_for(ops, LADDER_NP, 256)
        Np = LADDER_NP
        self.ld, self.ldLf = Np + 34, Np + 68
        low = np.arange(Np)[:, None] >= np.arange(Np)[None, :]
        Lm = Mat(np.where(low, f.L, sentinel(1)[0]), self.ld)
        Lf = Mat(rng_for("ladder Lf").standard_normal((Np, Np)), self.ldLf, F32)
        inv = np.concatenate([p.inv for p in f.cols])
        assert inv.size == Np // TILE * 2 * TILE * TILE
        invm, invf = Mat(inv), Mat(np.zeros(inv.size), dtype=F32)
        assert ops.call("lower_to_f32", Lm, self.ld, Np, Lf, self.ldLf) == OK and ops.call("vec_to_f32", invm, inv.size, invf) == OK
        assert Lf.guards_ok() and invf.guards_ok()
        self.Lf, self.invf = Lf.get().copy(), invf.get()[:, 0].copy()
        assert np.array_equal(bits(self.invf), bits(inv.astype(F32))) and not np.triu(self.Lf, 1).any()
        self.Li = tri_inv_ld(self.Lf.astype(np.float64))
        self.aLi = np.abs(self.Li).astype(np.float64)
        self._rhs = {}

    def rhs(self, mrows):
        """W standard_normal (two columns more than Np: not the call's), W Lf^-T in long double, |W| |Lf^-T|"""
        if mrows not in self._rhs:
            W = rng_for(f"ladder W[{mrows}]").standard_normal((mrows, LADDER_NP + 2)).astype(F32)
            W64 = W[:, :LADDER_NP].astype(np.float64)
            self._rhs[mrows] = (W, mm_ld(W64, self.Li), np.abs(W64) @ self.aLi.T)
        return self._rhs[mrows]


def ladder32(ops):
    return memo(("ladder32", ops.name), lambda: Ladder32(ops))


def _ladder_f32(ops, name, mrows, levels, build):
    d = ladder32(ops)
    Np, ldw = LADDER_NP, mrows + 36
    W0, ref, scale = d.rhs(mrows)
    Wt, Lf, invf = Mat(W0, ldw, F32), Mat(d.Lf, d.ldLf, F32), Mat(d.invf, dtype=F32)
    res = Result()
    ops.f32_build(F32_BUILDS[build])
    try:
        res.rc("fwd_subst_f32", ops.call("fwd_subst_f32", Wt, ldw, mrows, Np, Lf, d.ldLf, invf, list(levels), len(levels)))
    finally:
        ops.f32_build()
    num = memo(("ladder num", ops.name, mrows, levels, build), lambda: f32_ladder(
        W0[:, :Np].copy(), d.Lf, d.invf.reshape(Np // TILE, 2, TILE, TILE), levels, build in F32_WIDE, sequential=True))
    bound = subst_bound(res, "Wt", num, ref, scale)
    pad = lambda x: np.concatenate([x, np.zeros((mrows, 2), dtype=x.dtype)], axis=1)
    res.add("Wt", Wt, pad(ref), pad(bound), np.arange(Np + 2)[None, :] < Np)        # columns >= Np: untouched
    return res.add("Lf", Lf).add("invf", invf)


for _lv in LADDER_LEVELS:
    for _m in (128, 256):
        for _b in ("wide,rsd=4", "plain"):
            case("f32", f"fwd_subst_f32[levels={','.join(map(str, _lv))},mrows={_m},{_b}]",
                 ["gpak_dev_fwd_subst_f32", "gpak_dev_lower_to_f32", "gpak_dev_vec_to_f32"], mrows=_m, levels=_lv, build=_b)(_ladder_f32)


def _ladder_f32_default(ops, name):
    """nlevels = 0 is 128 / 512: the same bits"""
    d = ladder32(ops)
    Np, mrows = LADDER_NP, 128
    ldw = mrows + 36
    W0, _ref, _scale = d.rhs(mrows)
    res, outs = Result(), []
    for lv in ((), (128, 512)):
        Wt, Lf, invf = Mat(W0, ldw, F32), Mat(d.Lf, d.ldLf, F32), Mat(d.invf, dtype=F32)
        res.rc(f"fwd_subst_f32[nlevels={len(lv)}]", ops.call("fwd_subst_f32", Wt, ldw, mrows, Np, Lf, d.ldLf, invf, list(lv), len(lv)))
        res.add(f"Wt[nlevels={len(lv)}]", Wt, free=np.arange(Np + 2)[None, :] < Np)
        outs.append(Wt)
    return res.rc("elements that differ from levels = 128, 512", int(np.count_nonzero(bits(outs[0].full) != bits(outs[1].full))))


case("f32", "fwd_subst_f32[nlevels=0]", ["gpak_dev_fwd_subst_f32"])(_ladder_f32_default)


def _ladder_f32_refused(ops, name):
    d = ladder32(ops)
    Np, mrows = LADDER_NP, 128
    ldw = mrows + 36
    Wt, Lf, invf = Mat(d.rhs(mrows)[0], ldw, F32), Mat(d.Lf, d.ldLf, F32), Mat(d.invf, dtype=F32)
    res = Result()
    for label, lv, m, ld_ in (("levels do not ascend", (128, 512, 256), mrows, ldw), ("first level 256", (256, 512), mrows, ldw),
                              ("512 is no multiple of 384", (128, 384, 512), mrows, ldw), ("a level twice", (128, 128), mrows, ldw),
                              ("mrows=64", (128, 512), 64, ldw), ("ldw no multiple of 4", (128, 512), mrows, ldw + 2)):
        res.rc(label, ops.call("fwd_subst_f32", Wt, ld_, m, Np, Lf, d.ldLf, invf, list(lv), len(lv)), EINVAL)
    res.rc("Np=576", ops.call("fwd_subst_f32", Wt, ldw, mrows, 576, Lf, d.ldLf, invf, [128], 1), EINVAL)
    res.rc("Wt misaligned", ops.call("fwd_subst_f32", Off(Wt, 2), ldw, mrows, Np, Lf, d.ldLf, invf, [128], 1), EINVAL)
    return res.add("Wt", Wt).add("Lf", Lf).add("invf", invf)


case("f32", "fwd_subst_f32->EINVAL", ["gpak_dev_fwd_subst_f32"])(_ladder_f32_refused)


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
