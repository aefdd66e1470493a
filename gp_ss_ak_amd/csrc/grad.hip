// grad.hip -- the gradients of the negative log marginal likelihood on gfx950.
//
// gpak_grad / gpak_grad_hyb replace GP_utils::GradLL / dhyp / updateG / updateGlikelihood (GP_Utils.cpp:846-864,
// 1164-1284) with Kern_ExpAnisotropic::getGradients (Kernel.cpp:886-1263) and
// Kern_Bias::getGradients (:370-377), FORMULAS AS WRITTEN (this is not the
// true gradient -- the optimiser trajectory of the reference depends on it as it is).
// gpak_grad_exact is the derivative of nlZ itself; gpak_loo (leave-one-out cross-validation) is step 1 below alone and
// gpak_loo_grad the gradient of its pseudo-likelihood: the exact pass with another weight matrix; gpak_cv_groups_grad the
// same for the leave-group-out criterion of gpak_cv_groups (cv_groups.hip has its two kernels); gpak_dev_grad_*
// (further down) is the as-written gradient distributed over ranks by row blocks.
//
// Reference: Q = solve_chol(Lchol, diag(sW)) with N right-hand sides (2N^3 flops), ~15 N x N
// temporaries, six N x 3 * 3 x N GEMMs.  Here, for the Gaussian likelihood (d3lp = 0, so
// dfhat = dahat = 0, GP_Utils.cpp:414, 1210-1219), all three share
//   1. G = L^-T by blocked forward substitution on the identity, touching only the rows that
//      can be non-zero (N^3/3 flops, MFMA): grad_g_subst;
//   2. B^-1 = G G^T, lower tiles, k-loop started at the row tile (N^3/3 flops, MFMA);
//   3. ONE fused pass over the pairs i >= j that recomputes what it needs of K_ij from the coordinates and
//      accumulates NSUM sums the gradient entries are made of: gpak_grad_pairs_f64<Pass>, Pass = RefPass (as written)
//      or ExactPass.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/gpak_cv_folds.h"
#include "../../include/gpak_dev.h"
#include "../../include/gpak_dev_cv_kernels.h"
#include "gpak_internal.h"

#define PB 128
#define GT_ROWS 128
#define GT_COLS 64
#define NSUM 16  // sums of a pair pass (RefPass and ExactPass say what theirs are)
#define PARRG GPAK_PARR

// 1 on the diagonal of L^-T, 0 elsewhere, for the rows a rank owns: local row r of the slab (leading dimension ld,
// Np columns) is global row ((r / 128) * P + a) * 128 + r % 128; P = 1, a = 0: the whole matrix
__global__ void gpak_identity_f64(double *W, long ld, int Np, int P, int a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t tot = (size_t)Np * ld;
  if (i >= tot) return;
  const size_t c = i / ld, r = i - c * ld;
  const size_t grow = ((r / PB) * P + a) * PB + (r % PB);
  W[i] = (grow == c) ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------
// The pair pass over the lower triangle.  The skeleton owns the tiling (128 rows x 64 columns per workgroup, two
// rows per lane in registers, the column points in LDS), where a row of B^-1 lives, the i >= j filter,
// qw = q / sn2 - alpha_i alpha_j (dhyp, GP_Utils.cpp:1168: the W of the exact gradient) and the fixed-order
// reduction to part[block][NSUM].  A Pass supplies
//   Consts                what its body needs, by value;
//   Col, stage_col        what it keeps per column point in LDS beyond the transformed coordinates and alpha;
//   Row, stage_row        the same per row point, in registers;
//   pair                  the body: one pair (i, j), i >= j, accumulated into acc[NSUM].
// ---------------------------------------------------------------------------------------
struct PairIn {
  const double *U; int cap;          // transformed points (GPAK_PARR)
  const double *x0, *x1, *x2, *x3;   // raw input columns; x3 = nullptr for 3-column inputs
  const double *alpha, *Binv;
  long ld;                           // of Binv
  int N, nterms;
  double inv_sn2;
  // rowP > 0 (distributed gradient): this rank holds the B^-1 ROWS of the 128-row blocks g = t*rowP + rowA as a
  // compact (rows x Np) array whose 128-column groups are ordered by (g % rowP, g / rowP): see gpak_dev_grad_binv_rows
  int rowP, rowA, Tmax;
};

template <class Pass>
__global__ __launch_bounds__(256) void gpak_grad_pairs_f64(PairIn in, typename Pass::Consts pc, double *__restrict__ part) {
  const int rowP = in.rowP, N = in.N, nterms = in.nterms;
  const int row0 = (rowP ? blockIdx.x * rowP + in.rowA : blockIdx.x) * GT_ROWS, col0 = blockIdx.y * GT_COLS;
  const int bid = blockIdx.y * gridDim.x + blockIdx.x;
  __shared__ double cq[GPAK_MAX_TERMS][GPAK_PT][GT_COLS];  // transformed column points, per term
  __shared__ double cal[GT_COLS];                          // alpha of the column points
  __shared__ typename Pass::Col cp;
  __shared__ double red[4][NSUM];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double acc[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; k++) acc[k] = 0.0;
  if (row0 + GT_ROWS > col0) {  // tile touches the lower triangle
    if (t < GT_COLS) {
      const int j = col0 + t;
      const bool ok = j < N;
      for (int m = 0; m < nterms; m++)
#pragma unroll
        for (int c = 0; c < GPAK_PT; c++) cq[m][c][t] = ok ? PARRG(in.U, in.cap, m, c)[j] : 0.0;
      cal[t] = ok ? in.alpha[j] : 0.0;
      Pass::stage_col(cp, t, ok, j, in, pc);
    }
    __syncthreads();
    const int r = row0 + 2 * lane;
    // where row r / column j live in Binv
    const long rloc = rowP ? (long)blockIdx.x * GT_ROWS + 2 * lane : (long)r;
    long cgrp = 0;
    if (rowP) {
      const int g = col0 / PB;
      cgrp = ((long)(g % rowP) * in.Tmax + g / rowP) * PB - (long)g * PB;   // added to j: the permuted column
    }
    double pu[2][GPAK_MAX_TERMS][GPAK_PT], pal[2];
    typename Pass::Row pr[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int i = r + h;
      const bool ok = i < N;
#pragma unroll
      for (int m = 0; m < GPAK_MAX_TERMS; m++)
#pragma unroll
        for (int c = 0; c < GPAK_PT; c++) pu[h][m][c] = (ok && m < nterms) ? PARRG(in.U, in.cap, m, c)[i] : 0.0;
      pal[h] = ok ? in.alpha[i] : 0.0;
      Pass::stage_row(pr[h], ok, i, in, pc);
    }
    for (int c = 0; c < GT_COLS / 4; c++) {
      const int jl = w + 4 * c, j = col0 + jl;
      if (j >= N) continue;
      const double2 q2 = *reinterpret_cast<const double2 *>(in.Binv + rloc + (size_t)(j + cgrp) * in.ld);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int i = r + h;
        if (i >= N || i < j) continue;
        const double q = h ? q2.y : q2.x;
        const double qw = q * in.inv_sn2 - pal[h] * cal[jl];
        Pass::pair(acc, pu[h], cq, jl, pr[h], cp, q, qw, i == j, nterms, pc);
      }
    }
  }
  // block reduction (fixed order)
#pragma unroll
  for (int k = 0; k < NSUM; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (t < NSUM) part[(size_t)bid * NSUM + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

__global__ __launch_bounds__(256) void gpak_grad_reduce_f64(const double *__restrict__ part, int nblocks,
                                                            double *__restrict__ out) {
  __shared__ double sh[256];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += part[(size_t)b * NSUM + k];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[k] = sh[0];
}

// sum_i ((y_i - f_i)^2 / sn2 - 1)    (lp_dhyp, GP_Utils.cpp:858)
__global__ __launch_bounds__(1024) void gpak_lpdhyp_f64(int N, const double *__restrict__ y,
                                                         const double *__restrict__ f, double sn2, double *out) {
  __shared__ double sh[1024];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const double d = y[i] - f[i];
    s += (1.0 / sn2) * d * d - 1.0;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// Rot (Kernel.cpp:1399-1410) and, when D is given, its true derivatives D[a] = dRot / d angle_a,
// a = 0..2 = AngleX, AngleY, AngleZ
void gpak_rot_tables(const double *e, double R[3][3], double (*D)[3][3]) {
  const double al = e[0], be = e[2], te = e[4];
  const double ca = cos(al), sa = sin(al), cb = cos(be), sb = sin(be), ct = cos(te), st = sin(te);
  R[0][0] = ca * ct + sa * sb * st;
  R[0][1] = -sa * ct + ca * sb * st;
  R[0][2] = -cb * st;
  R[1][0] = sa * cb;
  R[1][1] = ca * cb;
  R[1][2] = sb;
  R[2][0] = ca * st - sa * sb * ct;
  R[2][1] = -sa * st - ca * sb * ct;
  R[2][2] = cb * ct;
  if (!D) return;
  D[0][0][0] = -sa * ct + ca * sb * st;  D[1][0][0] = sa * cb * st;    D[2][0][0] = -ca * st + sa * sb * ct;
  D[0][0][1] = -ca * ct - sa * sb * st;  D[1][0][1] = ca * cb * st;    D[2][0][1] = sa * st + ca * sb * ct;
  D[0][0][2] = 0.0;                      D[1][0][2] = sb * st;         D[2][0][2] = -cb * ct;
  D[0][1][0] = ca * cb;                  D[1][1][0] = -sa * sb;        D[2][1][0] = 0.0;
  D[0][1][1] = -sa * cb;                 D[1][1][1] = -ca * sb;        D[2][1][1] = 0.0;
  D[0][1][2] = 0.0;                      D[1][1][2] = cb;              D[2][1][2] = 0.0;
  D[0][2][0] = -sa * st - ca * sb * ct;  D[1][2][0] = -sa * cb * ct;   D[2][2][0] = ca * ct + sa * sb * st;
  D[0][2][1] = -ca * st + sa * sb * ct;  D[1][2][1] = -ca * cb * ct;   D[2][2][1] = -sa * ct + ca * sb * st;
  D[0][2][2] = 0.0;                      D[1][2][2] = -sb * ct;        D[2][2][2] = -cb * st;
}

// ---------------------------------------------------------------------------------------
// Steps 1 and 2.
// G = L^-T is upper triangular and its ROWS are independent right-hand sides of the blocked forward substitution on
// the identity (the test-major scheme of predict.hip), so rank a of P computes the rows of the 128-row blocks
// g = t*P + a into a compact slab (rows_a x Np, leading dimension lds) without communication; P = 1, a = 0 is the
// whole matrix.  Two levels like the Cholesky: 128-column steps inside a block column of nb columns, then one K = W
// update of the columns to the right; rows that enter the substitution later are still zero and are left out.
// ---------------------------------------------------------------------------------------
static int my_tiles(int Np, int P, int a) { const int T = Np / PB; return T > a ? (T - a + P - 1) / P : 0; }

// block column b of L, rows from its diagonal block down (leading dimension ldp), and its inverted 128-blocks
struct LBlockCol { const double *panel; long ldp; const double *inv; };

template <class Where>   // Where: int b -> LBlockCol
static void grad_g_subst(hipStream_t st, int Np, int nb, int P, int a, Where where, double *slab, long lds) {
  const int Ta = my_tiles(Np, P, a);
  if (Ta == 0) return;
  const size_t tot = (size_t)Np * lds;
  hipLaunchKernelGGL(gpak_identity_f64, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, slab, lds, Np, P, a);
  auto tiles_upto = [&](int gblock) { return gblock >= a ? std::min(Ta, (gblock - a) / P + 1) : 0; };   // g <= gblock
  for (int b = 0, J = 0; J < Np; b++, J += nb) {
    const int W = std::min(nb, Np - J);
    const LBlockCol L = where(b);
    for (int j0 = J; j0 < J + W; j0 += PB) {
      const int mt = tiles_upto(j0 / PB);   // rows below are still zero in L^-T
      if (mt == 0) continue;
      const double *inv = L.inv + (size_t)((j0 - J) / PB) * 2 * PB * PB;
      double *Wj = slab + (size_t)j0 * lds;
      gpak_launch_gemm_nt(st, mt, 1, PB, 1.0, Wj, lds, inv, PB, 0.0, Wj, lds, 0, 0, false, false);
      const int nin = (J + W - j0 - PB) / PB;
      if (nin > 0)
        gpak_launch_gemm_nt(st, mt, nin, PB, -1.0, Wj, lds, L.panel + (j0 + PB - J) + (size_t)(j0 - J) * L.ldp, L.ldp, 1.0,
                            slab + (size_t)(j0 + PB) * lds, lds, 0, 0, false, false);
    }
    const int nrest = (Np - J - W) / PB, mt2 = tiles_upto((J + W) / PB - 1);
    if (nrest > 0 && mt2 > 0)
      gpak_launch_gemm_nt(st, mt2, nrest, W, -1.0, slab + (size_t)J * lds, lds, L.panel + W, L.ldp, 1.0,
                          slab + (size_t)(J + W) * lds, lds, 0, 0, false, false);
  }
}

// single GPU: allocates the two N x N workspaces on first use, records ev[7] (the start of grad_ms) and leaves B^-1
// (lower tiles) in ctx->dBinv
static int grad_binv(gpak_ctx *ctx) {
  hipStream_t st = ctx->stream;
  const int Np = ctx->Np;
  const long ld = ctx->ld;
  if (!ctx->dG.reserve((size_t)ld * Np) || !ctx->dBinv.reserve((size_t)ld * Np)) {
    ctx->err = "device allocation failed for the gradient workspaces (2 N x N matrices)";
    ctx->dG.release(); ctx->dBinv.release();   // never one without the other: dG != NULL says that both exist
    ctx->dGpart.release(); ctx->dLoo.release();
    return GPAK_ENOMEM;
  }
  GPAK_HIP(hipEventRecord(ctx->ev[7], st));
  // 1. G = L^-T: block columns of 512 of the factor in dM, their inverted diagonal blocks in dInv
  const int GNB = 512;
  double *G = ctx->dG;
  grad_g_subst(st, Np, GNB, 1, 0, [&](int b) {
    const size_t J = (size_t)b * GNB;
    return LBlockCol{ctx->dM + J + J * ld, ld, ctx->dInv + J / PB * 2 * PB * PB};
  }, G, ld);
  // 2. B^-1 = G G^T (lower tiles); G[i,k] = 0 for k < i, so the k-loop starts at the row tile
  gpak_launch_gemm_nt(st, Np / PB, Np / PB, Np, 1.0, G, ld, G, ld, 0.0, ctx->dBinv, ld, 0, 0, true, true, true);
  return GPAK_OK;
}

// per-workgroup partial sums of a pair pass: at least `elems` doubles in ctx->dGpart
static int grad_partials(gpak_ctx *ctx, size_t elems) {
  if (ctx->dGpart.reserve(elems)) return GPAK_OK;
  ctx->err = "device allocation failed for gradient partial sums";
  return GPAK_ENOMEM;
}

// what gpak_cv_groups (cv_groups.hip) shares with the passes of this file: the scratch buffer, and G = L^-T of the
// context's factor as ONE Np x Np matrix (P = 1) in a buffer of the caller's
int gpak_grad_scratch(gpak_ctx *ctx, size_t elems) { return grad_partials(ctx, elems); }
// the L^-T workspace of gpak_loo (a slab) and gpak_cv_groups (the whole matrix) when the gradient has not allocated dG
bool gpak_loo_workspace(gpak_ctx *ctx, size_t elems) {
  if (ctx->dLoo.reserve(elems)) return true;
  (void)hipGetLastError();
  return false;
}

void gpak_grad_g_full(gpak_ctx *ctx, double *G, long ldg) {
  const int GNB = 512;
  const long ld = ctx->ld;
  grad_g_subst(ctx->stream, ctx->Np, GNB, 1, 0, [&](int b) {
    const size_t J = (size_t)b * GNB;
    return LBlockCol{ctx->dM + J + J * ld, ld, ctx->dInv + J / PB * 2 * PB * PB};
  }, G, ldg);
}
// the same driver on any lower factor held as ONE matrix: T = R^-T (n x n, n a multiple of 128, leading dimension ldt)
// of the factor R at M (leading dimension ld) whose inverted 128-blocks are at inv (gpak_cv_folds: a fold's own S)
void gpak_grad_g_of(hipStream_t st, int n, const double *M, long ld, const double *inv, double *T, long ldt) {
  const int GNB = 512;
  grad_g_subst(st, n, GNB, 1, 0, [&](int b) {
    const size_t J = (size_t)b * GNB;
    return LBlockCol{M + J + J * ld, ld, inv + J / PB * 2 * PB * PB};
  }, T, ldt);
}

// ---------------------------------------------------------------------------------------
// The as-written pass.  part[block][NSUM]:
//   [0..5] sum Rm * Di2^(p)   [6] sum QW * exp(-sqrt(D_expans))   [7] sum Q * K   [8] trace(QW)
//   [9+2t], [10+2t]  the two sums of stationary term t when it is an Exp or RBF child; those
//   children work on GP_utils' member D2 = the SUM of the children's D2 (Kernel.cpp:151, 491-540, 644-693)
//   [15] sum exp(-sqrt(D_expans)) * (x4_i - x4_j)^2 for 4-column inputs (Kernel.cpp:1246-1255: the weight is
//        KD2, not R -- RColon still holds KD2 from the Sigma block, reproduced as written)
// ---------------------------------------------------------------------------------------
struct GradConsts {
  double M[6][6];   // S % S_p, symmetric 3x3 stored as {00,01,02,11,12,22}, p = 0..5
  double m2[6][3];  // 2 * column sums of M_p : a_i^(p) = sum_k x_ik^2 m2[p][k]
  double var2, bias;
  int mode;
  int te;           // index of the ExpAns term (-1: none)
  int kinds[GPAK_MAX_TERMS];
};

// S, S_alpha.. as written at Kernel.cpp:955-1166 (the (0,0) z-term of the angle derivatives lacks
// its factor 2, :1003-1011) and M_p = S % S_p
static void build_grad_consts(const double *e, GradConsts &gc) {
  const double iw[3] = {e[1], e[3], e[5]};
  double R[3][3], D[3][3][3];
  gpak_rot_tables(e, R, D);
  double S[3][3], Sp[6][3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += iw[k] * R[r][k] * R[c][k];
      S[r][c] = s;
      for (int a = 0; a < 3; a++) {
        double t = 0.0;
        for (int k = 0; k < 3; k++) {
          double term = iw[k] * (D[a][r][k] * R[c][k] + R[r][k] * D[a][c][k]);
          if (r == 0 && c == 0 && k == 2) term *= 0.5;
          t += term;
        }
        Sp[2 * a][r][c] = t;
        Sp[2 * a + 1][r][c] = R[r][a] * R[c][a];
      }
    }
  const int ir[6] = {0, 0, 0, 1, 1, 2}, ic[6] = {0, 1, 2, 1, 2, 2};
  for (int p = 0; p < 6; p++) {
    double M[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) M[r][c] = S[r][c] * Sp[p][r][c];
    for (int q = 0; q < 6; q++) gc.M[p][q] = M[ir[q]][ic[q]];
    for (int k = 0; k < 3; k++) gc.m2[p][k] = 2.0 * (M[k][0] + M[k][1] + M[k][2]);
  }
}

// the gradient entries from the NSUM pair sums + the lp_dhyp sum (red[NSUM]); children in order, bias, sn2
void gpak_grad_assemble(const KernParams &kp, const int *kinds, const double *expans, int d, int N, double sn2,
                        const double *red, double *g) {
  int go = 0;
  for (int t = 0; t < kp.nterms; t++) {
    const KernTerm &T = kp.term[t];
    const double A = red[9 + 2 * t], B = red[10 + 2 * t];
    if (kinds[t] == GPAK_KERN_EXPANS) {
      for (int p = 0; p < 6; p++) g[go + p] = red[p];            // Kernel.cpp:1195-1233
      g[go + 6] = 2.0 * red[6] * expans[6];                      // :1241-1242
      // :1246-1257: 0 for 3-D inputs; with a rock-type column -2 * sum(KD2 % Di2_R) / N, Di2_R = 2 dx4^2
      g[go + 7] = d == 4 ? -4.0 * red[15] / (double)N : 0.0;
      go += 8;
    } else if (kinds[t] == GPAK_KERN_EXP) {                      // Kernel.cpp:671-690
      g[go] = T.var2 * A;
      g[go + 1] = B * sqrt(T.var2);
      go += 2;
    } else {                                                     // Kernel.cpp:512-538
      g[go] = T.var2 * (T.iw / 2) * A;                           // g1/2 = -(sum R . D2), R = var2 QW KD2 (-iw/2)
      g[go + 1] = -0.25 * T.var2 * A;                            // g2/2
      g[go + 2] = T.var2 * B;                                    // g3/2 = sigma^2 sum QW . KD2
      go += 3;
    }
  }
  g[go++] = red[8];                                              // Kern_Bias::getGradients: trace(QW)
  const double sum_dW = 0.5 * red[7];                            // dW = 0.5 * sum(Q % K, 1)
  g[go] = -1.0 * sum_dW * (2.0 / sn2) - red[NSUM];               // GP_Utils.cpp:1226
}

struct RefPass {
  struct Consts { KernParams kp; GradConsts gc; };
  struct Col {
    double x3[GT_COLS];        // raw 4th column (0 for 3-D)
    double m[6][3][GT_COLS];   // M_p x_j
    double a[6][GT_COLS];      // a_j^(p)
  };
  struct Row { double x[3], a[6], x3; };

  static __device__ __forceinline__ void stage_col(Col &s, int t, bool ok, int j, const PairIn &in, const Consts &k) {
    s.x3[t] = (ok && in.x3) ? in.x3[j] : 0.0;
    const double a = ok ? in.x0[j] : 0.0, b = ok ? in.x1[j] : 0.0, c = ok ? in.x2[j] : 0.0;
#pragma unroll
    for (int p = 0; p < 6; p++) {
      const double *M = k.gc.M[p];
      s.m[p][0][t] = M[0] * a + M[1] * b + M[2] * c;
      s.m[p][1][t] = M[1] * a + M[3] * b + M[4] * c;
      s.m[p][2][t] = M[2] * a + M[4] * b + M[5] * c;
      s.a[p][t] = a * a * k.gc.m2[p][0] + b * b * k.gc.m2[p][1] + c * c * k.gc.m2[p][2];
    }
  }
  static __device__ __forceinline__ void stage_row(Row &p, bool ok, int i, const PairIn &in, const Consts &k) {
    p.x3 = (ok && in.x3) ? in.x3[i] : 0.0;
    p.x[0] = ok ? in.x0[i] : 0.0; p.x[1] = ok ? in.x1[i] : 0.0; p.x[2] = ok ? in.x2[i] : 0.0;
#pragma unroll
    for (int q = 0; q < 6; q++)
      p.a[q] = p.x[0] * p.x[0] * k.gc.m2[q][0] + p.x[1] * p.x[1] * k.gc.m2[q][1] + p.x[2] * p.x[2] * k.gc.m2[q][2];
  }
  static __device__ __forceinline__ void pair(double (&acc)[NSUM], const double (&pu)[GPAK_MAX_TERMS][GPAK_PT],
                                              const double (&cq)[GPAK_MAX_TERMS][GPAK_PT][GT_COLS], int jl, const Row &pr,
                                              const Col &cp, double q, double qw, bool diag, int nterms, const Consts &k) {
    const KernParams &kp = k.kp;
    const GradConsts &gc = k.gc;
    const int te = gc.te;
    const double wgt = diag ? 1.0 : 2.0;  // every summand is symmetric in (i, j)
    double d2m[GPAK_MAX_TERMS], d2s = 0.0, kfull = gc.bias;
#pragma unroll
    for (int m = 0; m < GPAK_MAX_TERMS; m++) {
      if (m >= nterms) break;
      const double d2 = gpak_d2(pu[m][0], pu[m][1], pu[m][2], pu[m][3], pu[m][4], cq[m][0][jl], cq[m][1][jl], cq[m][2][jl],
                                cq[m][3][jl], cq[m][4][jl], gc.mode);
      d2m[m] = d2;
      d2s += d2;
      kfull += gpak_profile(d2, kp.term[m]);
    }
    acc[7] = fma(wgt * q, kfull, acc[7]);                       // sum(Q % K), GP_Utils.cpp:1206
    if (diag) acc[8] += qw;                                     // trace(QW), Kernel.cpp:370-377
    if (te >= 0) {
      const double sd = gpak_sqrt_nonneg(d2m[te]);              // Kernel.cpp:1178
      const double ek = gpak_exp_nonpos(-sd);                   // KD2, :1176
      const double dk = (sd == 0.0 || diag) ? 0.0 : ek * (-0.5 / sd);  // :1179-1184
      const double rm = gc.var2 * qw * dk;                      // R = Qs % dk, :927, :1185
#pragma unroll
      for (int p = 0; p < 6; p++) {
        const double xmx = pr.x[0] * cp.m[p][0][jl] + pr.x[1] * cp.m[p][1][jl] + pr.x[2] * cp.m[p][2][jl];
        const double di2 = pr.a[p] + cp.a[p][jl] - 4.0 * xmx;   // Di2, :1192-1194
        acc[p] = fma(wgt * rm, di2, acc[p]);
      }
      acc[6] = fma(wgt * qw, ek, acc[6]);                       // :1239-1241
      const double dx4 = pr.x3 - cp.x3[jl];
      acc[15] = fma(wgt * ek, dx4 * dx4, acc[15]);              // :1246-1253 (Di2_R = 2 dx4^2)
    }
#pragma unroll
    for (int m = 0; m < GPAK_MAX_TERMS; m++) {
      if (m >= nterms) break;
      if (gc.kinds[m] == GPAK_KERN_EXP) {                       // Kernel.cpp:644-693 on the summed D2
        const double sd = gpak_sqrt_nonneg(d2s), kd = gpak_exp_nonpos(-sd);
        const double dk = (sd == 0.0 || diag) ? 0.0 : kd * (-0.5 / sd);
        acc[9 + 2 * m] = fma(wgt * qw * dk, d2s, acc[9 + 2 * m]);
        acc[10 + 2 * m] = fma(wgt * qw * kd, kd, acc[10 + 2 * m]);
      } else if (gc.kinds[m] == GPAK_KERN_RBF) {                // Kernel.cpp:491-540 on the summed D2
        const double kd = gpak_exp_nonpos(-0.5 * kp.term[m].iw * d2s);
        acc[9 + 2 * m] = fma(wgt * qw * kd, d2s, acc[9 + 2 * m]);
        acc[10 + 2 * m] = fma(wgt * qw, kd, acc[10 + 2 * m]);
      }
    }
  }

  // host side of gpak_grad / gpak_grad_hyb
  static constexpr const char *entry = "gpak_grad";
  // Kern_White has no getGradients upstream (Kernel.h:257-283: the base method calls itself)
  static constexpr const char *white = "compositions with a White child have no gradient in the reference either";
  static constexpr bool lp_dhyp = true;   // red[NSUM] = the lp_dhyp sum
  static Consts consts(const KernParams &kp, const int *kinds, int te, const double *expans, double bias, int mode) {
    Consts k;
    memset(&k, 0, sizeof(k));
    k.kp = kp;
    if (te >= 0) build_grad_consts(expans, k.gc);
    k.gc.var2 = te >= 0 ? kp.term[te].var2 : 0.0;
    k.gc.bias = bias; k.gc.mode = mode; k.gc.te = te;
    for (int t = 0; t < GPAK_MAX_TERMS; t++) k.gc.kinds[t] = t < kp.nterms ? kinds[t] : -1;
    return k;
  }
  static void assemble(const gpak_ctx *ctx, const double *red, double *g) {
    gpak_grad_assemble(ctx->kp, ctx->kinds, ctx->expans, ctx->d, ctx->N, ctx->sn2, red, g);
  }
};

// ---------------------------------------------------------------------------------------
// The EXACT gradient of nlZ (gpak_grad_exact): d nlZ / d theta = 1/2 sum_ij W_ij dK_ij / d theta with
// W = (K + sn2 I)^-1 - alpha alpha^T, the skeleton's `qw`.  The pass accumulates sums that do not depend on which
// parameter is differentiated, and the host contracts them with the 3 x 3 matrices dA / d theta
// (gpak_grad_exact_assemble).  part[block][NSUM], sums over i >= j with weight 2 off the diagonal:
//   [0] sum W   [1] trace W   [2+t] sum W e_t   [5+t] sum W e'_t d2_t for an Exp (e' = dk) or RBF (e' = e) child, on the
//   child's OWN d2   [8..13] sum W dk D_a D_b, (a, b) = 00 01 02 11 12 22, D = x_i - x_j on the raw columns, ExpAns term
//   [14] sum W dk D_4^2 (raw 4th column)
// e_t = exp(-sqrt(d2_t)) or exp(-iw d2_t / 2), dk = -e / (2 sqrt(d2)) and 0 where d2 = 0 or i == j; d2_t from the
// transformed points by differences whatever dist_mode is (a gradient has no use for the expansion's cancellation noise)
// ---------------------------------------------------------------------------------------
// the gradient entries from the NSUM sums; pars[t] = the raw parameters of stationary term t in the reference's order
// (ExpAns 8, Exp {hyp, Sigma}, RBF {hyp, iw, Sigma}); layout of g as gpak_grad_hyb: children in order, bias, sn2
static void gpak_grad_exact_assemble(int nterms, const int *kinds, const double (*pars)[8], const double *red, double *g) {
  int go = 0;
  for (int t = 0; t < nterms; t++) {
    const double *p = pars[t];
    const double SWe = red[2 + t], SWd = red[5 + t];
    if (kinds[t] == GPAK_KERN_EXPANS) {
      // D = Delta^T A^2 Delta + (a33 Delta_4)^2, A = Rot diag(lam) Rot^T:  dD/dp = Delta^T (A A_p + A_p A) Delta
      const double var2 = p[6] * p[6], lam[3] = {p[1], p[3], p[5]};
      double R[3][3], D[3][3][3], A[3][3], T[3][3];
      gpak_rot_tables(p, R, D);
      T[0][0] = red[8]; T[0][1] = T[1][0] = red[9]; T[0][2] = T[2][0] = red[10];
      T[1][1] = red[11]; T[1][2] = T[2][1] = red[12]; T[2][2] = red[13];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
          A[r][c] = 0.0;
          for (int k = 0; k < 3; k++) A[r][c] += lam[k] * R[r][k] * R[c][k];
        }
      for (int q = 0; q < 6; q++) {
        const int a = q / 2;
        double Ap[3][3];
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) {
            if (q & 1) { Ap[r][c] = R[r][a] * R[c][a]; continue; }       // width lam_a: r_a r_a^T
            Ap[r][c] = 0.0;                                              // angle a: Rot_a Lam Rot^T + Rot Lam Rot_a^T
            for (int k = 0; k < 3; k++) Ap[r][c] += lam[k] * (D[a][r][k] * R[c][k] + R[r][k] * D[a][c][k]);
          }
        double s = 0.0;
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) {
            double m = 0.0;
            for (int k = 0; k < 3; k++) m += A[r][k] * Ap[k][c] + Ap[r][k] * A[k][c];
            s += m * T[r][c];
          }
        g[go + q] = 0.5 * var2 * s;
      }
      g[go + 6] = p[6] * SWe;
      g[go + 7] = p[7] * var2 * red[14];   // 0 for 3-column inputs: every Delta_4 is 0
      go += 8;
    } else if (kinds[t] == GPAK_KERN_EXP) {   // k = Sigma^2 exp(-sqrt(d2)), d2 = |Delta|^2 / hyp^2
      g[go] = -(p[1] * p[1] / p[0]) * SWd;
      g[go + 1] = p[1] * SWe;
      go += 2;
    } else {                                  // k = Sigma^2 exp(-iw d2 / 2), d2 = |Delta|^2 / hyp^2
      const double var2 = p[2] * p[2];
      g[go] = var2 * p[1] / (2.0 * p[0]) * SWd;
      g[go + 1] = -0.25 * var2 * SWd;
      g[go + 2] = p[2] * SWe;
      go += 3;
    }
  }
  g[go++] = 0.5 * red[0];   // K gets Sigma_Bias on every entry
  g[go] = 0.5 * red[1];     // and sn2 on the diagonal
}

struct ExactPass {
  struct Consts {
    double iw[GPAK_MAX_TERMS];
    int profile[GPAK_MAX_TERMS];
    int te;   // index of the ExpAns term (-1: none)
  };
  struct Col { double x[4][GT_COLS]; };   // raw columns (the 4th 0 for 3-D)
  struct Row { double x[4]; };

  static __device__ __forceinline__ void stage_col(Col &s, int t, bool ok, int j, const PairIn &in, const Consts &) {
    s.x[0][t] = ok ? in.x0[j] : 0.0; s.x[1][t] = ok ? in.x1[j] : 0.0; s.x[2][t] = ok ? in.x2[j] : 0.0;
    s.x[3][t] = (ok && in.x3) ? in.x3[j] : 0.0;
  }
  static __device__ __forceinline__ void stage_row(Row &p, bool ok, int i, const PairIn &in, const Consts &) {
    p.x[0] = ok ? in.x0[i] : 0.0; p.x[1] = ok ? in.x1[i] : 0.0; p.x[2] = ok ? in.x2[i] : 0.0;
    p.x[3] = (ok && in.x3) ? in.x3[i] : 0.0;
  }
  static __device__ __forceinline__ void pair(double (&acc)[NSUM], const double (&pu)[GPAK_MAX_TERMS][GPAK_PT],
                                              const double (&cq)[GPAK_MAX_TERMS][GPAK_PT][GT_COLS], int jl, const Row &pr,
                                              const Col &cp, double, double qw, bool diag, int nterms, const Consts &xc) {
    const int te = xc.te;
    const double wq = diag ? qw : 2.0 * qw;  // every summand is symmetric in (i, j)
    acc[0] += wq;
    if (diag) acc[1] += qw;
#pragma unroll
    for (int m = 0; m < GPAK_MAX_TERMS; m++) {
      if (m >= nterms) break;
      const double a = pu[m][0] - cq[m][0][jl], b = pu[m][1] - cq[m][1][jl], cc = pu[m][2] - cq[m][2][jl];
      const double e4 = pu[m][4] - cq[m][4][jl];
      const double d2 = a * a + b * b + cc * cc + e4 * e4;
      if (xc.profile[m] == GPAK_PROFILE_RBF) {
        const double we = wq * gpak_exp_nonpos(-0.5 * xc.iw[m] * d2);
        acc[2 + m] += we;
        acc[5 + m] = fma(we, d2, acc[5 + m]);
      } else {
        const double sd = gpak_sqrt_nonneg(d2);
        const double ek = gpak_exp_nonpos(-sd);
        const double wdk = (sd == 0.0 || diag) ? 0.0 : wq * ek * (-0.5 / sd);
        acc[2 + m] = fma(wq, ek, acc[2 + m]);
        if (m == te) {
          const double da = pr.x[0] - cp.x[0][jl], db = pr.x[1] - cp.x[1][jl], dc = pr.x[2] - cp.x[2][jl];
          const double dr = pr.x[3] - cp.x[3][jl];
          const double wa = wdk * da, wb = wdk * db;
          acc[8] = fma(wa, da, acc[8]);
          acc[9] = fma(wa, db, acc[9]);
          acc[10] = fma(wa, dc, acc[10]);
          acc[11] = fma(wb, db, acc[11]);
          acc[12] = fma(wb, dc, acc[12]);
          acc[13] = fma(wdk * dc, dc, acc[13]);
          acc[14] = fma(wdk * dr, dr, acc[14]);
        } else {
          acc[5 + m] = fma(wdk, d2, acc[5 + m]);
        }
      }
    }
  }

  // host side of gpak_grad_exact
  static constexpr const char *entry = "gpak_grad_exact";
  // a context cannot tell a White child of value 0 from none, so the entry would come and go with the value
  static constexpr const char *white = "compositions with a White child are not built";
  static constexpr bool lp_dhyp = false;
  static Consts consts(const KernParams &kp, const int *, int te, const double *, double, int) {
    Consts xc;
    memset(&xc, 0, sizeof(xc));
    xc.te = te;
    for (int t = 0; t < kp.nterms; t++) { xc.iw[t] = kp.term[t].iw; xc.profile[t] = kp.term[t].profile; }
    return xc;
  }
  static void assemble(const gpak_ctx *ctx, const double *red, double *g) {
    gpak_grad_exact_assemble(ctx->kp.nterms, ctx->kinds, ctx->tpars, red, g);
  }
};

// One pair pass on caller-owned buffers and the reduction of its block partials to out[NSUM]: what every entry point
// launches.  P == 0: B^-1 is Np x Np with leading dimension ld (the single-GPU layout, rowP = 0); P >= 1: rank a's row
// blocks as gpak_dev_grad_binv_rows leaves them (ld is then rows_a, whatever is passed); a rank without tiles launches
// nothing.  x_soa: the raw columns with stride xs, the 4th read only when d == 4.  te: index of the ExpAns child (-1: none),
// expans: its eight parameters.
template <class Pass>
static void pair_sums(hipStream_t st, const KernParams &kp, const int *kinds, int te, const double *expans, double bias,
                      int mode, int d, const double *u, int cap, const double *x_soa, int xs, int n, int Np,
                      const double *alpha, const double *binv, long ld, int P, int a, double sn2, double *part, double *out) {
  const int Ta = P ? my_tiles(Np, P, a) : Np / GT_ROWS;
  if (Ta == 0) return;
  const typename Pass::Consts pc = Pass::consts(kp, kinds, te, expans, bias, mode);
  const PairIn in = {u, cap, x_soa, x_soa + xs, x_soa + 2 * (size_t)xs, d == 4 ? x_soa + 3 * (size_t)xs : nullptr,
                     alpha, binv, P ? (long)Ta * PB : ld, n, kp.nterms, 1.0 / sn2, P, P ? a : 0, P ? my_tiles(Np, P, 0) : 0};
  const dim3 grid(Ta, Np / GT_COLS);
  hipLaunchKernelGGL(gpak_grad_pairs_f64<Pass>, grid, dim3(256), 0, st, in, pc, part);
  hipLaunchKernelGGL(gpak_grad_reduce_f64, dim3(NSUM), dim3(256), 0, st, part, (int)(grid.x * grid.y), out);
}

// what every single-GPU gradient checks first: ng against the composition's layout (children in order, 8 / 2 / 3
// entries, then bias and sn2), at most one ExpAns child (*te: its index, -1: none), no White child
static int grad_layout(gpak_ctx *ctx, const char *entry, const char *white, int ng, int *te) {
  const std::string who = std::string(entry) + ": ";
  int need = 2;
  *te = -1;
  for (int t = 0; t < ctx->kp.nterms; t++) {
    need += ctx->kinds[t] == GPAK_KERN_EXPANS ? 8 : ctx->kinds[t] == GPAK_KERN_EXP ? 2 : 3;
    if (ctx->kinds[t] == GPAK_KERN_EXPANS) {
      if (*te >= 0) { ctx->err = who + "at most one ExpAns child"; return GPAK_ENOTIMPL; }
      *te = t;
    }
  }
  if (ng != need) { ctx->err = who + "gradient vector has the wrong length"; return GPAK_EINVAL; }
  if (ctx->kp.white != 0.0) { ctx->err = who + white; return GPAK_ENOTIMPL; }
  return GPAK_OK;
}

// the single-GPU entry points: kinds of the current composition (set by gpak_set_params / gpak_set_kernel)
template <class Pass>
static int grad_single(gpak_ctx *ctx, double *g, int ng) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np;
  int te = -1;
  int rc = grad_layout(ctx, Pass::entry, Pass::white, ng, &te);
  if (rc) return rc;
  rc = grad_binv(ctx);
  if (rc) return rc;
  // 3. fused pair pass
  rc = grad_partials(ctx, (size_t)(Np / GT_ROWS) * (Np / GT_COLS) * NSUM);
  if (rc) return rc;
  rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  pair_sums<Pass>(st, ctx->kp, ctx->kinds, te, ctx->expans, ctx->bias, ctx->dist_mode, ctx->d, ctx->U.base, ctx->U.cap, ctx->dX,
                  Np, N, Np, ctx->dAlpha, ctx->dBinv, ctx->ld, 0, 0, ctx->sn2, ctx->dGpart, ctx->dRed + 8);
  if (Pass::lp_dhyp)
    hipLaunchKernelGGL(gpak_lpdhyp_f64, dim3(1), dim3(1024), 0, st, N, ctx->dy, ctx->dF, ctx->sn2, ctx->dRed + 8 + NSUM);
  double red[NSUM + 1];
  GPAK_HIP(hipMemcpyAsync(red, ctx->dRed + 8, sizeof(double) * (NSUM + Pass::lp_dhyp), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[3], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[3]));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[3]));
  ctx->times.grad_ms = ms;
  Pass::assemble(ctx, red, g);
  return GPAK_OK;
}
int gpak_grad_impl(gpak_ctx *ctx, double *g, int ng) { return grad_single<RefPass>(ctx, g, ng); }
int gpak_grad_exact_impl(gpak_ctx *ctx, double *g, int ng) { return grad_single<ExactPass>(ctx, g, ng); }

// ---------------------------------------------------------------------------------------
// Leave-one-out cross-validation (gpak_loo) from step 1 alone.  With Ky = K + sn2 I = sn2 B and B = L L^T,
//   d_i = [B^-1]_ii = sum_{k >= i} G_ik^2,   var_i = sn2 / d_i,   mean_i = y_i - alpha_i var_i
// (Rasmussen & Williams eq. 5.12).  G is formed by grad_g_subst in P passes; pass a holds the 128-row blocks
// g = t*P + a in a compact slab, so N^2 doubles are never needed at once.  Per pass:
//   gpak_loo_sumsq_f64    one partial per (row, 512-column chunk) of the slab;
//   gpak_loo_rowsum_f64   d_i = the row's partials added in ascending chunk order.
// The chunks are cut at ABSOLUTE column indices and the columns inside a chunk are dealt to the four waves by their
// absolute index, so the order in which the squares of row i are added depends on i alone: d_i is the same number
// whatever P, a or the leading dimension of the slab.  Then once, over the N rows: gpak_loo_finish_f64.
// ---------------------------------------------------------------------------------------
#define LOO_CHUNK 512   // columns per partial sum (a multiple of 128)
#define LOO_DEFAULT_ROWS 16384

// part[c * rows + r] = sum of G[r, k]^2 over the columns k >= 128 g of chunk c, for local row r of row block
// g = (r / 128) * P + a.  Lanes run along the rows (the slab is column-major: one 16-byte load per lane, 1 KiB per
// wave and column), wave w takes the columns k = w (mod 4).  Chunks left of the diagonal block are structural zeros:
// neither read nor written (gpak_loo_rowsum_f64 starts at the diagonal's chunk).
__global__ __launch_bounds__(256) void gpak_loo_sumsq_f64(const double *__restrict__ slab, long lds, int Np, int P, int a,
                                                          long rows, double *__restrict__ part) {
  const int t = blockIdx.x, c = blockIdx.y;
  const int kd = (t * P + a) * PB;   // first column of the diagonal block
  const int k1 = min(Np, (c + 1) * LOO_CHUNK);
  if (k1 <= kd) return;
  const int k0 = max(c * LOO_CHUNK, kd);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ double sh[4][PB];
  const double *p = slab + (size_t)t * PB + 2 * lane + (size_t)(k0 + w) * lds;
  const size_t step = 4 * (size_t)lds;
  double s0 = 0.0, s1 = 0.0;
  // k1 - k0 is a multiple of 128: 32 columns or more per wave, eight loads in flight per lane
  for (int k = k0 + w; k < k1; k += 32) {
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const double2 *>(p + u * step);
#pragma unroll
    for (int u = 0; u < 8; u++) {
      s0 = fma(v[u].x, v[u].x, s0);
      s1 = fma(v[u].y, v[u].y, s1);
    }
    p += 8 * step;
  }
  sh[w][2 * lane] = s0;
  sh[w][2 * lane + 1] = s1;
  __syncthreads();
  if (threadIdx.x < PB) {
    const int r = threadIdx.x;
    part[(size_t)c * rows + (size_t)t * PB + r] = ((sh[0][r] + sh[1][r]) + sh[2][r]) + sh[3][r];
  }
}

// d[global row] = the row's partials, ascending from the chunk that holds its diagonal block
__global__ __launch_bounds__(256) void gpak_loo_rowsum_f64(const double *__restrict__ part, long rows, int nch, int P, int a,
                                                           double *__restrict__ d) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const long g = (r / PB) * P + a;
  double s = 0.0;
  for (int c = (int)(g * PB / LOO_CHUNK); c < nch; c++) s += part[(size_t)c * rows + r];
  d[g * PB + r % PB] = s;
}

// var_i = sn2 / d_i, mean_i = y_i - alpha_i var_i for i < N (padding rows take no part) and, per workgroup,
// part[block][NSUM]: [0] sum (y - mean)^2   [1] sum (y - mean)^2 / var   [2] sum log var -- reduced in fixed order by
// gpak_grad_reduce_f64
__global__ __launch_bounds__(256) void gpak_loo_finish_f64(int N, const double *__restrict__ d, const double *__restrict__ y,
                                                           const double *__restrict__ alpha, double sn2,
                                                           double *__restrict__ mean, double *__restrict__ var,
                                                           double *__restrict__ part) {
  __shared__ double red[4][3];
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[3] = {0.0, 0.0, 0.0};
  if (i < N) {
    const double v = sn2 / d[i];
    const double m = y[i] - alpha[i] * v;
    var[i] = v;
    mean[i] = m;
    const double r = y[i] - m;
    acc[0] = r * r;
    acc[1] = r * r / v;
    acc[2] = log(v);
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3)
    part[(size_t)blockIdx.x * NSUM + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The launches of the two steps on explicit arguments: what gpak_loo, gpak_loo_grad and the entries of
// gpak_dev_cv_kernels.h all run.  Pass a of P on a slab with Ta = my_tiles(Np, P, a) > 0 row tiles: part takes
// nch * Ta * 128 doubles (nch = the 512-column chunks of Np), d the Ta * 128 entries of the pass's rows.
static int loo_chunks(int Np) { return (Np + LOO_CHUNK - 1) / LOO_CHUNK; }
static void loo_launch_rowsumsq(hipStream_t st, const double *slab, long lds, int Np, int P, int a, double *part, double *d) {
  const int Ta = my_tiles(Np, P, a), nch = loo_chunks(Np);
  const long rows = (long)Ta * PB;
  hipLaunchKernelGGL(gpak_loo_sumsq_f64, dim3(Ta, nch), dim3(256), 0, st, slab, lds, Np, P, a, rows, part);
  hipLaunchKernelGGL(gpak_loo_rowsum_f64, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, part, rows, nch, P, a, d);
}
// mean, var and the three sums in out[0..2]; fin takes ceil(N / 256) * NSUM doubles
static void loo_launch_finish(hipStream_t st, int N, const double *d, const double *y, const double *alpha, double sn2,
                              double *mean, double *var, double *fin, double *out) {
  const int nfin = (N + 255) / 256;
  hipLaunchKernelGGL(gpak_loo_finish_f64, dim3(nfin), dim3(256), 0, st, N, d, y, alpha, sn2, mean, var, fin);
  hipLaunchKernelGGL(gpak_grad_reduce_f64, dim3(3), dim3(256), 0, st, fin, nfin, out);
}

// the summary from the three sums of gpak_loo_finish_f64 (gpak_loo and gpak_loo_grad: the same expressions, so the same bytes)
static void loo_fill_summary(gpak_loo_summary *summary, const double *red, int N, double ms, int P) {
  if (!summary) return;
  summary->mse = red[0] / N;
  summary->mssr = red[1] / N;
  summary->log_pl = -0.5 * (red[1] + red[2] + N * log(2.0 * M_PI));
  summary->ms = ms;
  summary->passes = P;
}

int gpak_loo_impl(gpak_ctx *ctx, double *mean, double *var, gpak_loo_summary *summary) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, T = Np / PB;
  // where G goes: the gradient's N x N workspace once it exists (one pass), otherwise a slab of LOO's own
  int P = 1;
  long lds = ctx->ld;
  double *slab = ctx->dG;
  if (!slab) {
    const long pad = ctx->ld - Np;   // the context's own padding of a leading dimension
    int rt = std::min(T, (ctx->loo_rows > 0 ? ctx->loo_rows : LOO_DEFAULT_ROWS) / PB);   // row tiles held at once
    for (;;) {
      P = (T + rt - 1) / rt;
      lds = (long)my_tiles(Np, P, 0) * PB + pad;
      if (gpak_loo_workspace(ctx, (size_t)lds * Np)) break;
      if (rt == 1) {
        ctx->err = "device allocation failed for the leave-one-out workspace (128 rows of L^-T do not fit)";
        return GPAK_ENOMEM;
      }
      rt = (rt + 1) / 2;   // hold fewer rows at once
    }
    slab = ctx->dLoo;
  }
  const int nch = (Np + LOO_CHUNK - 1) / LOO_CHUNK, nfin = (N + 255) / 256;
  const long rows_max = (long)my_tiles(Np, P, 0) * PB;
  // scratch in the gradient's partial-sum buffer: d, mean, var (Np each), the finish kernel's block sums, the chunk sums
  int rc = grad_partials(ctx, 3 * (size_t)Np + (size_t)nfin * NSUM + (size_t)nch * rows_max);
  if (rc) return rc;
  double *dd = ctx->dGpart, *dmean = dd + Np, *dvar = dmean + Np, *fin = dvar + Np, *part = fin + (size_t)nfin * NSUM;
  double *out = ctx->dRed + 32;
  GPAK_HIP(hipEventRecord(ctx->ev[7], st));
  const int GNB = 512;
  for (int a = 0; a < P; a++) {
    if (my_tiles(Np, P, a) == 0) continue;
    grad_g_subst(st, Np, GNB, P, a, [&](int b) {
      const size_t J = (size_t)b * GNB;
      return LBlockCol{ctx->dM + J + J * ctx->ld, ctx->ld, ctx->dInv + J / PB * 2 * PB * PB};
    }, slab, lds);
    loo_launch_rowsumsq(st, slab, lds, Np, P, a, part, dd);
  }
  loo_launch_finish(st, N, dd, ctx->dy, ctx->dAlpha, ctx->sn2, dmean, dvar, fin, out);
  double red[3];
  GPAK_HIP(hipMemcpyAsync(red, out, sizeof(red), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[9], st));
  if (mean) GPAK_HIP(hipMemcpyAsync(mean, dmean, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (var) GPAK_HIP(hipMemcpyAsync(var, dvar, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipStreamSynchronize(st));
  GPAK_HIP(hipGetLastError());
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[9]));
  loo_fill_summary(summary, red, N, ms, P);
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// The gradient of the leave-one-out pseudo-likelihood (gpak_loo_grad): F = -log_pl of gpak_loo (Rasmussen & Williams
// eq. 5.10-5.13).  With Kinv = (K + sn2 I)^-1 = B^-1 / sn2, alpha = Kinv y and kappa_i = Kinv_ii = d_i / sn2,
//   F = sum_i [ -1/2 log kappa_i + alpha_i^2 / (2 kappa_i) ] + N/2 log 2 pi,    dF / d theta = 1/2 sum_ij W_ij dK_ij / d theta,
//   c_i = (1 / kappa_i + alpha_i^2 / kappa_i^2) / 2,   b_i = alpha_i / kappa_i,   v = Kinv b,
//   W = 2 M - v alpha^T - alpha v^T,   M = Kinv diag(c) Kinv = H H^T,   H = Kinv diag(sqrt c).
// W is symmetric and every sum of ExactPass is linear in the weight, so the pass and its host assembly serve as they
// are: handed sn2 = 1 and a zero alpha, the skeleton's qw is the stored entry itself.  Memory: the gradient's two
// N x N workspaces and nothing else -- G then H in dG, B^-1 then W (lower tiles) in dBinv.
// ---------------------------------------------------------------------------------------
#define LM_T 64   // tile of the mirror and rank-2 kernels; 128 / LM_T tiles per GEMM tile side

// s_i = sqrt(c_i) / sn2 (column scale of H = B^-1 diag(s)) and r_i = b_i / sn2 (right-hand side of v = B^-1 r) for
// i < N; 0 on the padding
__global__ __launch_bounds__(256) void gpak_loo_vectors_f64(int N, int Np, const double *__restrict__ d,
                                                            const double *__restrict__ alpha, double sn2,
                                                            double *__restrict__ s, double *__restrict__ r) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Np) return;
  double sv = 0.0, rv = 0.0;
  if (i < N) {
    const double ik = sn2 / d[i];          // 1 / kappa_i: the LOO variance
    const double b = alpha[i] * ik;        // y_i - mu_i
    const double c = 0.5 * (ik + b * b);
    sv = sqrt(c) / sn2;
    rv = b / sn2;
  }
  s[i] = sv;
  r[i] = rv;
}

// H[i, k] = s_k B^-1[max(i, k), min(i, k)] for i, k < N and 0 elsewhere: the FULL Np x Np matrix from the stored lower
// tiles of B^-1.  One workgroup per 64 x 64 tile (bi >= bj) of the lower triangle: it writes the tile itself from
// registers and its transpose through LDS, so that the reads and both writes run along columns, 16 bytes per lane.
// A lane holds the row pair (2l, 2l + 1); in LDS both indices are permuted, x -> x / 2 + 32 (x & 1), and the pitch is
// 65: the stores of a half-wave then go to consecutive doubles and its transposed loads to doubles 65 apart, both free
// of bank conflicts.  A tile on the diagonal holds both halves of its own output: every entry is taken from the lower
// half, so that H diag(1/s) is symmetric bit for bit.  Np^2 / 2 reads, Np^2 writes.
#define LM_PERM(x) (((x) >> 1) + 32 * ((x) & 1))
__global__ __launch_bounds__(256) void gpak_loo_mirror_scale_f64(int N, const double *__restrict__ Binv, long ldb,
                                                                 const double *__restrict__ s, double *__restrict__ H, long ldh) {
  const int bi = blockIdx.x, bj = blockIdx.y;
  if (bi < bj) return;
  __shared__ double tile[LM_T][LM_T + 1];   // tile[LM_PERM(k)][LM_PERM(i)] = B^-1[i0 + i, k0 + k]
  const int i0 = bi * LM_T, k0 = bj * LM_T;
  const int l = threadIdx.x & 31, r = 2 * l, c8 = threadIdx.x >> 5;
  const bool diag = bi == bj;
  // rows i0 + r, i0 + r + 1 of the stored tile, eight of its columns
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = c8 + 8 * u;
    const double2 q = *reinterpret_cast<const double2 *>(Binv + (size_t)(i0 + r) + (size_t)(k0 + c) * ldb);
    tile[LM_PERM(c)][l] = q.x;
    tile[LM_PERM(c)][l + 32] = q.y;
    if (!diag) {
      const double sk = s[k0 + c];   // 0 for k >= N
      double2 o;
      o.x = i0 + r < N ? sk * q.x : 0.0;
      o.y = i0 + r + 1 < N ? sk * q.y : 0.0;
      *reinterpret_cast<double2 *>(H + (size_t)(i0 + r) + (size_t)(k0 + c) * ldh) = o;
    }
  }
  __syncthreads();
  if (diag) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int c = c8 + 8 * u, pc = LM_PERM(c);
      const double sk = s[k0 + c];
      double2 o;
      o.x = i0 + r < N ? sk * (r >= c ? tile[pc][l] : tile[l][pc]) : 0.0;
      o.y = i0 + r + 1 < N ? sk * (r + 1 >= c ? tile[pc][l + 32] : tile[l + 32][pc]) : 0.0;
      *reinterpret_cast<double2 *>(H + (size_t)(i0 + r) + (size_t)(k0 + c) * ldh) = o;
    }
    return;
  }
  // the transpose: rows k0 + r, k0 + r + 1 and eight of the columns i0 + c of H
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = c8 + 8 * u, pc = LM_PERM(c);
    const double si = s[i0 + c];     // 0 for i >= N
    double2 o;
    o.x = k0 + r < N ? si * tile[l][pc] : 0.0;
    o.y = k0 + r + 1 < N ? si * tile[l + 32][pc] : 0.0;
    *reinterpret_cast<double2 *>(H + (size_t)(k0 + r) + (size_t)(i0 + c) * ldh) = o;
  }
}

// W[i, j] -= v_i alpha_j + alpha_i v_j on the 64 x 64 tiles bi >= bj of the lower triangle, in place (v and alpha are 0 on
// the padding)
__global__ __launch_bounds__(256) void gpak_loo_rank2_f64(double *__restrict__ W, long ld, const double *__restrict__ v,
                                                          const double *__restrict__ alpha) {
  const int bi = blockIdx.x, bj = blockIdx.y;
  if (bi < bj) return;
  const int i = bi * LM_T + 2 * (threadIdx.x & 31), c8 = threadIdx.x >> 5;
  const double2 vi = *reinterpret_cast<const double2 *>(v + i), ai = *reinterpret_cast<const double2 *>(alpha + i);
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int j = bj * LM_T + c8 + 8 * u;
    const double vj = v[j], aj = alpha[j];
    double2 *p = reinterpret_cast<double2 *>(W + (size_t)i + (size_t)j * ld);
    double2 w = *p;
    w.x -= fma(vi.x, aj, ai.x * vj);
    w.y -= fma(vi.y, aj, ai.y * vj);
    *p = w;
  }
}

// The launches of the three on explicit arguments: what the gradients and the entries of gpak_dev_cv_kernels.h both run
static void loo_launch_vectors(hipStream_t st, int N, int Np, const double *d, const double *alpha, double sn2, double *s,
                               double *r) {
  hipLaunchKernelGGL(gpak_loo_vectors_f64, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, N, Np, d, alpha, sn2, s, r);
}
static void loo_launch_mirror_scale(hipStream_t st, int N, int Np, const double *Binv, long ldb, const double *s, double *H,
                                    long ldh) {
  hipLaunchKernelGGL(gpak_loo_mirror_scale_f64, dim3(Np / LM_T, Np / LM_T), dim3(256), 0, st, N, Binv, ldb, s, H, ldh);
}
static void loo_launch_rank2(hipStream_t st, int Np, double *W, long ld, const double *v, const double *alpha) {
  hipLaunchKernelGGL(gpak_loo_rank2_f64, dim3(Np / LM_T, Np / LM_T), dim3(256), 0, st, W, ld, v, alpha);
}

// gpak_loo_grad on a single-GPU context whose factor and alpha are current.  Everything goes to the context's stream
// and the host waits once, at the end.  Afterwards dG holds H and dBinv holds W: no claim is left behind, because
// gpak_grad / gpak_grad_hyb / gpak_grad_exact run grad_binv (G and B^-1 anew) and gpak_loo runs grad_g_subst (G anew)
// on EVERY call -- the context keeps no validity flag for either workspace.  dAlpha, the factor, nlZ and the first two
// vectors of dWork (z_ok) are only read.
int gpak_loo_grad_layout(gpak_ctx *ctx, int ng) {
  int te;
  return grad_layout(ctx, "gpak_loo_grad", ExactPass::white, ng, &te);
}

int gpak_loo_grad_impl(gpak_ctx *ctx, double *g, int ng, gpak_loo_summary *summary) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, T = Np / PB;
  const long ld = ctx->ld;
  int te = -1;
  int rc = grad_layout(ctx, "gpak_loo_grad", ExactPass::white, ng, &te);
  if (rc) return rc;
  // scratch in the gradient's partial-sum buffer: gpak_loo's layout (d, mean, var, the finish kernel's block sums, the
  // chunk sums), reused by the pair pass once d has been consumed
  const int nch = (Np + LOO_CHUNK - 1) / LOO_CHUNK, nfin = (N + 255) / 256;
  rc = grad_partials(ctx, std::max(3 * (size_t)Np + (size_t)nfin * NSUM + (size_t)nch * Np,
                                   (size_t)(Np / GT_ROWS) * (Np / GT_COLS) * NSUM));
  if (rc) return rc;
  rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  double *dd = ctx->dGpart, *dmean = dd + Np, *dvar = dmean + Np, *fin = dvar + Np, *part = fin + (size_t)nfin * NSUM;
  // five vectors of dWork behind the back substitution's scratch (which starts at 2 Np: api.hip sizes dWork as 70 Np +
  // that scratch), in what is otherwise the Gram mat-vec's transient room
  const int bw = ctx->bwd_bw;
  double *bs_scratch = ctx->dWork + 2 * (size_t)Np;
  double *vs = bs_scratch + (size_t)std::max(8 + bw / 32, 34) * bw, *vr = vs + Np, *vz = vr + Np, *vv = vz + Np, *zero = vv + Np;
  // 1. G = L^-T in dG, B^-1 in dBinv (records ev[7])
  rc = grad_binv(ctx);
  if (rc) return rc;
  // 2. the LOO diagonal and summary: what gpak_loo launches on dG (P = 1)
  loo_launch_rowsumsq(st, ctx->dG, ld, Np, 1, 0, part, dd);
  loo_launch_finish(st, N, dd, ctx->dy, ctx->dAlpha, ctx->sn2, dmean, dvar, fin, ctx->dRed + 32);
  // 3. s, r and v = B^-1 r by two substitutions on scratch vectors
  loo_launch_vectors(st, N, Np, dd, ctx->dAlpha, ctx->sn2, vs, vr);
  gpak_launch_trsv_fwd(st, Np, ctx->dM, ld, ctx->dInv, vr, vz);
  gpak_backsolve(ctx, st, vz, vv, bs_scratch);
  // 4. H into dG (G has been consumed)
  loo_launch_mirror_scale(st, N, Np, ctx->dBinv, ld, vs, ctx->dG, ld);
  // 5. 2 M = 2 H H^T, lower tiles, into dBinv; H is full: the k-loop runs over all of Np
  gpak_launch_gemm_nt(st, T, T, Np, 2.0, ctx->dG, ld, ctx->dG, ld, 0.0, ctx->dBinv, ld, 0, 0, true, true, false);
  // 6. W = 2 M - v alpha^T - alpha v^T
  loo_launch_rank2(st, Np, ctx->dBinv, ld, vv, ctx->dAlpha);
  // 7. the exact pass with W for its weight
  GPAK_HIP(hipMemsetAsync(zero, 0, sizeof(double) * Np, st));
  pair_sums<ExactPass>(st, ctx->kp, ctx->kinds, te, ctx->expans, ctx->bias, ctx->dist_mode, ctx->d, ctx->U.base, ctx->U.cap,
                       ctx->dX, Np, N, Np, zero, ctx->dBinv, ld, 0, 0, 1.0, ctx->dGpart, ctx->dRed + 8);
  double red[NSUM], lred[3];
  GPAK_HIP(hipMemcpyAsync(red, ctx->dRed + 8, sizeof(red), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(lred, ctx->dRed + 32, sizeof(lred), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[3], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[3]));
  GPAK_HIP(hipGetLastError());
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[3]));
  ctx->times.grad_ms = ms;
  ExactPass::assemble(ctx, red, g);
  loo_fill_summary(summary, lred, N, ms, 1);
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// The gradient of the leave-group-out criterion (gpak_cv_groups_grad): F = -log_pl of gpak_cv_groups.  With Ky = K + sn2 I =
// sn2 B, Kinv = B^-1 / sn2, alpha = Kinv y and, for a group with index set I, S = [B^-1]_II = R R^T, X = R^-1,
// w = X alpha_I, e_I = sn2 X^T w = y_I - mean_I:
//   F = sum_g [ 1/2 alpha_I . e_I - 1/2 log |S / sn2| ] + N/2 log 2 pi.
// d alpha = -Kinv dK alpha and d(Kinv)_II = -[Kinv dK Kinv]_II give
//   dF / d theta = 1/2 sum_ij W_ij d(Ky)_ij / d theta,   W = Kinv C Kinv - v alpha^T - alpha v^T,
//   C = blockdiag(C_I),  C_I = sn2 S^-1 + e_I e_I^T,  e = the N-vector of all e_I,  v = Kinv e.
// C_I = Q_I Q_I^T in closed form (cv_groups.hip), so W = H H^T - v alpha^T - alpha v^T with H = Kinv[:, perm] blockdiag(Q_I);
// the column order of H does not matter to H H^T, so H is mixed in place, column set by column set.  Groups of one sample:
// C_i = 2 c_i of gpak_loo_grad and W is its W.  W is symmetric: the exact pass and its assembly serve unchanged, handed
// sn2 = 1 and a zero alpha, as in gpak_loo_grad_impl.  Memory: the gradient's two N x N workspaces and the scratch buffer
// (the S of every group, one 128 x 128 matrix per bin of the mix, vectors and lists).
// ---------------------------------------------------------------------------------------
// s_k = c for k < N, 0 on the padding
__global__ __launch_bounds__(256) void gpak_lgo_colscale_f64(int N, int Np, double c, double *__restrict__ s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < Np) s[i] = i < N ? c : 0.0;
}
static void lgo_launch_colscale(hipStream_t st, int N, int Np, double c, double *s) {
  hipLaunchKernelGGL(gpak_lgo_colscale_f64, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, N, Np, c, s);
}

int gpak_cv_groups_grad_layout(gpak_ctx *ctx, int ng) {
  int te;
  return grad_layout(ctx, "gpak_cv_groups_grad", ExactPass::white, ng, &te);
}

// gpak_cv_groups_grad on a single-GPU context whose factor and alpha are current, the labels already checked.  Everything
// goes to the context's stream and the host waits once, at the end.  Afterwards dG holds H and dBinv holds W: no claim is
// left behind (see gpak_loo_grad_impl: the context keeps no validity flag for either workspace).  dAlpha, the factor, nlZ
// and the first two vectors of dWork are only read.
int gpak_cv_groups_grad_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *g, int ng,
                             gpak_cv_groups_summary *summary) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, T = Np / PB;
  const long ld = ctx->ld;
  int te = -1;
  int rc = grad_layout(ctx, "gpak_cv_groups_grad", ExactPass::white, ng, &te);
  if (rc) return rc;
  // the lists of gpak_cv_groups_impl, and the bins of the column mix: bin b holds the positions bstart[b] .. bstart[b + 1]
  // of perm; the Q of group g starts at (c0, c0) of its bin's row-major 128 x 128 matrix, c0 its first column in the bin
  const size_t nG = (size_t)n_groups;
  std::vector<long long> soff(nG + 1), qoff(nG);
  std::vector<int> sizes(nG), first(nG + 1);
  int max_size = 0;
  soff[0] = 0;
  for (size_t k = 0; k < nG; k++) {
    sizes[k] = offs[k + 1] - offs[k];
    max_size = std::max(max_size, sizes[k]);
    soff[k + 1] = soff[k] + gpak_cvg_s_elems(sizes[k]);
  }
  const int n_bins = gpak_cvg_pack_bins(sizes.data(), n_groups, first.data());
  std::vector<int> bstart((size_t)n_bins + 1);
  for (int b = 0; b <= n_bins; b++) bstart[b] = offs[first[b]];
  for (int b = 0; b < n_bins; b++)
    for (int k = first[b]; k < first[b + 1]; k++)
      qoff[k] = (long long)b * PB * PB + (long long)(offs[k] - bstart[b]) * (PB + 1);
  // scratch in the gradient's partial-sum buffer: gpak_cv_groups' layout (the S of every group, mean, var, logp, the groups'
  // three sums), then e (Np), the bins' matrices, the pair pass's block sums; then the lists
  const size_t nS = (size_t)soff[nG], nQ = (size_t)n_bins * PB * PB, nP = (size_t)T * (Np / GT_COLS) * NSUM;
  const size_t n_dbl = nS + 2 * (size_t)N + 4 * nG + (size_t)Np + nQ + nP;
  const size_t n_ll = 2 * nG + 1, n_int = (size_t)N + nG + 1 + 1 + (size_t)n_bins + 1;
  rc = grad_partials(ctx, n_dbl + n_ll + (n_int + 1) / 2);
  if (rc) return rc;
  rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  double *dS = ctx->dGpart, *dmean = dS + nS, *dvar = dmean + N, *dlogp = dvar + N, *dgsum = dlogp + nG;
  double *dE = dgsum + 3 * nG, *dQb = dE + Np, *part = dQb + nQ;
  long long *dsoff = reinterpret_cast<long long *>(part + nP), *dqoff = dsoff + nG + 1;
  int *dperm = reinterpret_cast<int *>(dqoff + nG), *doffs = dperm + N, *dinfo = doffs + nG + 1, *dbstart = dinfo + 1;
  // five vectors of dWork behind the back substitution's scratch, as gpak_loo_grad_impl takes them
  const int bw = ctx->bwd_bw;
  double *bs_scratch = ctx->dWork + 2 * (size_t)Np;
  double *vs = bs_scratch + (size_t)std::max(8 + bw / 32, 34) * bw, *vr = vs + Np, *vz = vr + Np, *vv = vz + Np, *zero = vv + Np;
  const int info0 = INT_MAX;
  GPAK_HIP(hipMemcpyAsync(dsoff, soff.data(), sizeof(long long) * (nG + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dqoff, qoff.data(), sizeof(long long) * nG, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dperm, perm, sizeof(int) * N, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(doffs, offs, sizeof(int) * (nG + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dinfo, &info0, sizeof(int), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dbstart, bstart.data(), sizeof(int) * ((size_t)n_bins + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemsetAsync(dE, 0, sizeof(double) * ((size_t)Np + nQ), st));   // e on the padding, the bins off their diagonal blocks
  // 1. G = L^-T in dG, B^-1 in dBinv (records ev[7])
  rc = grad_binv(ctx);
  if (rc) return rc;
  // 2. the two passes of gpak_cv_groups on dG, the solve pass with the weights e and Q
  gpak_cvg_launch_gram(ctx, ctx->dG, ld, n_groups, dperm, doffs, dsoff, dS);
  gpak_cvg_launch_solve_weights(ctx, n_groups, max_size, dS, dsoff, dperm, doffs, dmean, dvar, dlogp, dgsum, dinfo, dE, dQb, dqoff);
  // 3. r = e / sn2 and v = B^-1 r = Kinv e by two substitutions on scratch vectors
  gpak_launch_scale(st, Np, dE, 1.0 / ctx->sn2, vr);
  gpak_launch_trsv_fwd(st, Np, ctx->dM, ld, ctx->dInv, vr, vz);
  gpak_backsolve(ctx, st, vz, vv, bs_scratch);
  // 4. Kinv, full and zero on the padding, into dG (G has been consumed)
  lgo_launch_colscale(st, N, Np, 1.0 / ctx->sn2, vs);
  loo_launch_mirror_scale(st, N, Np, ctx->dBinv, ld, vs, ctx->dG, ld);
  // 5. H = Kinv[:, perm] blockdiag(Q_I), in place
  gpak_cvg_launch_mix(ctx, ctx->dG, ld, n_bins, dperm, dbstart, dQb);
  // 6. H H^T, lower tiles, into dBinv; H is full: the k-loop runs over all of Np
  gpak_launch_gemm_nt(st, T, T, Np, 1.0, ctx->dG, ld, ctx->dG, ld, 0.0, ctx->dBinv, ld, 0, 0, true, true, false);
  // 7. W = H H^T - v alpha^T - alpha v^T
  loo_launch_rank2(st, Np, ctx->dBinv, ld, vv, ctx->dAlpha);
  // 8. the exact pass with W for its weight
  GPAK_HIP(hipMemsetAsync(zero, 0, sizeof(double) * Np, st));
  pair_sums<ExactPass>(st, ctx->kp, ctx->kinds, te, ctx->expans, ctx->bias, ctx->dist_mode, ctx->d, ctx->U.base, ctx->U.cap,
                       ctx->dX, Np, N, Np, zero, ctx->dBinv, ld, 0, 0, 1.0, part, ctx->dRed + 8);
  double red[NSUM];
  std::vector<double> hsum(4 * nG);   // logp, then the three sums per group
  int info = 0;
  GPAK_HIP(hipMemcpyAsync(red, ctx->dRed + 8, sizeof(red), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(hsum.data(), dlogp, sizeof(double) * 4 * nG, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[3], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[3]));
  GPAK_HIP(hipGetLastError());
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[3]));
  ctx->times.grad_ms = ms;
  if (summary) {
    double sse = 0.0, ssr = 0.0, md = 0.0, lp = 0.0;
    for (size_t k = 0; k < nG; k++) {   // ascending, as gpak_cv_groups_impl adds them
      lp += hsum[k];
      sse += hsum[nG + 3 * k];
      ssr += hsum[nG + 3 * k + 1];
      md += hsum[nG + 3 * k + 2];
    }
    summary->mse = sse / N;
    summary->mssr = ssr / N;
    summary->msmd = md / N;
    summary->log_pl = lp;
    summary->ms = ms;
    summary->groups = n_groups;
    summary->max_size = max_size;
  }
  if (info != INT_MAX) {
    for (int k = 0; k < ng; k++) g[k] = std::numeric_limits<double>::quiet_NaN();
    ctx->err = "gpak_cv_groups_grad: S = [B^-1]_II of group " + std::to_string(info - 1) + " is not positive definite";
    return GPAK_ENOTPD;
  }
  ExactPass::assemble(ctx, red, g);
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// The gradient of the k-fold criterion (gpak_cv_folds_grad): F = -log_pl of gpak_cv_folds, the derivation above with groups of
// any size.  C_I = Q_I Q_I^T holds in the same closed form whatever the group's size, with X^T = T = R^-T of cv_folds.hip:
//   Q_I = sqrt(sn2) T + (beta / sqrt(sn2)) e_I w^T,   beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)).
// The groups of at most GPAK_CV_GROUP_MAX samples take the passes of gpak_cv_groups_grad_impl on the compacted lists of
// gpak_cv_folds_impl (without a larger group: the same launches on the same lists, the same bytes).  Every other group
// runs gpak_cv_folds_impl's sequence (gpak_cvf_run_group) and leaves Q_I in dCvfQ; its columns of Kinv are mixed out of
// place through dCvfP once Kinv stands in dG: up to two column tiles by gpak_cvf_mix_f64, wider by a gather, the bulk GEMM and
// a scatter (gpak_cvf_mix_group).  Memory beyond gpak_cv_groups_grad's and gpak_cv_folds': dCvfQ, and dCvfP grown to
// Np x m_p,max, twice that when the largest group goes by GEMM.
// ---------------------------------------------------------------------------------------
int gpak_cv_folds_grad_layout(gpak_ctx *ctx, int ng) {
  int te;
  return grad_layout(ctx, "gpak_cv_folds_grad", ExactPass::white, ng, &te);
}

int gpak_cv_folds_grad_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *g, int ng,
                            gpak_cv_groups_summary *summary, int flags) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, T = Np / PB;
  const long ld = ctx->ld;
  int te = -1;
  int rc = grad_layout(ctx, "gpak_cv_folds_grad", ExactPass::white, ng, &te);
  if (rc) return rc;
  gpak_cvf_plan pl;
  gpak_cvf_make_plan(perm, offs, n_groups, Np, !(flags & GPAK_CV_FOLDS_NO_BATCH), pl);
  const size_t nSm = pl.small_id.size(), nL = pl.large_id.size(), nG = (size_t)n_groups;
  // the bins of the small groups' column mix, over the compacted lists: as gpak_cv_groups_grad_impl
  std::vector<long long> qoff(nSm);
  std::vector<int> sizes(nSm), first(nSm + 1), bstart(1, 0);
  int n_bins = 0;
  if (nSm) {
    for (size_t k = 0; k < nSm; k++) sizes[k] = pl.soffs[k + 1] - pl.soffs[k];
    n_bins = gpak_cvg_pack_bins(sizes.data(), (int)nSm, first.data());
    bstart.resize((size_t)n_bins + 1);
    for (int b = 0; b <= n_bins; b++) bstart[b] = pl.soffs[first[b]];
    for (int b = 0; b < n_bins; b++)
      for (int k = first[b]; k < first[b + 1]; k++)
        qoff[k] = (long long)b * PB * PB + (long long)(pl.soffs[k] - bstart[b]) * (PB + 1);
  }
  rc = gpak_cvf_reserve(ctx, "gpak_cv_folds_grad", pl, true);
  if (rc) return rc;
  // scratch in the gradient's partial-sum buffer: gpak_cv_folds' layout (the S of every small group, mean, var, then per kind
  // of group logp and the three sums), then e (Np), the bins' matrices, the pair pass's block sums; then the lists
  const size_t nSs = (size_t)pl.soff.back(), nQ = (size_t)n_bins * PB * PB, nPp = (size_t)T * (Np / GT_COLS) * NSUM;
  const size_t n_dbl = nSs + 2 * (size_t)N + 4 * nG + (size_t)Np + nQ + nPp;
  const size_t n_ll = 2 * nSm + 1, n_int = pl.sperm.size() + (nSm + 1) + (size_t)N + (1 + nL) + (size_t)n_bins + 1;
  rc = grad_partials(ctx, n_dbl + n_ll + (n_int + 1) / 2);
  if (rc) return rc;
  rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  double *dS = ctx->dGpart, *dmean = dS + nSs, *dvar = dmean + N;
  double *dlogp_s = dvar + N, *dgsum_s = dlogp_s + nSm, *dlogp_l = dgsum_s + 3 * nSm, *dgsum_l = dlogp_l + nL;
  double *dE = dgsum_l + 3 * nL, *dQb = dE + Np, *part = dQb + nQ;
  long long *dsoff = reinterpret_cast<long long *>(part + nPp), *dqoff = dsoff + nSm + 1;
  int *dsperm = reinterpret_cast<int *>(dqoff + nSm), *dsoffs = dsperm + pl.sperm.size(), *dperm = dsoffs + nSm + 1;
  int *dinfo = dperm + N, *dbstart = dinfo + 1 + nL;        // dinfo[0]: the batched groups; [1 + k]: one-at-a-time group k
  // five vectors of dWork behind the back substitution's scratch, as gpak_loo_grad_impl takes them
  const int bw = ctx->bwd_bw;
  double *bs_scratch = ctx->dWork + 2 * (size_t)Np;
  double *vs = bs_scratch + (size_t)std::max(8 + bw / 32, 34) * bw, *vr = vs + Np, *vz = vr + Np, *vv = vz + Np, *zero = vv + Np;
  const std::vector<int> info0(1 + nL, INT_MAX);
  GPAK_HIP(hipMemcpyAsync(dinfo, info0.data(), sizeof(int) * (1 + nL), hipMemcpyHostToDevice, st));
  if (nSm) {
    GPAK_HIP(hipMemcpyAsync(dsoff, pl.soff.data(), sizeof(long long) * (nSm + 1), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dqoff, qoff.data(), sizeof(long long) * nSm, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dsperm, pl.sperm.data(), sizeof(int) * pl.sperm.size(), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dsoffs, pl.soffs.data(), sizeof(int) * (nSm + 1), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dbstart, bstart.data(), sizeof(int) * ((size_t)n_bins + 1), hipMemcpyHostToDevice, st));
  }
  if (nL) GPAK_HIP(hipMemcpyAsync(dperm, perm, sizeof(int) * N, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemsetAsync(dE, 0, sizeof(double) * ((size_t)Np + nQ), st));   // e on the padding, the bins off their diagonal blocks
  // 1. G = L^-T in dG, B^-1 in dBinv (records ev[7])
  rc = grad_binv(ctx);
  if (rc) return rc;
  // 2. the small groups: the two passes of gpak_cv_groups on dG, the solve pass with the weights e and Q
  if (nSm) {
    gpak_cvg_launch_gram(ctx, ctx->dG, ld, (int)nSm, dsperm, dsoffs, dsoff, dS);
    gpak_cvg_launch_solve_weights(ctx, (int)nSm, pl.max_small, dS, dsoff, dsperm, dsoffs, dmean, dvar, dlogp_s, dgsum_s, dinfo, dE,
                                  dQb, dqoff);
  }
  // 3. every other group alone: gpak_cv_folds' sequence, then its Q into the store and its e into dE
  for (size_t k = 0; k < nL; k++)
    if ((rc = gpak_cvf_run_group(ctx, pl, k, perm, offs, ctx->dG, dperm, dinfo + 1 + k, dmean, dvar, dlogp_l + k, dgsum_l + 3 * k, dE)))
      return rc;
  // 4. r = e / sn2 and v = B^-1 r = Kinv e by two substitutions on scratch vectors
  gpak_launch_scale(st, Np, dE, 1.0 / ctx->sn2, vr);
  gpak_launch_trsv_fwd(st, Np, ctx->dM, ld, ctx->dInv, vr, vz);
  gpak_backsolve(ctx, st, vz, vv, bs_scratch);
  // 5. Kinv, full and zero on the padding, into dG (G has been consumed)
  lgo_launch_colscale(st, N, Np, 1.0 / ctx->sn2, vs);
  loo_launch_mirror_scale(st, N, Np, ctx->dBinv, ld, vs, ctx->dG, ld);
  // 6. H = Kinv[:, I] Q_I: the bins of the small groups in place,
  if (nSm) gpak_cvg_launch_mix(ctx, ctx->dG, ld, n_bins, dsperm, dbstart, dQb);
  // 7. every other group through dCvfP (the group sequences are done with it)
  for (size_t k = 0; k < nL; k++) {
    const int gk = pl.large_id[k], o = offs[gk];
    gpak_cvf_mix_group(ctx, pl, k, dperm + o, offs[gk + 1] - o);
  }
  // 8. W = H H^T - v alpha^T - alpha v^T (lower tiles, into dBinv) and the exact pass with W for its weight
  gpak_launch_gemm_nt(st, T, T, Np, 1.0, ctx->dG, ld, ctx->dG, ld, 0.0, ctx->dBinv, ld, 0, 0, true, true, false);
  loo_launch_rank2(st, Np, ctx->dBinv, ld, vv, ctx->dAlpha);
  GPAK_HIP(hipMemsetAsync(zero, 0, sizeof(double) * Np, st));
  pair_sums<ExactPass>(st, ctx->kp, ctx->kinds, te, ctx->expans, ctx->bias, ctx->dist_mode, ctx->d, ctx->U.base, ctx->U.cap,
                       ctx->dX, Np, N, Np, zero, ctx->dBinv, ld, 0, 0, 1.0, part, ctx->dRed + 8);
  double red[NSUM];
  std::vector<double> hsum(4 * nG);   // as on the device: logp and the three sums of the small groups, then of the others
  std::vector<int> hinfo(1 + nL, 0);
  GPAK_HIP(hipMemcpyAsync(red, ctx->dRed + 8, sizeof(red), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(hsum.data(), dlogp_s, sizeof(double) * 4 * nG, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(hinfo.data(), dinfo, sizeof(int) * (1 + nL), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[3], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[3]));
  GPAK_HIP(hipGetLastError());
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[3]));
  ctx->times.grad_ms = ms;
  rc = gpak_cvf_finish(ctx, "gpak_cv_folds_grad", pl, hsum.data(), hinfo.data(), ms, nullptr, summary);
  if (rc) {
    for (int k = 0; k < ng; k++) g[k] = std::numeric_limits<double>::quiet_NaN();
    return rc;
  }
  ExactPass::assemble(ctx, red, g);
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// The as-written gradient distributed over P ranks that all hold the factor as packed panels (csrc/dist.hip):
// rank a computes its rows of G = L^-T (grad_g_subst: N^3/(3P) flops, no communication); the slabs are all-gathered
// (the caller's broadcasts); B^-1 rows of the same blocks = sum_k G[I,k] G[J,k] for J <= I against every rank's slab --
// N^3/(3P) flops; then the pair pass on those rows and one all-reduce of the NSUM sums.
// ---------------------------------------------------------------------------------------
static int status() { return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP; }

extern "C" int gpak_dev_grad_g_rows(void *stream, int Np, int nb, int P, int a, const double *const *panels,
                                    const double *const *invs, double *slab) {
  grad_g_subst((hipStream_t)stream, Np, nb, P, a, [&](int b) { return LBlockCol{panels[b], Np - (long)b * nb, invs[b]}; },
               slab, (long)my_tiles(Np, P, a) * PB);
  return status();
}

// binv: rows_a x (P * Tmax * 128), leading dimension rows_a; the 128-column group of global block g = u*P + b sits at
// group index b*Tmax + u (so that the launch for source rank b writes a contiguous range of tile columns).  One call
// per source rank: the caller needs only its own slab and the one that is passing through (dist.hip streams them)
extern "C" int gpak_dev_grad_binv_rows(void *stream, int Np, int P, int a, int b, const double *slab_a, const double *slab_b,
                                       double *binv) {
  hipStream_t st = (hipStream_t)stream;
  if (b < 0 || b >= P || a < 0 || a >= P) return GPAK_EINVAL;
  const int Ta = my_tiles(Np, P, a), Tb = my_tiles(Np, P, b), Tmax = my_tiles(Np, P, 0);
  if (Ta == 0 || Tb == 0) return GPAK_OK;
  const long rows = (long)Ta * PB;
  // tile (t, u): global row block t*P + a, global column block u*P + b; needed when u*P + b <= t*P + a, i.e.
  // skipped when t < u + (b > a ? 1 : 0)
  gpak_launch_gemm_nt_k0map(st, Ta, Tb, Np, 1.0, slab_a, rows, slab_b, (long)Tb * PB, binv + (size_t)b * Tmax * PB * rows,
                            rows, b > a ? 1 : 0, P, a);
  return status();
}

// the distributed entry points know one composition: ExpAns + Bias
static KernParams expans_kp(const double *expans, double bias, int dist_mode) {
  KernParams kp;
  const int kinds[GPAK_MAX_TERMS] = {GPAK_KERN_EXPANS, 0, 0};
  gpak_build_kp(1, kinds, expans, bias, 0.0, dist_mode & 0xF, &kp, nullptr);
  kp.d = (dist_mode & GPAK_DIST_D4) ? 4 : 3;
  return kp;
}

// Either pass alone on caller-owned buffers (gpak_dev.h): out16[0..NSUM) = the sums of rank a's row blocks (P >= 1), or
// of the whole lower triangle (P == 0); part: Ta * (Np / 64) * NSUM doubles of scratch.  `kern` as gpak_dev_transform_k.
extern "C" int gpak_dev_grad_pair_sums(void *stream, int pass, const double *u, int cap, const double *x_soa, int xs, int n,
                                       int Np, const double *alpha, const double *binv, long ld, int P, int a,
                                       const double *kern, double bias, double sn2, int dist_mode, double *part,
                                       double *out16) {
  hipStream_t st = (hipStream_t)stream;
  if (pass != 0 && pass != 1) return GPAK_EINVAL;
  if (P < 0 || (P > 0 && (a < 0 || a >= P)) || (P == 0 && (ld & 1))) return GPAK_EINVAL;
  const bool hyb = dist_mode & GPAK_DIST_HYB;
  int kinds[GPAK_MAX_TERMS] = {GPAK_KERN_EXPANS, 0, 0};
  for (int t = 0; hyb && t < GPAK_MAX_TERMS; t++) kinds[t] = (int)kern[1 + t];
  KernParams kp;
  if (gpak_build_kp(hyb ? (int)kern[0] : 1, kinds, hyb ? kern + 5 : kern, bias, hyb ? kern[4] : 0.0, dist_mode & 0xF, &kp,
                    nullptr) != GPAK_OK)
    return GPAK_EINVAL;
  kp.d = (dist_mode & GPAK_DIST_D4) ? 4 : 3;
  if (kp.white != 0.0) return GPAK_EINVAL;
  int te = -1;
  const double *expans = nullptr, *p = hyb ? kern + 5 : kern;
  for (int t = 0; t < kp.nterms; t++) {
    if (kinds[t] == GPAK_KERN_EXPANS) {
      if (te >= 0) return GPAK_EINVAL;
      te = t; expans = p;
    }
    p += kinds[t] == GPAK_KERN_EXPANS ? 8 : kinds[t] == GPAK_KERN_EXP ? 2 : 3;
  }
  hipMemsetAsync(out16, 0, sizeof(double) * NSUM, st);
  if (pass == 0)
    pair_sums<RefPass>(st, kp, kinds, te, expans, bias, kp.mode, kp.d, u, cap, x_soa, xs, n, Np, alpha, binv, ld, P, a, sn2,
                       part, out16);
  else
    pair_sums<ExactPass>(st, kp, kinds, te, expans, bias, kp.mode, kp.d, u, cap, x_soa, xs, n, Np, alpha, binv, ld, P, a, sn2,
                         part, out16);
  return status();
}

// out[0..NSUM) = this rank's share of the as-written pair sums, out[NSUM] = sum_i ((y_i - f_i)^2 / sn2 - 1) (replicated:
// NOT to be all-reduced); the distributed entry points know one composition: ExpAns + Bias
extern "C" int gpak_dev_grad_pairs_rows(void *stream, const double *u, int cap, const double *x_soa, int xs, int n, int Np,
                                        const double *y, const double *f, const double *alpha, const double *binv, int P,
                                        int a, const double *expans, double bias, double sn2, int dist_mode, double *part,
                                        double *out) {
  if (P < 1) return GPAK_EINVAL;
  const int rc = gpak_dev_grad_pair_sums(stream, 0, u, cap, x_soa, xs, n, Np, alpha, binv, 0, P, a, expans, bias, sn2,
                                         dist_mode & ~GPAK_DIST_HYB, part, out);
  if (rc != GPAK_OK) return rc;
  hipLaunchKernelGGL(gpak_lpdhyp_f64, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, y, f, sn2, out + NSUM);
  return status();
}

// the constants of the pair pass (M_p = S % S_p as {00,01,02,11,12,22}, and 2 * its column sums): exported so that a
// test engine can restate the pass without restating Kernel.cpp:955-1166 a third time
extern "C" int gpak_dev_grad_consts(const double *expans, double *M36, double *m2_18) {
  GradConsts gc;
  memset(&gc, 0, sizeof(gc));
  build_grad_consts(expans, gc);
  memcpy(M36, gc.M, sizeof(double) * 36);
  memcpy(m2_18, gc.m2, sizeof(double) * 18);
  return GPAK_OK;
}

// host side of the distributed gradient: g[10] from the all-reduced sums
extern "C" int gpak_dev_grad_finish_d(const double *expans, double bias, double sn2, int n, int d, const double *red,
                                      double *g) {
  const KernParams kp = expans_kp(expans, bias, GPAK_DIST_DIRECT);
  const int kinds[GPAK_MAX_TERMS] = {GPAK_KERN_EXPANS, 0, 0};
  gpak_grad_assemble(kp, kinds, expans, d == 4 ? 4 : 3, n, sn2, red, g);
  return GPAK_OK;
}
extern "C" int gpak_dev_grad_finish(const double *expans, double bias, double sn2, int n, const double *red, double *g) {
  return gpak_dev_grad_finish_d(expans, bias, sn2, n, 3, red, g);
}

// ---------------------------------------------------------------------------------------
// include/gpak_dev_cv_kernels.h: the leave-one-out kernels alone on caller-owned device buffers, through the launches the
// calls above run
// ---------------------------------------------------------------------------------------
static bool loo_misaligned(const void *p) { return (reinterpret_cast<size_t>(p) & 15) != 0; }
static bool loo_bad_np(int Np) { return Np < PB || Np % PB != 0; }

extern "C" int gpak_dev_loo_rowsumsq(void *stream, const double *slab, long lds, int Np, int P, int a, double *part, double *d) {
  if (!slab || !part || !d || loo_bad_np(Np) || P < 1 || a < 0 || a >= P) return GPAK_EINVAL;
  const int Ta = my_tiles(Np, P, a);
  if (Ta == 0 || lds < (long)Ta * PB || (lds & 1) || loo_misaligned(slab)) return GPAK_EINVAL;
  loo_launch_rowsumsq((hipStream_t)stream, slab, lds, Np, P, a, part, d);
  return status();
}

extern "C" int gpak_dev_loo_finish(void *stream, int N, const double *d, const double *y, const double *alpha, double sn2,
                                   double *mean, double *var, double *part, double *sums) {
  if (!d || !y || !alpha || !mean || !var || !part || !sums || N < 1 || !(sn2 > 0.0)) return GPAK_EINVAL;
  loo_launch_finish((hipStream_t)stream, N, d, y, alpha, sn2, mean, var, part, sums);
  return status();
}

extern "C" int gpak_dev_loo_vectors(void *stream, int N, int Np, const double *d, const double *alpha, double sn2, double *s,
                                    double *r) {
  if (!d || !alpha || !s || !r || N < 1 || N > Np || !(sn2 > 0.0)) return GPAK_EINVAL;
  loo_launch_vectors((hipStream_t)stream, N, Np, d, alpha, sn2, s, r);
  return status();
}

extern "C" int gpak_dev_loo_mirror_scale(void *stream, int N, int Np, const double *Binv, long ldb, const double *s, double *H,
                                         long ldh) {
  if (!Binv || !s || !H || N < 1 || N > Np || loo_bad_np(Np) || ldb < Np || ldh < Np || (ldb & 1) || (ldh & 1) ||
      loo_misaligned(Binv) || loo_misaligned(H))
    return GPAK_EINVAL;
  loo_launch_mirror_scale((hipStream_t)stream, N, Np, Binv, ldb, s, H, ldh);
  return status();
}

extern "C" int gpak_dev_loo_rank2(void *stream, int Np, double *W, long ld, const double *v, const double *alpha) {
  if (!W || !v || !alpha || loo_bad_np(Np) || ld < Np || (ld & 1) || loo_misaligned(W) || loo_misaligned(v) ||
      loo_misaligned(alpha))
    return GPAK_EINVAL;
  loo_launch_rank2((hipStream_t)stream, Np, W, ld, v, alpha);
  return status();
}

extern "C" int gpak_dev_lgo_colscale(void *stream, int N, int Np, double c, double *s) {
  if (!s || N < 0 || N > Np || Np < 1) return GPAK_EINVAL;
  lgo_launch_colscale((hipStream_t)stream, N, Np, c, s);
  return status();
}
