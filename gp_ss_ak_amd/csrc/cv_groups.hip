// cv_groups.hip -- leave-group-out cross-validation from the Cholesky factor on gfx950 (gpak_cv_groups).
//
// With Ky = K + sn2 I = sn2 B, B = L L^T, G = L^-T (upper triangular) and alpha = Ky^-1 y (Rasmussen & Williams 5.4.2 in
// block form), for a group with index set I of size s <= GPAK_CV_GROUP_MAX:
//   S       = [B^-1]_II = G_I G_I^T = R R^T           (R lower triangular)
//   e_I     = sn2 S^-1 alpha_I,   mean_I = y_I - e_I
//   Sigma_I = sn2 S^-1,           var_i = sn2 sum_j (R^-1)_ji^2
//   logp_g  = -1/2 alpha_I . e_I - 1/2 (s log sn2 - 2 sum_j log R_jj) - s/2 log 2 pi
// Three steps on the context's stream, one host synchronisation at the end:
//   1. G as ONE full matrix: gpak_grad_g_full (grad.hip: the L^-T driver with P = 1);
//   2. gpak_cvg_gram_f64    one workgroup per group: S from the group's rows of G, fp64 MFMA, lower 16 x 16 tiles;
//   3. gpak_cvg_solve_f64   one workgroup per group: R, R^-1, e, var, logp and the group's three sums, S in LDS.
// The summary is added on the host over the groups in ascending order.
//
// gpak_cv_groups_grad (grad.hip) runs the same two passes and needs, per group, the weights of the gradient of
// F = -log_pl:  C_I = sn2 S^-1 + e_I e_I^T = Q_I Q_I^T  with, for X = R^-1 and w = X alpha_I (so e_I = sn2 X^T w),
//   C_I = sn2 X^T (I + sn2 w w^T) X,   (I + beta w w^T)^2 = I + sn2 w w^T  for  beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)),
//   Q_I = sqrt(sn2) X^T + (beta / sqrt(sn2)) e_I w^T
// -- a factor in closed form, no second Cholesky.  gpak_cvg_solve_f64<true> writes e_I and Q_I beside its other outputs
// and gpak_cvg_mix_f64 multiplies the columns of Kinv by the Q_I, a bin of groups at a time.
#include <atomic>
#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/gpak_dev_cv_kernels.h"
#include "gpak_internal.h"

#define CVG_MAX GPAK_CV_GROUP_MAX   // 128: rows of a group, 8 MFMA tiles of 16
#define CVG_KC 32                   // columns of G staged per step (cut at absolute multiples of CVG_KC)
#define CVG_PITCH 144               // doubles per staged column: 288 dwords = 32 (mod 64), so the two 16-lane halves of a
                                    // half-wave's fragment read (k, k + 1) fall on disjoint banks
#define CVG_RP 129                  // row pitch of the solve's LDS matrix: rows and columns both conflict-free

typedef double cvg_d4 __attribute__((ext_vector_type(4)));

static __host__ __device__ inline int cvg_pad16(int s) { return (s + 15) & ~15; }

// S of group g = blockIdx.x, lower 16 x 16 tiles (the diagonal tiles whole), column-major with leading dimension
// sp = pad16(s) at Sbuf + soff[g].  Rows s..sp of the staged columns are zero, so the padding of S is zero.
// The columns run from the 128-tile that holds the group's smallest row (everything left of it is exact zeros of
// gpak_identity_f64) in steps of CVG_KC; a step is staged in LDS by all four waves (lanes along the group's rows: a
// contiguous hole reads 512 bytes per wave and column) while the next is on its way to registers.  Wave w owns the tile
// rows w and 7 - w: 9 of the 36 lower tiles each.  Every element S_ij is ONE accumulator chain over the 4-column MFMA
// steps in ascending absolute column order, and the skipped columns contribute exact zeros: the order in which the
// products of S_ij are added depends on (i, j) alone -- not on the grid, the buffer that holds G or its leading dimension.
__global__ __launch_bounds__(256) void gpak_cvg_gram_f64(const double *__restrict__ G, long ld, int Np,
                                                         const int *__restrict__ perm, const int *__restrict__ offs,
                                                         const long long *__restrict__ soff, double *__restrict__ Sbuf) {
  __shared__ double sh[CVG_KC * CVG_PITCH];
  const int g = blockIdx.x;
  const int o = offs[g], s = offs[g + 1] - o, sp = cvg_pad16(s);
  const int nt = __builtin_amdgcn_readfirstlane(sp >> 4);
  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int rtA = w, rtB = 7 - w;
  const int r = t & 127, kh = t >> 7;      // staging: row r of the group, columns kh * 16 .. kh * 16 + 15 of the step
  const bool live = r < s;
  const int row = live ? perm[o + r] : 0;
  const int k0 = (perm[o] / CVG_MAX) * CVG_MAX;   // the members are sorted: perm[o] is the smallest row
  cvg_d4 accA[4], accB[8];
#pragma unroll
  for (int c = 0; c < 4; c++) accA[c] = (cvg_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 8; c++) accB[c] = (cvg_d4){0.0, 0.0, 0.0, 0.0};
  double v[16];
  const double *p = G + (size_t)row + (size_t)(k0 + kh * 16) * ld;
  auto load = [&]() {
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = live ? p[(size_t)u * ld] : 0.0;
    p += (size_t)CVG_KC * ld;
  };
  load();
  for (int k = k0; k < Np; k += CVG_KC) {
#pragma unroll
    for (int u = 0; u < 16; u++) sh[(kh * 16 + u) * CVG_PITCH + r] = v[u];
    __syncthreads();
    if (k + CVG_KC < Np) load();
#pragma unroll
    for (int kq = 0; kq < CVG_KC / 4; kq++) {
      const double *col = sh + (kq * 4 + l4) * CVG_PITCH + l15;
      double f[8];
#pragma unroll
      for (int c = 0; c < 8; c++) f[c] = c < nt ? col[c * 16] : 0.0;
      if (rtA < nt) {
        const double fa = col[rtA * 16];
#pragma unroll
        for (int c = 0; c < 4; c++)
          if (c <= rtA) accA[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[c], fa, accA[c], 0, 0, 0);
      }
      if (rtB < nt) {
        const double fb = col[rtB * 16];
#pragma unroll
        for (int c = 0; c < 8; c++)
          if (c <= rtB) accB[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[c], fb, accB[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // lane holds of tile (rt, ct): row rt * 16 + l15, columns ct * 16 + l4 + 4 q
  double *S = Sbuf + soff[g];
  if (rtA < nt) {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c <= rtA)
#pragma unroll
        for (int q = 0; q < 4; q++) S[(size_t)(rtA * 16 + l15) + (size_t)(c * 16 + l4 + 4 * q) * sp] = accA[c][q];
  }
  if (rtB < nt) {
#pragma unroll
    for (int c = 0; c < 8; c++)
      if (c <= rtB)
#pragma unroll
        for (int q = 0; q < 4; q++) S[(size_t)(rtB * 16 + l15) + (size_t)(c * 16 + l4 + 4 * q) * sp] = accB[c][q];
  }
}

// Group g = blockIdx.x from its S.  One LDS matrix A (row pitch CVG_RP) holds R on and below the diagonal and, once R is
// final, X^T = R^-T strictly above it (the diagonal of X = R^-1 in xd): right-looking Cholesky by all 256 threads, then
// thread i forms column i of X by forward substitution, then the vectors
//   w = X alpha_I,   e = sn2 X^T w,   var_i = sn2 sum_j X_ji^2
// and thread 0 adds the group's sums in ascending order: gsum[3 g ..] = sum e_i^2, sum e_i^2 / var_i, alpha_I . e_I.
// A pivot that is not positive: the group's outputs are NaN and info takes the smallest such g + 1.
// kWeights (gpak_cv_groups_grad): the same arithmetic, and afterwards e_I scattered into E (an Np-vector the caller has
// zeroed) and Q_I written ROW-major with pitch CVG_MAX at Qb + qoff[g] -- the diagonal block of the group's bin matrix,
// whose rows are what gpak_cvg_mix_f64 stages; X, w and e are in LDS already and Q needs no more of it.  A failed group
// writes neither.
template <bool kWeights>
__global__ __launch_bounds__(256) void gpak_cvg_solve_f64(const double *__restrict__ Sbuf, const long long *__restrict__ soff,
                                                          const int *__restrict__ perm, const int *__restrict__ offs,
                                                          const double *__restrict__ y, const double *__restrict__ alpha,
                                                          double sn2, double *__restrict__ mean, double *__restrict__ var,
                                                          double *__restrict__ logp, double *__restrict__ gsum, int *info,
                                                          double *__restrict__ E, double *__restrict__ Qb,
                                                          const long long *__restrict__ qoff) {
  extern __shared__ double cvg_lds[];
  const int g = blockIdx.x, t = threadIdx.x;
  const int o = offs[g], s = offs[g + 1] - o, sp = cvg_pad16(s);
  double *A = cvg_lds;                       // s rows of CVG_RP
  double *xd = A + (size_t)s * CVG_RP;       // then six vectors of CVG_MAX
  double *al = xd + CVG_MAX, *wv = al + CVG_MAX, *ev = wv + CVG_MAX, *vv = ev + CVG_MAX, *lg = vv + CVG_MAX;
  const double *S = Sbuf + soff[g];
  for (int e = t; e < sp * s; e += 256) {    // columns 0 .. s - 1, rows j .. s - 1
    const int i = e % sp, j = e / sp;
    if (i >= j && i < s) A[i * CVG_RP + j] = S[e];
  }
  if (t < s) al[t] = alpha[perm[o + t]];
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < s; j++) {
    const double d = A[j * CVG_RP + j];      // every thread reads the same value: the branch is uniform
    if (!(d > 0.0)) { ok = false; break; }
    const double rj = sqrt(d), ri = 1.0 / rj;
    __syncthreads();
    if (t == 0) { A[j * CVG_RP + j] = rj; xd[j] = ri; lg[j] = log(rj); }
    for (int i = j + 1 + t; i < s; i += 256) A[i * CVG_RP + j] *= ri;
    __syncthreads();
    for (int k = j + 1 + (t >> 4); k < s; k += 16) {   // column k of the trailing block, rows k .. s - 1, 16 lanes each
      const double akj = A[k * CVG_RP + j];
      for (int i = k + (t & 15); i < s; i += 16) A[i * CVG_RP + k] = fma(-A[i * CVG_RP + j], akj, A[i * CVG_RP + k]);
    }
    __syncthreads();
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (!ok) {
    if (t < s) { mean[perm[o + t]] = nan; var[perm[o + t]] = nan; }
    if (t == 0) {
      logp[g] = nan;
      gsum[3 * g] = gsum[3 * g + 1] = gsum[3 * g + 2] = nan;
      atomicMin(info, g + 1);
    }
    return;
  }
  // column i of X = R^-1 by thread i: X_ii = 1 / R_ii, X_ji = -(sum_{i <= k < j} R_jk X_ki) / R_jj, kept as A[i][j] (j > i).
  // j is uniform and k descends from j - 1 in every lane: R_jk is one address per step (a broadcast) and the lanes' own
  // X_ki lie CVG_RP apart
  for (int j = 1; j < s; j++) {
    const int i = t;
    if (i < j) {
      const double *Rj = A + j * CVG_RP;
      double *xi = A + i * CVG_RP;
      double acc = 0.0;
#pragma unroll 4
      for (int k = j - 1; k > i; k--) acc = fma(Rj[k], xi[k], acc);
      acc = fma(Rj[i], xd[i], acc);
      xi[j] = -acc * xd[j];
    }
  }
  __syncthreads();
  if (t < s) {                               // w_j = sum_{i <= j} X_ji alpha_i
    const int j = t;
    double acc = 0.0;
    for (int i = 0; i < j; i++) acc = fma(A[i * CVG_RP + j], al[i], acc);
    wv[j] = fma(xd[j], al[j], acc);
  }
  __syncthreads();
  if (t < s) {                               // e_i = sn2 sum_{j >= i} X_ji w_j,  var_i = sn2 sum_{j >= i} X_ji^2
    const int i = t;
    double e = xd[i] * wv[i], q = xd[i] * xd[i];
    for (int j = i + 1; j < s; j++) {
      const double x = A[i * CVG_RP + j];
      e = fma(x, wv[j], e);
      q = fma(x, x, q);
    }
    e *= sn2;
    q *= sn2;
    ev[i] = e;
    vv[i] = q;
    const int n = perm[o + i];
    mean[n] = y[n] - e;
    var[n] = q;
  }
  __syncthreads();
  if (t == 0) {
    double sse = 0.0, ssr = 0.0, md = 0.0, ld = 0.0;
    for (int i = 0; i < s; i++) {
      sse = fma(ev[i], ev[i], sse);
      ssr += ev[i] * ev[i] / vv[i];
      md = fma(al[i], ev[i], md);
      ld += lg[i];
    }
    gsum[3 * g] = sse;
    gsum[3 * g + 1] = ssr;
    gsum[3 * g + 2] = md;
    logp[g] = -0.5 * md - 0.5 * (s * log(sn2) - 2.0 * ld) - 0.5 * s * 1.8378770664093454836;   // log 2 pi
  }
  if (kWeights) {
    double ww = 0.0;                         // |w|^2, the same chain in every thread
    for (int j = 0; j < s; j++) ww = fma(wv[j], wv[j], ww);
    const double rs = sqrt(sn2), br = sn2 / (1.0 + sqrt(fma(sn2, ww, 1.0))) / rs;
    if (t < s) E[perm[o + t]] = ev[t];
    double *Q = Qb + qoff[g];
    for (int e = t; e < s * s; e += 256) {   // Q_ij = sqrt(sn2) X_ji + (beta / sqrt(sn2)) e_i w_j; X_ji = 0 for j < i
      const int i = e / s, j = e - i * s;
      const double x = j > i ? A[i * CVG_RP + j] : j == i ? xd[i] : 0.0;
      Q[i * CVG_MAX + j] = fma(br * ev[i], wv[j], rs * x);
    }
  }
}

// H[:, cols] <- H[:, cols] Qbin in place, cols = perm[bstart[b] .. bstart[b + 1]) the columns of bin b = blockIdx.y (at most
// CVG_MAX of them), rows the 128-row tile blockIdx.x.  Qbin is the bin's CVG_MAX x CVG_MAX matrix at Qb + b * CVG_MAX^2,
// row-major: the Q_I of its groups on the diagonal, zero elsewhere (no structural-zero skipping: the dense product is
// 2 * 128^2 flop per row and bin).  The scattered columns are each contiguous along the rows: a step of CVM_KC of them and
// the same rows of Qbin are staged in LDS by all four waves, lanes along the rows / along Qbin's columns, while the next
// step is on its way to registers.  Wave w owns the output row tiles 2 w and 2 w + 1 and all column tiles: every element
// is ONE accumulator chain over k ascending, so two calls return the same bytes.  The tile's outputs stay in registers
// until the last step has been staged -- by then every read of the tile is done, and no other workgroup touches its
// elements: in place is safe.  Columns past the bin's width are neither read nor written.
#define CVM_KC 16
__global__ __launch_bounds__(256) void gpak_cvg_mix_f64(double *H, long ld, const int *__restrict__ perm,
                                                        const int *__restrict__ bstart, const double *__restrict__ Qb) {
  __shared__ double shA[CVM_KC * CVG_PITCH], shQ[CVM_KC * CVG_PITCH];
  const int b = blockIdx.y;
  const int p0 = bstart[b], width = bstart[b + 1] - p0;
  const int nct = __builtin_amdgcn_readfirstlane((width + 15) >> 4);
  const int kend = (width + CVM_KC - 1) / CVM_KC * CVM_KC;
  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = t & 127, kh = t >> 7;        // staging: row r of the tile / column r of Qbin, steps kh * 8 .. kh * 8 + 7
  double *Hr = H + (size_t)blockIdx.x * CVG_MAX;
  const double *Q = Qb + (size_t)b * CVG_MAX * CVG_MAX;
  cvg_d4 acc[2][8];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int c = 0; c < 8; c++) acc[h][c] = (cvg_d4){0.0, 0.0, 0.0, 0.0};
  double va[8], vq[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int k = k0 + kh * 8 + u;
      const bool live = k < width;
      va[u] = live ? Hr[(size_t)r + (size_t)perm[p0 + (live ? k : 0)] * ld] : 0.0;
      vq[u] = live ? Q[(size_t)k * CVG_MAX + r] : 0.0;
    }
  };
  load(0);
  for (int k0 = 0; k0 < kend; k0 += CVM_KC) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      shA[(kh * 8 + u) * CVG_PITCH + r] = va[u];
      shQ[(kh * 8 + u) * CVG_PITCH + r] = vq[u];
    }
    __syncthreads();
    if (k0 + CVM_KC < kend) load(k0 + CVM_KC);
#pragma unroll
    for (int kq = 0; kq < CVM_KC / 4; kq++) {
      const double *ca = shA + (kq * 4 + l4) * CVG_PITCH + l15, *cq = shQ + (kq * 4 + l4) * CVG_PITCH + l15;
      const double fa0 = ca[(2 * w) * 16], fa1 = ca[(2 * w + 1) * 16];
#pragma unroll
      for (int c = 0; c < 8; c++)
        if (c < nct) {
          const double fq = cq[c * 16];
          acc[0][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fq, fa0, acc[0][c], 0, 0, 0);
          acc[1][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fq, fa1, acc[1][c], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  // lane holds of tile (rt, ct): row rt * 16 + l15, columns ct * 16 + l4 + 4 q
#pragma unroll
  for (int c = 0; c < 8; c++)
    if (c < nct)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int col = c * 16 + l4 + 4 * q;
        if (col < width) {
          double *out = Hr + (size_t)perm[p0 + col] * ld;
          out[(2 * w) * 16 + l15] = acc[0][c][q];
          out[(2 * w + 1) * 16 + l15] = acc[1][c][q];
        }
      }
}

static size_t cvg_solve_lds(int s) { return sizeof(double) * ((size_t)s * CVG_RP + 6 * CVG_MAX); }

// the substitution, the Gram pass and the solve pass of the context's last gpak_cv_groups, in ms.  Not part of the C-ABI
// (no header declares it): tools/time_cv_groups.py reads it through the shared object.
extern "C" int gpak_cv_groups_last_split(gpak_ctx *ctx, double *ms3) {
  if (!ctx || !ms3 || ctx->multi) return GPAK_EINVAL;
  for (int k = 0; k < 3; k++) ms3[k] = ctx->cvg_ms[k];
  return GPAK_OK;
}

// The two passes on device lists, on the context's stream (gpak_cv_folds runs them on its groups of at most CVG_MAX
// samples): perm / offs / soff as the kernels take them, soff[g + 1] - soff[g] = gpak_cvg_s_elems(size of group g)
long long gpak_cvg_s_elems(int s) { return (long long)cvg_pad16(s) * cvg_pad16(s); }
// The launches themselves, on explicit arguments: what the context's calls and the entries of gpak_dev_cv_kernels.h both run
static void cvg_gram_on(hipStream_t st, const double *G, long ld, int Np, int n_groups, const int *dperm, const int *doffs,
                        const long long *dsoff, double *dS) {
  hipLaunchKernelGGL(gpak_cvg_gram_f64, dim3(n_groups), dim3(256), 0, st, G, ld, Np, dperm, doffs, dsoff, dS);
}
template <bool kWeights>
static void cvg_solve_on(hipStream_t st, int device, const double *y, const double *alpha, double sn2, int n_groups,
                         int max_size, const double *dS, const long long *dsoff, const int *dperm, const int *doffs,
                         double *dmean, double *dvar, double *dlogp, double *dgsum, int *dinfo, double *dE, double *dQb,
                         const long long *dqoff) {
  // more than 64 KiB of dynamic LDS needs the opt-in, once per kernel and per device
  {
    static std::atomic<unsigned long long> done_mask{0};
    const unsigned long long bit = 1ull << (device & 63);
    if (!(done_mask.load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gpak_cvg_solve_f64<kWeights>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)cvg_solve_lds(CVG_MAX));
      done_mask.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(gpak_cvg_solve_f64<kWeights>, dim3(n_groups), dim3(256), cvg_solve_lds(max_size), st, dS, dsoff, dperm,
                     doffs, y, alpha, sn2, dmean, dvar, dlogp, dgsum, dinfo, dE, dQb, dqoff);
}
static void cvg_mix_on(hipStream_t st, double *H, long ld, int Np, int n_bins, const int *dperm, const int *dbstart,
                       const double *dQb) {
  hipLaunchKernelGGL(gpak_cvg_mix_f64, dim3(Np / CVG_MAX, n_bins), dim3(256), 0, st, H, ld, dperm, dbstart, dQb);
}
void gpak_cvg_launch_gram(gpak_ctx *ctx, const double *G, long ld, int n_groups, const int *dperm, const int *doffs,
                          const long long *dsoff, double *dS) {
  cvg_gram_on(ctx->stream, G, ld, ctx->Np, n_groups, dperm, doffs, dsoff, dS);
}
void gpak_cvg_launch_solve(gpak_ctx *ctx, int n_groups, int max_size, const double *dS, const long long *dsoff,
                           const int *dperm, const int *doffs, double *dmean, double *dvar, double *dlogp, double *dgsum,
                           int *dinfo) {
  cvg_solve_on<false>(ctx->stream, ctx->device, ctx->dy, ctx->dAlpha, ctx->sn2, n_groups, max_size, dS, dsoff, dperm, doffs,
                      dmean, dvar, dlogp, dgsum, dinfo, nullptr, nullptr, nullptr);
}
void gpak_cvg_launch_solve_weights(gpak_ctx *ctx, int n_groups, int max_size, const double *dS, const long long *dsoff,
                                   const int *dperm, const int *doffs, double *dmean, double *dvar, double *dlogp,
                                   double *dgsum, int *dinfo, double *dE, double *dQb, const long long *dqoff) {
  cvg_solve_on<true>(ctx->stream, ctx->device, ctx->dy, ctx->dAlpha, ctx->sn2, n_groups, max_size, dS, dsoff, dperm, doffs,
                     dmean, dvar, dlogp, dgsum, dinfo, dE, dQb, dqoff);
}
void gpak_cvg_launch_mix(gpak_ctx *ctx, double *H, long ld, int n_bins, const int *dperm, const int *dbstart, const double *dQb) {
  cvg_mix_on(ctx->stream, H, ld, ctx->Np, n_bins, dperm, dbstart, dQb);
}

// ---- include/gpak_dev_cv_kernels.h: the three kernels alone on caller-owned device buffers ---------------------------
static int cvg_status() { return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP; }

extern "C" int gpak_dev_cvg_gram(void *stream, const double *G, long ld, int Np, const int *perm, const int *offs,
                                 int n_groups, const long long *soff, double *S) {
  if (!G || !perm || !offs || !soff || !S || n_groups < 1 || Np < CVG_MAX || Np % CVG_MAX || ld < Np) return GPAK_EINVAL;
  cvg_gram_on((hipStream_t)stream, G, ld, Np, n_groups, perm, offs, soff, S);
  return cvg_status();
}

extern "C" int gpak_dev_cvg_solve(void *stream, const double *S, const long long *soff, const int *perm, const int *offs,
                                  int n_groups, int max_size, const double *y, const double *alpha, double sn2,
                                  double *mean, double *var, double *logp, double *gsum, int *info, double *E, double *Qb,
                                  const long long *qoff) {
  const int n_w = (E != nullptr) + (Qb != nullptr) + (qoff != nullptr);
  if (!S || !soff || !perm || !offs || !y || !alpha || !mean || !var || !logp || !gsum || !info || n_groups < 1 ||
      max_size < 1 || max_size > CVG_MAX || !(sn2 > 0.0) || (n_w != 0 && n_w != 3))
    return GPAK_EINVAL;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return GPAK_EHIP;
  if (n_w)
    cvg_solve_on<true>((hipStream_t)stream, device, y, alpha, sn2, n_groups, max_size, S, soff, perm, offs, mean, var, logp,
                       gsum, info, E, Qb, qoff);
  else
    cvg_solve_on<false>((hipStream_t)stream, device, y, alpha, sn2, n_groups, max_size, S, soff, perm, offs, mean, var, logp,
                        gsum, info, nullptr, nullptr, nullptr);
  return cvg_status();
}

extern "C" int gpak_dev_cvg_mix(void *stream, double *H, long ld, int Np, const int *perm, const int *bstart, int n_bins,
                                const double *Qb) {
  if (!H || !perm || !bstart || !Qb || n_bins < 1 || Np < CVG_MAX || Np % CVG_MAX || ld < Np) return GPAK_EINVAL;
  cvg_mix_on((hipStream_t)stream, H, ld, Np, n_bins, perm, bstart, Qb);
  return cvg_status();
}

// The bins of the column mix: consecutive groups of the (group, sample) order packed greedily into bins of at most
// CVG_MAX columns -- a group opens a new bin when it does not fit the current one, so two adjacent bins hold more than
// CVG_MAX columns together and there are at most 2 N / CVG_MAX + 1 of them.  first[b] = the first group of bin b,
// first[n_bins] = n_groups (room for n_groups + 1 entries); returns n_bins.  sizes: every one in [1, CVG_MAX].  Not part
// of the C-ABI (no header declares it): tests/test_cv_groups_grad.py holds it to these properties.
extern "C" int gpak_cvg_pack_bins(const int *sizes, int n_groups, int *first) {
  int nb = 0, fill = 0;
  for (int g = 0; g < n_groups; g++) {
    if (g == 0 || fill + sizes[g] > CVG_MAX) { first[nb++] = g; fill = 0; }
    fill += sizes[g];
  }
  first[nb] = n_groups;
  return nb;
}

// gpak_cv_groups on a single-GPU context whose factor and alpha are current, the labels already checked (api.hip):
// perm = the samples sorted by (group, sample), offs = where each group starts in it (n_groups + 1 entries)
int gpak_cv_groups_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *mean, double *var,
                        double *group_logp, gpak_cv_groups_summary *summary) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np;
  const long ld = ctx->ld;
  // where G goes: the gradient's workspace once it exists, otherwise the leave-one-out buffer grown to the whole matrix.
  // (dG is never allocated alone: grad_binv takes dG != NULL to mean that dBinv exists too.)
  double *G = ctx->dG;
  if (!G) {
    if (!gpak_loo_workspace(ctx, (size_t)ld * Np)) {
      ctx->err = "device allocation failed for the leave-group-out workspace (L^-T as one N x N matrix)";
      return GPAK_ENOMEM;
    }
    G = ctx->dLoo;
  }
  // scratch in the gradient's partial-sum buffer: the S of every group, mean, var (N each), logp (n_groups), the groups'
  // three sums; then the index lists
  std::vector<long long> soff((size_t)n_groups + 1);
  int max_size = 0;
  soff[0] = 0;
  for (int g = 0; g < n_groups; g++) {
    const int s = offs[g + 1] - offs[g], sp = cvg_pad16(s);
    max_size = std::max(max_size, s);
    soff[g + 1] = soff[g] + (long long)sp * sp;
  }
  const size_t nS = (size_t)soff[n_groups], nG = (size_t)n_groups;
  const size_t n_dbl = nS + 2 * (size_t)N + 4 * nG;
  const size_t n_ll = nG + 1, n_int = (size_t)N + nG + 1 + 1;
  int rc = gpak_grad_scratch(ctx, n_dbl + n_ll + (n_int + 1) / 2);
  if (rc) return rc;
  double *dS = ctx->dGpart, *dmean = dS + nS, *dvar = dmean + N, *dlogp = dvar + N, *dgsum = dlogp + nG;
  long long *dsoff = reinterpret_cast<long long *>(dgsum + 3 * nG);
  int *dperm = reinterpret_cast<int *>(dsoff + n_ll), *doffs = dperm + N, *dinfo = doffs + nG + 1;
  const int info0 = INT_MAX;
  GPAK_HIP(hipMemcpyAsync(dsoff, soff.data(), sizeof(long long) * n_ll, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dperm, perm, sizeof(int) * N, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(doffs, offs, sizeof(int) * (nG + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dinfo, &info0, sizeof(int), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipEventRecord(ctx->ev[7], st));
  gpak_grad_g_full(ctx, G, ld);
  GPAK_HIP(hipEventRecord(ctx->ev[5], st));
  gpak_cvg_launch_gram(ctx, G, ld, n_groups, dperm, doffs, dsoff, dS);
  GPAK_HIP(hipEventRecord(ctx->ev[6], st));
  gpak_cvg_launch_solve(ctx, n_groups, max_size, dS, dsoff, dperm, doffs, dmean, dvar, dlogp, dgsum, dinfo);
  GPAK_HIP(hipEventRecord(ctx->ev[9], st));
  std::vector<double> hsum(4 * nG), hmean, hvar;   // logp, then the three sums per group
  int info = 0;
  GPAK_HIP(hipMemcpyAsync(hsum.data(), dlogp, sizeof(double) * 4 * nG, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, st));
  if (mean) GPAK_HIP(hipMemcpyAsync(mean, dmean, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (var) GPAK_HIP(hipMemcpyAsync(var, dvar, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipStreamSynchronize(st));
  GPAK_HIP(hipGetLastError());
  float ms = 0, part[3] = {0, 0, 0};
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[9]));
  GPAK_HIP(hipEventElapsedTime(&part[0], ctx->ev[7], ctx->ev[5]));
  GPAK_HIP(hipEventElapsedTime(&part[1], ctx->ev[5], ctx->ev[6]));
  GPAK_HIP(hipEventElapsedTime(&part[2], ctx->ev[6], ctx->ev[9]));
  for (int k = 0; k < 3; k++) ctx->cvg_ms[k] = part[k];
  if (group_logp)
    for (size_t g = 0; g < nG; g++) group_logp[g] = hsum[g];
  if (summary) {
    double sse = 0.0, ssr = 0.0, md = 0.0, lp = 0.0;
    for (size_t g = 0; g < nG; g++) {   // ascending: a fixed order
      lp += hsum[g];
      sse += hsum[nG + 3 * g];
      ssr += hsum[nG + 3 * g + 1];
      md += hsum[nG + 3 * g + 2];
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
    ctx->err = "gpak_cv_groups: S = [B^-1]_II of group " + std::to_string(info - 1) + " is not positive definite";
    return GPAK_ENOTPD;
  }
  return GPAK_OK;
}
