// cv_folds.hip -- k-fold cross-validation from the Cholesky factor on gfx950 (gpak_cv_folds): gpak_cv_groups for groups
// of any size.
//
// The mathematics is that of cv_groups.hip.  With G = L^-T as one matrix and alpha = Ky^-1 y, for a group with index set
// I of m samples:  S = G_I G_I^T = R R^T,  T = R^-T,  w = T^T alpha_I,  e_I = sn2 T w,  var_i = sn2 sum_{j >= i} T_ij^2.
// On the context's stream, one host synchronisation at the end:
//   1. G: gpak_grad_g_full, into dG when the gradient owns one, else into dLoo (exactly as gpak_cv_groups_impl);
//   2. the groups of at most GPAK_CV_GROUP_MAX samples: the two batched kernels of cv_groups.hip on compacted lists, one
//      launch each -- a labelling without a larger group gives the bytes of gpak_cv_groups;
//   3. every other group alone, in ascending group number, in workspaces sized by the largest of them:
//        gpak_cvf_pack_f64      P = the group's rows of G from the 128-tile k0 of its smallest row on, zero rows up to
//                               m_p = m rounded up to 128
//        gpak_launch_gemm_nt    S = P P^T on the lower 128-tiles (K = Np - k0, beta = 0): the N^3 / k product
//        gpak_cvf_pad_f64       the padding of S becomes the identity
//        gpak_factor_panel      R, 512 columns at a time with the K = W update to their right; inverse blocks and an
//                               info word of the group's own
//        gpak_grad_g_of         T = R^-T, over P
//        gpak_cvf_w_f64, gpak_cvf_ev_f64, gpak_cvf_sums_f64   w; e, var, mean; log det R and the group's three sums
// Orders of summation.  S_ij: one accumulator chain of the product's tile over k ascending from k0; the kernel the
// launcher picks depends on (m_p, Np - k0) and the process-wide tuning alone.  w_j: thread t of 256 adds rows t, t + 256,
// ... ascending, then a fixed tree.  e_i, var_i: four chains over the columns j = q (mod 4), j ascending, combined as
// (0 + 1) + (2 + 3).  The group's sums: thread t adds i = t, t + 256, ..., then a fixed tree.  Every one of them is a
// function of the group's member set and the factor: not of the other groups, the label numbering, the grid or the
// buffer that holds G.
// gpak_cv_folds_grad (grad.hip) runs the same groups through the same functions of this file and takes from it, per
// one-at-a-time group, the weight factor Q_I (gpak_cvf_q_f64) and the column mix H[:, I] <- H[:, I] Q_I (gpak_cvf_mix_f64).
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/gpak_cv_folds.h"
#include "../../include/gpak_dev_cv.h"
#include "../../include/gpak_dev_cv_kernels.h"
#include "../../include/gpak_dev_cv_mix.h"
#include "gpak_internal.h"

#define CVF_TB 128        // the product's tile
#define CVF_PACK_COLS 32  // columns of P per workgroup of the pack: 8 per wave, all in flight at once

static int cvf_pad128(int m) { return (m + CVF_TB - 1) / CVF_TB * CVF_TB; }

// P[r, c] = G[rows[r], k0 + c] for r < m and 0 for m <= r < m_p, c < ncols.  Workgroup (x, y): rows 128 x .. 128 x + 127,
// columns 32 y .. 32 y + 31.  Lanes run along r, two rows each: a wave stores 1 KiB contiguous per column (16 B per lane
// when VEC: P 16-byte aligned and ldp even) and reads its 128 rows of one column of G -- 1 KiB contiguous where the
// members are consecutive samples, one 8-byte word per 128-byte line where they are scattered.  Wave w takes the columns
// w, w + 4, ... of the 32; its 8 loads per row are issued before the first store.
template <bool VEC>
__global__ __launch_bounds__(256) void gpak_cvf_pack_f64(const double *__restrict__ G, long ld, const int *__restrict__ rows,
                                                         int m, int k0, int ncols, double *__restrict__ P, long ldp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = blockIdx.x * CVF_TB + 2 * lane;          // < m_p: the grid has m_p / 128 workgroups along x
  const bool la = r0 < m, lb = r0 + 1 < m;
  const double *ga = G + (size_t)k0 * ld + (la ? rows[r0] : 0);
  const double *gb = G + (size_t)k0 * ld + (lb ? rows[r0 + 1] : 0);
  const int c0 = blockIdx.y * CVF_PACK_COLS + w;
  double a[CVF_PACK_COLS / 4], b[CVF_PACK_COLS / 4];
#pragma unroll
  for (int u = 0; u < CVF_PACK_COLS / 4; u++) {
    const int c = c0 + 4 * u;
    const bool in = c < ncols;
    a[u] = (in && la) ? ga[(size_t)c * ld] : 0.0;
    b[u] = (in && lb) ? gb[(size_t)c * ld] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < CVF_PACK_COLS / 4; u++) {
    const int c = c0 + 4 * u;
    if (c >= ncols) continue;
    double *p = P + (size_t)c * ldp + r0;
    if (VEC) {
      *reinterpret_cast<double2 *>(p) = make_double2(a[u], b[u]);
    } else {
      p[0] = a[u];
      p[1] = b[u];
    }
  }
}

void gpak_launch_pack_rows(hipStream_t st, const double *G, long ld, int Np, const int *rows, int m, int k0, double *P,
                           long ldp) {
  const int mp = cvf_pad128(m), ncols = Np - k0;
  const dim3 grid(mp / CVF_TB, (ncols + CVF_PACK_COLS - 1) / CVF_PACK_COLS);
  const bool vec = (reinterpret_cast<size_t>(P) & 15) == 0 && (ldp & 1) == 0;
  if (vec) hipLaunchKernelGGL(gpak_cvf_pack_f64<true>, grid, dim3(256), 0, st, G, ld, rows, m, k0, ncols, P, ldp);
  else hipLaunchKernelGGL(gpak_cvf_pack_f64<false>, grid, dim3(256), 0, st, G, ld, rows, m, k0, ncols, P, ldp);
}

extern "C" int gpak_dev_pack_rows(void *stream, const double *G, long ld, int Np, const int *rows, int m, int k0, double *P,
                                  long ldp) {
  if (!G || !rows || !P || m < 1 || m > Np || k0 < 0 || k0 >= Np || ld < Np || ldp < cvf_pad128(m)) return GPAK_EINVAL;
  gpak_launch_pack_rows((hipStream_t)stream, G, ld, Np, rows, m, k0, P, ldp);
  return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP;
}

// rows and columns m .. mp - 1 of the lower triangle of S become the identity (the product left zeros there: the rows of
// P beyond m are zero), so that the factorisation runs over whole tiles and a padded column is never a failing pivot
__global__ __launch_bounds__(256) void gpak_cvf_pad_f64(double *__restrict__ S, long lds, int m, int mp) {
  const int np = mp - m;                                   // < 128
  for (int e = threadIdx.x; e < np * np; e += 256) {
    const int i = m + e % np, j = m + e / np;
    if (i >= j) S[(size_t)i + (size_t)j * lds] = i == j ? 1.0 : 0.0;
  }
}
// the launches of the stage kernels on explicit arguments: what gpak_cvf_run_group / the column mix and the entries of
// gpak_dev_cv_kernels.h both run
static void cvf_launch_pad(hipStream_t st, double *S, long lds, int m) {
  const int mp = cvf_pad128(m);
  if (mp == m) return;   // nothing to pad
  hipLaunchKernelGGL(gpak_cvf_pad_f64, dim3(1), dim3(256), 0, st, S, lds, m, mp);
}

// w_j = sum_{i <= j} T_ij alpha_I,i: workgroup j.  Thread t adds the rows t, t + 256, ... in ascending order, then the tree.
__global__ __launch_bounds__(256) void gpak_cvf_w_f64(const double *__restrict__ T, long ldt, const int *__restrict__ rows,
                                                      const double *__restrict__ alpha, double *__restrict__ wv) {
  __shared__ double red[256];
  const int j = blockIdx.x, t = threadIdx.x;
  const double *col = T + (size_t)j * ldt;
  double s = 0.0;
  for (int i = t; i <= j; i += 256) s = fma(col[i], alpha[rows[i]], s);
  red[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) wv[j] = red[0];
}
static void cvf_launch_w(hipStream_t st, const double *T, long ldt, int m, const int *rows, const double *alpha, double *wv) {
  hipLaunchKernelGGL(gpak_cvf_w_f64, dim3(m), dim3(256), 0, st, T, ldt, rows, alpha, wv);
}

// e_i = sn2 sum_{j >= i} T_ij w_j and var_i = sn2 sum_{j >= i} T_ij^2 in one pass over the upper triangle of T, then
// mean and var through the group's rows.  Workgroup: 64 rows (the lanes: a wave reads 512 contiguous bytes of a column),
// wave q the columns j = q (mod 4) in ascending order; the four chains are added as (0 + 1) + (2 + 3).  A group whose
// factorisation failed (info) gets NaN.
__global__ __launch_bounds__(256) void gpak_cvf_ev_f64(const double *__restrict__ T, long ldt, int m,
                                                       const double *__restrict__ wv, const int *__restrict__ rows,
                                                       const double *__restrict__ y, double sn2, const int *__restrict__ info,
                                                       double *__restrict__ ev, double *__restrict__ vv,
                                                       double *__restrict__ mean, double *__restrict__ var) {
  __shared__ double re[4][64], rv[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 64, i = i0 + lane;
  const bool live = i < m;
  double e = 0.0, v = 0.0;
  if (live) {
    const double *row = T + i;
#pragma unroll 4
    for (int j = i0 + q; j < m; j += 4) {
      const double x = j >= i ? row[(size_t)j * ldt] : 0.0;
      e = fma(x, wv[j], e);
      v = fma(x, x, v);
    }
  }
  re[q][lane] = e;
  rv[q][lane] = v;
  __syncthreads();
  if (q == 0 && live) {
    e = sn2 * ((re[0][lane] + re[1][lane]) + (re[2][lane] + re[3][lane]));
    v = sn2 * ((rv[0][lane] + rv[1][lane]) + (rv[2][lane] + rv[3][lane]));
    if (*info != INT_MAX) e = v = __longlong_as_double(0x7ff8000000000000LL);
    ev[i] = e;
    vv[i] = v;
    const int n = rows[i];
    mean[n] = y[n] - e;
    var[n] = v;
  }
}
static void cvf_launch_ev(hipStream_t st, const double *T, long ldt, int m, const double *wv, const int *rows, const double *y,
                          double sn2, const int *info, double *ev, double *vv, double *mean, double *var) {
  hipLaunchKernelGGL(gpak_cvf_ev_f64, dim3((m + 63) / 64), dim3(256), 0, st, T, ldt, m, wv, rows, y, sn2, info, ev, vv, mean, var);
}

// one workgroup: gsum[0..2] = sum e_i^2, sum e_i^2 / var_i, alpha_I . e_I and logp from those and sum log R_ii.  Thread t
// adds i = t, t + 256, ... in ascending order, then the tree.
__global__ __launch_bounds__(256) void gpak_cvf_sums_f64(const double *__restrict__ R, long ldr, int m,
                                                         const double *__restrict__ ev, const double *__restrict__ vv,
                                                         const int *__restrict__ rows, const double *__restrict__ alpha,
                                                         double sn2, const int *__restrict__ info, double *__restrict__ logp,
                                                         double *__restrict__ gsum) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  double sse = 0.0, ssr = 0.0, md = 0.0, ld = 0.0;
  for (int i = t; i < m; i += 256) {
    const double e = ev[i];
    sse = fma(e, e, sse);
    ssr += e * e / vv[i];
    md = fma(alpha[rows[i]], e, md);
    ld += log(R[(size_t)i + (size_t)i * ldr]);
  }
  red[0][t] = sse; red[1][t] = ssr; red[2][t] = md; red[3][t] = ld;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h)
#pragma unroll
      for (int k = 0; k < 4; k++) red[k][t] += red[k][t + h];
    __syncthreads();
  }
  if (t == 0) {
    const bool bad = *info != INT_MAX;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    gsum[0] = bad ? nan : red[0][0];
    gsum[1] = bad ? nan : red[1][0];
    gsum[2] = bad ? nan : red[2][0];
    logp[0] = bad ? nan : -0.5 * red[2][0] - 0.5 * (m * log(sn2) - 2.0 * red[3][0]) - 0.5 * m * 1.8378770664093454836;   // log 2 pi
  }
}
static void cvf_launch_sums(hipStream_t st, const double *R, long ldr, int m, const double *ev, const double *vv, const int *rows,
                            const double *alpha, double sn2, const int *info, double *logp, double *gsum) {
  hipLaunchKernelGGL(gpak_cvf_sums_f64, dim3(1), dim3(256), 0, st, R, ldr, m, ev, vv, rows, alpha, sn2, info, logp, gsum);
}

// the substitution, the batched small groups, and pack / product / factor + inverse + finish summed over the other groups
// of the context's last gpak_cv_folds, in ms.  Not part of the C-ABI (no header declares it): tools/time_cv_folds.py
// reads it through the shared object.
extern "C" int gpak_cv_folds_last_split(gpak_ctx *ctx, double *ms5) {
  if (!ctx || !ms5 || ctx->multi) return GPAK_EINVAL;
  for (int k = 0; k < 5; k++) ms5[k] = ctx->cvf_ms[k];
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// What gpak_cv_folds_grad (grad.hip) needs of a one-at-a-time group beyond its outputs: the weight factor of the gradient,
//   Q_I = sqrt(sn2) T + (beta / sqrt(sn2)) e_I w^T,   beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)),   Q_I Q_I^T = sn2 S^-1 + e_I e_I^T
// (the closed form of cv_groups.hip: T = R^-T is its X^T), and the column mix H[:, I] <- H[:, I] Q_I for a group wider
// than one bin of gpak_cvg_mix_f64.
// ---------------------------------------------------------------------------------------
// sc[0] = sqrt(sn2), sc[1] = beta / sqrt(sn2).  |w|^2: thread t adds j = t, t + 256, ... in ascending order, then the tree.
__global__ __launch_bounds__(256) void gpak_cvf_beta_f64(const double *__restrict__ wv, int m, double sn2, double *__restrict__ sc) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int j = t; j < m; j += 256) s = fma(wv[j], wv[j], s);
  red[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) {
    const double rs = sqrt(sn2);
    sc[0] = rs;
    sc[1] = sn2 / (1.0 + sqrt(fma(sn2, red[0], 1.0))) / rs;
  }
}
static void cvf_launch_beta(hipStream_t st, const double *wv, int m, double sn2, double *sc) {
  hipLaunchKernelGGL(gpak_cvf_beta_f64, dim3(1), dim3(256), 0, st, wv, m, sn2, sc);
}

// Q[i, j] = sc[0] T_ij + sc[1] e_i w_j for i, j < m (T_ij = 0 for j < i) and 0 on the rest of m_p x m_p, column-major with
// leading dimension ldq -- or, TRANSPOSED, Q^T so stored: the B operand of the GEMM that mixes a wide group; e_I scattered
// into E.  Workgroup (x, y): rows 128 x .. 128 x + 127, columns 16 y .. 16 y + 15.
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void gpak_cvf_q_f64(const double *__restrict__ T, long ldt, int m, const double *__restrict__ wv,
                                                      const double *__restrict__ ev, const double *__restrict__ sc,
                                                      const int *__restrict__ rows, double *__restrict__ Q, long ldq,
                                                      double *__restrict__ E) {
  const int i = blockIdx.x * CVF_TB + (threadIdx.x & 127), jh = threadIdx.x >> 7;
  const double rs = sc[0], br = sc[1];
  const bool live = i < m;
  const double be = live ? br * ev[i] : 0.0;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int j = blockIdx.y * 16 + jh + 2 * u;
    double q = 0.0;
    if (live && j < m) q = fma(be, wv[j], rs * (j >= i ? T[(size_t)i + (size_t)j * ldt] : 0.0));
    Q[TRANSPOSED ? (size_t)j + (size_t)i * ldq : (size_t)i + (size_t)j * ldq] = q;
  }
  if (blockIdx.y == 0 && jh == 0 && live) E[rows[i]] = ev[i];
}
static void cvf_launch_q(hipStream_t st, bool transposed, const double *T, long ldt, int m, const double *wv, const double *ev,
                         const double *sc, const int *rows, double *Q, long ldq, double *E) {
  const int mp = cvf_pad128(m);
  const dim3 grid(mp / CVF_TB, mp / 16);
  if (transposed) hipLaunchKernelGGL(gpak_cvf_q_f64<true>, grid, dim3(256), 0, st, T, ldt, m, wv, ev, sc, rows, Q, ldq, E);
  else hipLaunchKernelGGL(gpak_cvf_q_f64<false>, grid, dim3(256), 0, st, T, ldt, m, wv, ev, sc, rows, Q, ldq, E);
}

// Z[:, c] = sum_{k < m} H[:, cols[k]] Q[k, c] for c < m: the mix for a column set of any width, out of place (block column J
// of the result would overwrite columns that block J' still reads).  Workgroup (x, y): the 128 x 128 tile of Z at rows
// 128 x, columns 128 y.  Wave w owns the row tiles 2 w and 2 w + 1 of 16 and all eight column tiles.  The gathered columns
// of H are each contiguous along the rows, and the MFMA's H operand wants, per k-step of 4, rows l15 of the columns
// k + l4: a lane loads its own operand words from H + cols[k] * ld -- 128 contiguous bytes per 16 lanes, no pack pass and
// no LDS round trip.  A step of CVX_KC rows of Q (what all four waves share) is staged in one of two LDS buffers, lanes
// along k (contiguous in the column-major Q); the operand words and the rows of Q of the next step, and the indices of the
// one after, are on their way to registers while a step's MFMAs run.  Every element of Z is ONE accumulator chain over k
// ascending: two calls return the same bytes.  Rows k >= m and columns c >= m of Q are not read, columns c >= m and rows
// >= Np of Z not written.
#define CVX_KC 16
#define CVX_PITCH 144   // doubles per staged row of Q: 288 dwords = 32 (mod 64), the MFMA reads of a wave are conflict-free
typedef double cvf_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void gpak_cvf_mix_f64(const double *__restrict__ H, long ld, int Np, const int *__restrict__ cols,
                                                        int m, const double *__restrict__ Q, long ldq, double *__restrict__ Z,
                                                        long ldz) {
  __shared__ double shQ[2][CVX_KC * CVX_PITCH];
  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int c0 = blockIdx.y * CVF_TB;
  const int ncol = min(CVF_TB, m - c0);                  // >= 1: the grid has ceil(m / 128) workgroups along y
  const int nct = __builtin_amdgcn_readfirstlane((ncol + 15) >> 4);
  const int ra = blockIdx.x * CVF_TB + (2 * w) * 16 + l15, rb = ra + 16;
  const bool la = ra < Np, lb = rb < Np;
  const int sk = t & 15, sc = t >> 4;                    // staging: row k0 + sk of Q, columns sc, sc + 16, ...
  const int kend = (m + CVX_KC - 1) / CVX_KC * CVX_KC;
  cvf_d4 acc[2][8];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int c = 0; c < 8; c++) acc[h][c] = (cvf_d4){0.0, 0.0, 0.0, 0.0};
  int ix[CVX_KC / 4];
  double va[CVX_KC / 4], vb[CVX_KC / 4], vq[8];
  auto load_idx = [&](int k0) {
#pragma unroll
    for (int kq = 0; kq < CVX_KC / 4; kq++) {
      const int k = k0 + kq * 4 + l4;
      ix[kq] = k < m ? cols[k] : -1;
    }
  };
  auto load = [&](int k0) {
#pragma unroll
    for (int kq = 0; kq < CVX_KC / 4; kq++) {
      const bool live = ix[kq] >= 0;
      const double *col = H + (size_t)(live ? ix[kq] : 0) * ld;
      va[kq] = (live && la) ? col[ra] : 0.0;
      vb[kq] = (live && lb) ? col[rb] : 0.0;
    }
    const int k = k0 + sk;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int c = sc + 16 * u;
      vq[u] = (k < m && c < ncol) ? Q[(size_t)k + (size_t)(c0 + c) * ldq] : 0.0;
    }
  };
  load_idx(0);
  load(0);
  load_idx(CVX_KC);
  int buf = 0;
  for (int k0 = 0; k0 < kend; k0 += CVX_KC) {
    double *sq = shQ[buf];
    double fa[CVX_KC / 4], fb[CVX_KC / 4];
#pragma unroll
    for (int u = 0; u < 8; u++) sq[sk * CVX_PITCH + sc + 16 * u] = vq[u];
#pragma unroll
    for (int kq = 0; kq < CVX_KC / 4; kq++) { fa[kq] = va[kq]; fb[kq] = vb[kq]; }
    __syncthreads();   // one per step: the other buffer was last read before this barrier
    if (k0 + CVX_KC < kend) {
      load(k0 + CVX_KC);
      load_idx(k0 + 2 * CVX_KC);
    }
#pragma unroll
    for (int kq = 0; kq < CVX_KC / 4; kq++) {
      const double *cq = sq + (kq * 4 + l4) * CVX_PITCH + l15;
#pragma unroll
      for (int c = 0; c < 8; c++)
        if (c < nct) {
          const double fq = cq[c * 16];
          acc[0][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fq, fa[kq], acc[0][c], 0, 0, 0);
          acc[1][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fq, fb[kq], acc[1][c], 0, 0, 0);
        }
    }
    buf ^= 1;
  }
  // lane holds of tile (rt, ct): row rt * 16 + l15, columns ct * 16 + l4 + 4 q
#pragma unroll
  for (int c = 0; c < 8; c++)
    if (c < nct)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int col = c * 16 + l4 + 4 * q;
        if (col < ncol) {
          double *out = Z + (size_t)(c0 + col) * ldz;
          if (la) out[ra] = acc[0][c][q];
          if (lb) out[rb] = acc[1][c][q];
        }
      }
}

// H[:, cols[c]] = Z[:, c]: workgroup (c, x) the rows 512 x .. of column c, two rows per lane
__global__ __launch_bounds__(256) void gpak_cvf_unmix_f64(double *__restrict__ H, long ld, int Np, const int *__restrict__ cols,
                                                          const double *__restrict__ Z, long ldz) {
  const int c = blockIdx.x;
  double *h = H + (size_t)cols[c] * ld;
  const double *z = Z + (size_t)c * ldz;
  for (int r = blockIdx.y * 512 + threadIdx.x; r < min(Np, (int)(blockIdx.y + 1) * 512); r += 256) h[r] = z[r];
}
static void cvf_launch_unmix(hipStream_t st, double *H, long ld, int Np, const int *cols, int m, const double *Z, long ldz) {
  hipLaunchKernelGGL(gpak_cvf_unmix_f64, dim3(m, (Np + 511) / 512), dim3(256), 0, st, H, ld, Np, cols, Z, ldz);
}

// the product, then -- stream-ordered behind every workgroup of it -- the write-back
void gpak_launch_mix_cols(hipStream_t st, double *H, long ld, int Np, const int *cols, int m, const double *Q, long ldq,
                          double *Z, long ldz) {
  hipLaunchKernelGGL(gpak_cvf_mix_f64, dim3((Np + CVF_TB - 1) / CVF_TB, (m + CVF_TB - 1) / CVF_TB), dim3(256), 0, st, H, ld, Np,
                     cols, m, Q, ldq, Z, ldz);
  cvf_launch_unmix(st, H, ld, Np, cols, m, Z, ldz);
}

// The same mix from existing parts, for a group wide enough that the bulk GEMM's rate pays for two more passes over the
// columns (DESIGN.md section 4.4 has the measurements): A[:, c] = H[:, cols[c]] for c < m and 0 up to m_p; Cw = A Qt^T by
// gpak_launch_gemm_nt (K = m_p: Qt is Q^T, zero outside m x m); H[:, cols[c]] = Cw[:, c].  Np a multiple of 128; A and Cw
// Np x m_p each, leading dimension Np.
__global__ __launch_bounds__(256) void gpak_cvf_gather_f64(const double *__restrict__ H, long ld, int Np, const int *__restrict__ cols,
                                                           int m, double *__restrict__ A, long lda) {
  const int c = blockIdx.x;
  const double *h = c < m ? H + (size_t)cols[c] * ld : nullptr;
  double *a = A + (size_t)c * lda;
  for (int r = blockIdx.y * 512 + threadIdx.x; r < min(Np, (int)(blockIdx.y + 1) * 512); r += 256) a[r] = h ? h[r] : 0.0;
}
static void cvf_launch_gather(hipStream_t st, const double *H, long ld, int Np, const int *cols, int m, double *A, long lda) {
  hipLaunchKernelGGL(gpak_cvf_gather_f64, dim3(cvf_pad128(m), (Np + 511) / 512), dim3(256), 0, st, H, ld, Np, cols, m, A, lda);
}

static void cvf_mix_cols_gemm(hipStream_t st, double *H, long ld, int Np, const int *cols, int m, const double *Qt, long ldq,
                              double *A, double *Cw) {
  const int mp = cvf_pad128(m);
  cvf_launch_gather(st, H, ld, Np, cols, m, A, (long)Np);
  gpak_launch_gemm_nt(st, Np / CVF_TB, mp / CVF_TB, mp, 1.0, A, (long)Np, Qt, ldq, 0.0, Cw, (long)Np, 0, 0, false, false);
  cvf_launch_unmix(st, H, ld, Np, cols, m, Cw, (long)Np);
}

// which of the two a one-at-a-time group of m samples takes: measured, the fused kernel is ahead up
// to two column tiles at N = 32768 and the composition from there on, by a third for a fold of N / 10
static bool cvf_mix_by_gemm(int m) { return cvf_pad128(m) > 2 * CVF_TB; }

void gpak_cvf_mix_group(gpak_ctx *ctx, const gpak_cvf_plan &pl, size_t k, const int *cols, int m) {
  const int Np = ctx->Np, mp = cvf_pad128(m);
  double *Q = ctx->dCvfQ + pl.qoff[k], *W = ctx->dCvfP;
  if (cvf_mix_by_gemm(m)) cvf_mix_cols_gemm(ctx->stream, ctx->dG, ctx->ld, Np, cols, m, Q, (long)mp, W, W + (size_t)Np * pl.mp_max);
  else gpak_launch_mix_cols(ctx->stream, ctx->dG, ctx->ld, Np, cols, m, Q, (long)mp, W, (long)Np);
}

extern "C" int gpak_dev_mix_cols(void *stream, double *H, long ld, int Np, const int *cols, int m, const double *Q, long ldq,
                                 double *Z, long ldz) {
  if (!H || !cols || !Q || !Z || m < 1 || m > Np || ld < Np || ldq < m || ldz < Np) return GPAK_EINVAL;
  gpak_launch_mix_cols((hipStream_t)stream, H, ld, Np, cols, m, Q, ldq, Z, ldz);
  return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP;
}

// ---- include/gpak_dev_cv_kernels.h: the stage kernels of a one-at-a-time group alone on caller-owned device buffers ----
static int cvf_status() { return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP; }

extern "C" int gpak_dev_cvf_pad(void *stream, double *S, long lds, int m) {
  if (!S || m < 1 || lds < cvf_pad128(m)) return GPAK_EINVAL;
  cvf_launch_pad((hipStream_t)stream, S, lds, m);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_w(void *stream, const double *T, long ldt, int m, const int *rows, const double *alpha, double *wv) {
  if (!T || !rows || !alpha || !wv || m < 1 || ldt < m) return GPAK_EINVAL;
  cvf_launch_w((hipStream_t)stream, T, ldt, m, rows, alpha, wv);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_ev(void *stream, const double *T, long ldt, int m, const double *wv, const int *rows, const double *y,
                               double sn2, const int *info, double *ev, double *vv, double *mean, double *var) {
  if (!T || !wv || !rows || !y || !info || !ev || !vv || !mean || !var || m < 1 || ldt < m) return GPAK_EINVAL;
  cvf_launch_ev((hipStream_t)stream, T, ldt, m, wv, rows, y, sn2, info, ev, vv, mean, var);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_sums(void *stream, const double *R, long ldr, int m, const double *ev, const double *vv,
                                 const int *rows, const double *alpha, double sn2, const int *info, double *logp,
                                 double *gsum) {
  if (!R || !ev || !vv || !rows || !alpha || !info || !logp || !gsum || m < 1 || ldr < m) return GPAK_EINVAL;
  cvf_launch_sums((hipStream_t)stream, R, ldr, m, ev, vv, rows, alpha, sn2, info, logp, gsum);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_beta(void *stream, const double *wv, int m, double sn2, double *sc) {
  if (!wv || !sc || m < 1) return GPAK_EINVAL;
  cvf_launch_beta((hipStream_t)stream, wv, m, sn2, sc);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_q(void *stream, int transposed, const double *T, long ldt, int m, const double *wv, const double *ev,
                              const double *sc, const int *rows, double *Q, long ldq, double *E) {
  if (!T || !wv || !ev || !sc || !rows || !Q || !E || m < 1 || ldt < m || ldq < cvf_pad128(m)) return GPAK_EINVAL;
  cvf_launch_q((hipStream_t)stream, transposed != 0, T, ldt, m, wv, ev, sc, rows, Q, ldq, E);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_gather(void *stream, const double *H, long ld, int Np, const int *cols, int m, double *A, long lda) {
  if (!H || !cols || !A || m < 1 || m > Np || ld < Np || lda < Np) return GPAK_EINVAL;
  cvf_launch_gather((hipStream_t)stream, H, ld, Np, cols, m, A, lda);
  return cvf_status();
}

extern "C" int gpak_dev_cvf_unmix(void *stream, double *H, long ld, int Np, const int *cols, int m, const double *Z, long ldz) {
  if (!H || !cols || !Z || m < 1 || m > Np || ld < Np || ldz < Np) return GPAK_EINVAL;
  cvf_launch_unmix((hipStream_t)stream, H, ld, Np, cols, m, Z, ldz);
  return cvf_status();
}

// ---------------------------------------------------------------------------------------
// What gpak_cv_folds and gpak_cv_folds_grad share: the two kinds of groups, the workspaces, one group's sequence, the
// summary and the failed group.
// ---------------------------------------------------------------------------------------
void gpak_cvf_make_plan(const int *perm, const int *offs, int n_groups, int Np, bool batch, gpak_cvf_plan &pl) {
  pl = gpak_cvf_plan();
  pl.n_groups = n_groups;
  pl.soffs.assign(1, 0);
  pl.soff.assign(1, 0);
  for (int g = 0; g < n_groups; g++) {
    const int o = offs[g], m = offs[g + 1] - o;
    pl.max_size = std::max(pl.max_size, m);
    if (batch && m <= GPAK_CV_GROUP_MAX) {
      pl.small_id.push_back(g);
      pl.sperm.insert(pl.sperm.end(), perm + o, perm + o + m);
      pl.soffs.push_back((int)pl.sperm.size());
      pl.soff.push_back(pl.soff.back() + gpak_cvg_s_elems(m));
      pl.max_small = std::max(pl.max_small, m);
    } else {
      pl.large_id.push_back(g);
      const int mp = cvf_pad128(m), k0 = perm[o] / CVF_TB * CVF_TB;   // the members are sorted: perm[o] is the smallest row
      pl.mp_max = std::max(pl.mp_max, mp);
      pl.nP = std::max(pl.nP, (size_t)mp * (size_t)(Np - k0));        // >= mp * mp: T = R^-T fits where P was
      pl.qoff.push_back(pl.nQ);
      pl.nQ += (size_t)mp * mp;
    }
  }
}

int gpak_cvf_reserve(gpak_ctx *ctx, const char *who, const gpak_cvf_plan &pl, bool grad) {
  const size_t nL = pl.large_id.size();
  if (!nL) return GPAK_OK;
  const int mp_max = pl.mp_max;
  // the gradient's mix writes its Np x m_p result where P was; by GEMM it also holds the gathered columns there
  const size_t nP = grad ? std::max(pl.nP, (size_t)(cvf_mix_by_gemm(mp_max) ? 2 : 1) * ctx->Np * mp_max) : pl.nP;
  const size_t nS = (size_t)mp_max * mp_max, nI = (size_t)(mp_max / CVF_TB) * 2 * CVF_TB * CVF_TB;
  const size_t nV = 3 * (size_t)mp_max + (grad ? 2 : 0);
  const char *what = nullptr;
  size_t bytes = 0;
  if (!ctx->dCvfP.reserve(nP)) {
    what = grad ? "P, the packed rows of L^-T of the largest group, and the N x m_p operand and result of its column mix"
                : "P, the packed rows of L^-T of the largest group";
    bytes = nP;
  }
  else if (!ctx->dCvfS.reserve(nS)) { what = "S = P P^T of the largest group"; bytes = nS; }
  else if (!ctx->dCvfInv.reserve(nI)) { what = "the inverse blocks of S's factor"; bytes = nI; }
  else if (!ctx->dCvfVec.reserve(nV)) { what = "the vectors w, e, var"; bytes = nV; }
  else if (grad && !ctx->dCvfQ.reserve(pl.nQ)) { what = "the weight factors Q of all groups above 128 samples"; bytes = pl.nQ; }
  if (what) {
    (void)hipGetLastError();
    ctx->err = std::string(who) + ": device allocation failed for " + what + " (" + std::to_string(bytes * sizeof(double)) +
               " bytes; the largest group has " + std::to_string(pl.max_size) + " samples)";
    return GPAK_ENOMEM;
  }
  while (ctx->ev_cvf.size() < 3 * nL) {
    hipEvent_t e;
    GPAK_HIP(hipEventCreate(&e));
    ctx->ev_cvf.push_back(e);
  }
  return GPAK_OK;
}

int gpak_cvf_run_group(gpak_ctx *ctx, const gpak_cvf_plan &pl, size_t k, const int *perm, const int *offs, const double *G,
                       const int *dperm, int *info, double *dmean, double *dvar, double *dlogp, double *dgsum, double *dE) {
  hipStream_t st = ctx->stream;
  const int Np = ctx->Np, mp_max = pl.mp_max;
  const long ld = ctx->ld;
  double *P = ctx->dCvfP, *S = ctx->dCvfS, *inv = ctx->dCvfInv;
  double *wv = ctx->dCvfVec, *ev = wv + mp_max, *vv = ev + mp_max;
  const int g = pl.large_id[k], o = offs[g], m = offs[g + 1] - o;
  const int mp = cvf_pad128(m), mt = mp / CVF_TB, k0 = perm[o] / CVF_TB * CVF_TB;
  const int *rows = dperm + o;
  const long ldp = mp, lds = mp;
  gpak_launch_pack_rows(st, G, ld, Np, rows, m, k0, P, ldp);
  GPAK_HIP(hipEventRecord(ctx->ev_cvf[3 * k], st));
  gpak_launch_gemm_nt(st, mt, mt, Np - k0, 1.0, P, ldp, P, ldp, 0.0, S, lds, 0, 0, true, false);
  GPAK_HIP(hipEventRecord(ctx->ev_cvf[3 * k + 1], st));
  cvf_launch_pad(st, S, lds, m);
  for (int J = 0; J < mp; J += 512) {
    const int W = std::min(512, mp - J), c0 = J + W, rest = (mp - c0) / CVF_TB;
    gpak_factor_panel(st, S, lds, mp, J, W, inv, info, true, false, ctx->sched.potrf_co);
    if (rest > 0) {
      const double *Pn = S + c0 + (size_t)J * lds;
      gpak_launch_gemm_nt(st, rest, rest, W, -1.0, Pn, lds, Pn, lds, 1.0, S + c0 + (size_t)c0 * lds, lds, 0, 0, true, false);
    }
  }
  double *T = P;                                          // the product is done with P
  const long ldt = mp;
  gpak_grad_g_of(st, mp, S, lds, inv, T, ldt);
  cvf_launch_w(st, T, ldt, m, rows, ctx->dAlpha, wv);
  cvf_launch_ev(st, T, ldt, m, wv, rows, ctx->dy, ctx->sn2, info, ev, vv, dmean, dvar);
  cvf_launch_sums(st, S, lds, m, ev, vv, rows, ctx->dAlpha, ctx->sn2, info, dlogp, dgsum);
  if (dE) {                                               // the gradient's weights of this group
    double *sc = vv + mp_max, *Q = ctx->dCvfQ + pl.qoff[k];
    cvf_launch_beta(st, wv, m, ctx->sn2, sc);
    cvf_launch_q(st, cvf_mix_by_gemm(m), T, ldt, m, wv, ev, sc, rows, Q, (long)mp, dE);   // as gpak_cvf_mix_group will read it
  }
  GPAK_HIP(hipEventRecord(ctx->ev_cvf[3 * k + 2], st));
  return GPAK_OK;
}

int gpak_cvf_finish(gpak_ctx *ctx, const char *who, const gpak_cvf_plan &pl, const double *hsum, const int *hinfo, double ms,
                    double *group_logp, gpak_cv_groups_summary *summary) {
  const size_t nSm = pl.small_id.size(), nL = pl.large_id.size(), nG = (size_t)pl.n_groups;
  // per group, in the caller's numbering: logp and the three sums
  std::vector<const double *> lp_of(nG), gs_of(nG);
  for (size_t k = 0; k < nSm; k++) { lp_of[pl.small_id[k]] = &hsum[k]; gs_of[pl.small_id[k]] = &hsum[nSm + 3 * k]; }
  for (size_t k = 0; k < nL; k++) { lp_of[pl.large_id[k]] = &hsum[4 * nSm + k]; gs_of[pl.large_id[k]] = &hsum[4 * nSm + nL + 3 * k]; }
  if (group_logp)
    for (size_t g = 0; g < nG; g++) group_logp[g] = *lp_of[g];
  if (summary) {
    double sse = 0.0, ssr = 0.0, md = 0.0, lp = 0.0;
    for (size_t g = 0; g < nG; g++) {   // ascending: a fixed order
      lp += *lp_of[g];
      sse += gs_of[g][0];
      ssr += gs_of[g][1];
      md += gs_of[g][2];
    }
    summary->mse = sse / ctx->N;
    summary->mssr = ssr / ctx->N;
    summary->msmd = md / ctx->N;
    summary->log_pl = lp;
    summary->ms = ms;
    summary->groups = pl.n_groups;
    summary->max_size = pl.max_size;
  }
  int failed = INT_MAX;   // the smallest group number whose S failed
  if (hinfo[0] != INT_MAX) failed = pl.small_id[(size_t)hinfo[0] - 1];
  for (size_t k = 0; k < nL; k++)
    if (hinfo[1 + k] != INT_MAX) { failed = std::min(failed, pl.large_id[k]); break; }
  if (failed != INT_MAX) {
    ctx->err = std::string(who) + ": S = [B^-1]_II of group " + std::to_string(failed) + " is not positive definite";
    return GPAK_ENOTPD;
  }
  return GPAK_OK;
}

int gpak_cv_folds_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *mean, double *var,
                       double *group_logp, gpak_cv_groups_summary *summary, int flags) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np;
  const long ld = ctx->ld;
  // the two kinds of groups.  Small: compacted lists for the batched kernels.  Large: where each starts in perm.
  gpak_cvf_plan pl;
  gpak_cvf_make_plan(perm, offs, n_groups, Np, !(flags & GPAK_CV_FOLDS_NO_BATCH), pl);
  const size_t nSm = pl.small_id.size(), nL = pl.large_id.size(), nG = (size_t)n_groups;
  // where G goes: as gpak_cv_groups_impl
  double *G = ctx->dG;
  if (!G) {
    if (!gpak_loo_workspace(ctx, (size_t)ld * Np)) {
      ctx->err = "gpak_cv_folds: device allocation failed for L^-T as one N x N matrix (" +
                 std::to_string((size_t)ld * Np * sizeof(double)) + " bytes)";
      return GPAK_ENOMEM;
    }
    G = ctx->dLoo;
  }
  int rc = gpak_cvf_reserve(ctx, "gpak_cv_folds", pl, false);
  if (rc) return rc;
  // scratch in the gradient's partial-sum buffer: the S of every small group, mean, var (N each), then per kind of group
  // logp and the three sums (small groups first); then the index lists
  const size_t nSs = (size_t)pl.soff.back();
  const size_t n_dbl = nSs + 2 * (size_t)N + 4 * nG;
  const size_t n_ll = nSm + 1, n_int = pl.sperm.size() + (nSm + 1) + (size_t)N + (1 + nL);
  rc = gpak_grad_scratch(ctx, n_dbl + n_ll + (n_int + 1) / 2);
  if (rc) return rc;
  double *dS = ctx->dGpart, *dmean = dS + nSs, *dvar = dmean + N;
  double *dlogp_s = dvar + N, *dgsum_s = dlogp_s + nSm, *dlogp_l = dgsum_s + 3 * nSm, *dgsum_l = dlogp_l + nL;
  long long *dsoff = reinterpret_cast<long long *>(dgsum_l + 3 * nL);
  int *dsperm = reinterpret_cast<int *>(dsoff + n_ll), *dsoffs = dsperm + pl.sperm.size(), *dperm = dsoffs + nSm + 1;
  int *dinfo = dperm + N;                                   // [0]: the batched groups; [1 + k]: one-at-a-time group k
  const std::vector<int> info0(1 + nL, INT_MAX);
  GPAK_HIP(hipMemcpyAsync(dinfo, info0.data(), sizeof(int) * (1 + nL), hipMemcpyHostToDevice, st));
  if (nSm) {
    GPAK_HIP(hipMemcpyAsync(dsoff, pl.soff.data(), sizeof(long long) * n_ll, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dsperm, pl.sperm.data(), sizeof(int) * pl.sperm.size(), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dsoffs, pl.soffs.data(), sizeof(int) * (nSm + 1), hipMemcpyHostToDevice, st));
  }
  if (nL) GPAK_HIP(hipMemcpyAsync(dperm, perm, sizeof(int) * N, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipEventRecord(ctx->ev[7], st));
  gpak_grad_g_full(ctx, G, ld);
  GPAK_HIP(hipEventRecord(ctx->ev[5], st));
  if (nSm) {
    gpak_cvg_launch_gram(ctx, G, ld, (int)nSm, dsperm, dsoffs, dsoff, dS);
    gpak_cvg_launch_solve(ctx, (int)nSm, pl.max_small, dS, dsoff, dsperm, dsoffs, dmean, dvar, dlogp_s, dgsum_s, dinfo);
  }
  GPAK_HIP(hipEventRecord(ctx->ev[6], st));
  for (size_t k = 0; k < nL; k++)
    if ((rc = gpak_cvf_run_group(ctx, pl, k, perm, offs, G, dperm, dinfo + 1 + k, dmean, dvar, dlogp_l + k, dgsum_l + 3 * k, nullptr)))
      return rc;
  GPAK_HIP(hipEventRecord(ctx->ev[9], st));
  std::vector<double> hsum(4 * nG);   // as on the device: logp and the three sums of the small groups, then of the others
  std::vector<int> hinfo(1 + nL, 0);
  GPAK_HIP(hipMemcpyAsync(hsum.data(), dlogp_s, sizeof(double) * 4 * nG, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(hinfo.data(), dinfo, sizeof(int) * (1 + nL), hipMemcpyDeviceToHost, st));
  if (mean) GPAK_HIP(hipMemcpyAsync(mean, dmean, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (var) GPAK_HIP(hipMemcpyAsync(var, dvar, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipStreamSynchronize(st));
  GPAK_HIP(hipGetLastError());
  float ms = 0, a = 0, b = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[9]));
  GPAK_HIP(hipEventElapsedTime(&a, ctx->ev[7], ctx->ev[5]));
  GPAK_HIP(hipEventElapsedTime(&b, ctx->ev[5], ctx->ev[6]));
  double part[5] = {a, b, 0, 0, 0};
  for (size_t k = 0; k < nL; k++) {
    hipEvent_t before = k ? ctx->ev_cvf[3 * k - 1] : ctx->ev[6];
    for (int s = 0; s < 3; s++) {
      float t = 0;
      GPAK_HIP(hipEventElapsedTime(&t, s ? ctx->ev_cvf[3 * k + s - 1] : before, ctx->ev_cvf[3 * k + s]));
      part[2 + s] += t;
    }
  }
  for (int k = 0; k < 5; k++) ctx->cvf_ms[k] = part[k];
  return gpak_cvf_finish(ctx, "gpak_cv_folds", pl, hsum.data(), hinfo.data(), ms, group_logp, summary);
}

