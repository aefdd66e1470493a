// design.hip -- infill drilling design on gfx950 (gpak_design): rank candidate holes by the variance they would remove.
//
// The stack z = [block averages of the T targets (T_p rows); latent values at the Mc candidate points (Mc_p rows)] and its
// posterior covariance P = prior - W W^T / sn2 are assembled with the joint call's own steps, in its buffers:
//   dWt   rows [0, T_p): the averaged fill of the targets; rows [T_p, S): the same fill of the candidates as blocks of one
//         point; then ONE substitution W = Kbar^T L^-T over all S rows;
//   dC    lower tiles of S x S: the pair fill of the targets (white / nd on the diagonal), the pair fill of the candidates
//         (nothing on it), and between them the averaged fill of the target blocks against the candidate POINTS, written
//         into the unused upper-right block and transposed below the diagonal (gpak_design_transpose_f64); then ONE SYRK.
// Targets come first and are padded to a tile boundary, so the candidate x target block P_{I,b} lies in the stored lower
// triangle.  Per hole h with rows I:  A_h = P_II + (sn2 + white) I = R R^T,  reduction[b, h] = |R^-1 P_{I,b}|^2,
// gain[h] = sum_b wt_b reduction[b, h]  (gpak_design_score_f64: one workgroup per live hole).
// A pick h*: X* = R*^-1 again from the same kernel (kEmitX), G = P_{:,I*} gathered from both sides of the lower storage
// (gpak_design_gather_f64), U = G X*^T and P -= U U^T on the lower tiles by gpak_launch_gemm_nt, U zero-padded to 128
// columns.  The argmax runs on the host over the gains of the round (ascending h, strict >: a tie goes to the smallest h):
// one host synchronisation per pick.
#include <atomic>
#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "gpak_internal.h"
#include "../../include/gpak_design.h"
#include "../../include/gpak_dev_design.h"

#define DSG_MAX GPAK_CV_GROUP_MAX   // 128: points of a hole, 8 MFMA tiles of 16
#define DSG_RP 129                  // row pitch of the LDS matrix of the Cholesky: rows and columns both conflict-free
                                    // (cv_groups.hip, CVG_RP: a column walk strides 258 dwords = 2 banks)
#define DSG_SC 32                   // target columns staged per step: two MFMA column tiles
#define DSG_SP 130                  // doubles per staged target column: 260 dwords = 4 (mod 64), so the 32 lanes of a half-wave
                                    // (16 columns x 2 consecutive k) read 32 disjoint bank pairs
#define DSG_HEAD 64                 // doubles in front of both phases' LDS: the hole's 128 row indices

typedef double dsg_d4 __attribute__((ext_vector_type(4)));

static __host__ __device__ inline int dsg_pad16(int s) { return (s + 15) & ~15; }

// Hole h = live[blockIdx.x] (live == nullptr: blockIdx.x).  Phase 1, as gpak_cvg_solve_f64: A_h gathered through the hole's
// rows into an LDS matrix of pitch DSG_RP, the right-looking Cholesky by all 256 threads, then thread i forms column i of
// X = R^-1 by forward substitution; R stays on and below the diagonal, X^T strictly above it, X's diagonal in xd.
// Phase 2: wave w takes the row tiles w and 7 - w of X (as gpak_cvg_gram_f64 balances the triangle) and loads their
// fragments into registers ONCE -- 4 (rt + 1) k-steps of tile row rt, the all-zero tiles right of the diagonal are never
// touched -- after which the LDS matrix is dead and its space is reused.
// Phase 3: Z = X P_{I,.} over the T target columns, DSG_SC at a time: all four waves stage the step's columns of P_{I,.}
// (lanes along the hole's rows: a contiguous hole reads 1 KiB per column) while the next step is on its way to registers;
// every wave runs v_mfma_f64_16x16x4 over its two row tiles and both column tiles: four independent accumulator chains.
// Z_ib is ONE chain over k ascending.  Its squares are added per lane over q ascending, the 32 (row tile, l4) partial sums
// of a column in ascending order by one lane, and gain[h] is one chain over b ascending (wave 0): the order of every sum
// depends on the element alone -- not on the grid, the other holes, T's padding or the buffer that holds P.
// A pivot that is not positive: gain[h] and column h of reduction are NaN and info takes the smallest such h + 1.
// kEmitX: the kernel stops after phase 1 and writes X (128 x 128, column-major, zero outside the hole's triangle) to Xout.
template <bool kEmitX>
__global__ __launch_bounds__(256) void gpak_design_score_f64(const double *__restrict__ P, long ld, int T,
                                                             const int *__restrict__ rows, const int *__restrict__ offs,
                                                             const int *__restrict__ live, double noise,
                                                             const double *__restrict__ wt, double *__restrict__ gain,
                                                             double *__restrict__ red, long ldr, int *info,
                                                             double *__restrict__ Xout) {
  extern __shared__ double dsg_lds[];
  const int t = threadIdx.x;
  const int h = live ? live[blockIdx.x] : (int)blockIdx.x;
  const int o = offs[h], s = offs[h + 1] - o;
  int *ridx = reinterpret_cast<int *>(dsg_lds);
  double *A = dsg_lds + DSG_HEAD;            // s rows of DSG_RP
  double *xd = A + (size_t)s * DSG_RP;       // DSG_MAX
  if (t < DSG_MAX) ridx[t] = t < s ? rows[o + t] : 0;
  __syncthreads();
  for (int e = t; e < s * s; e += 256) {     // rows ascending within the hole: (i, j), i >= j, is in the lower storage
    const int i = e % s, j = e / s;
    if (i >= j) {
      const double v = P[(size_t)ridx[i] + (size_t)ridx[j] * ld];
      A[i * DSG_RP + j] = i == j ? v + noise : v;
    }
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < s; j++) {
    const double d = A[j * DSG_RP + j];      // every thread reads the same value: the branch is uniform
    if (!(d > 0.0)) { ok = false; break; }
    const double rj = sqrt(d), ri = 1.0 / rj;
    __syncthreads();
    if (t == 0) { A[j * DSG_RP + j] = rj; xd[j] = ri; }
    for (int i = j + 1 + t; i < s; i += 256) A[i * DSG_RP + j] *= ri;
    __syncthreads();
    for (int k = j + 1 + (t >> 4); k < s; k += 16) {   // column k of the trailing block, rows k .. s - 1, 16 lanes each
      const double akj = A[k * DSG_RP + j];
      for (int i = k + (t & 15); i < s; i += 16) A[i * DSG_RP + k] = fma(-A[i * DSG_RP + j], akj, A[i * DSG_RP + k]);
    }
    __syncthreads();
  }
  if (!ok) {
    if (kEmitX) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (red)
      for (int b = t; b < T; b += 256) red[(size_t)b + (size_t)h * ldr] = nan;
    if (t == 0) { gain[h] = nan; atomicMin(info, h + 1); }
    return;
  }
  // column i of X by thread i: X_ii = 1 / R_ii, X_ji = -(sum_{i <= k < j} R_jk X_ki) / R_jj, kept as A[i][j] (j > i)
  for (int j = 1; j < s; j++) {
    const int i = t;
    if (i < j) {
      const double *Rj = A + j * DSG_RP;
      double *xi = A + i * DSG_RP;
      double acc = 0.0;
#pragma unroll 4
      for (int k = j - 1; k > i; k--) acc = fma(Rj[k], xi[k], acc);
      acc = fma(Rj[i], xd[i], acc);
      xi[j] = -acc * xd[j];
    }
  }
  __syncthreads();
  // X_rk for k <= r < s, zero elsewhere
  auto xval = [&](int r, int k) { return (r < s && k <= r) ? (k == r ? xd[r] : A[k * DSG_RP + r]) : 0.0; };
  if (kEmitX) {
    for (int e = t; e < DSG_MAX * DSG_MAX; e += 256) Xout[e] = xval(e % DSG_MAX, e / DSG_MAX);
    return;
  }

  const int lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nt = __builtin_amdgcn_readfirstlane(dsg_pad16(s) >> 4);
  const int rtA = w, rtB = 7 - w;
  const int nkA = rtA < nt ? 4 * (rtA + 1) : 0, nkB = rtB < nt ? 4 * (rtB + 1) : 0;   // k-steps of 4 of the two row tiles
  double xa[16], xb[32];
#pragma unroll
  for (int kt = 0; kt < 16; kt++) xa[kt] = kt < nkA ? xval(rtA * 16 + l15, kt * 4 + l4) : 0.0;
#pragma unroll
  for (int kt = 0; kt < 32; kt++) xb[kt] = kt < nkB ? xval(rtB * 16 + l15, kt * 4 + l4) : 0.0;
  __syncthreads();                           // the LDS matrix is dead from here

  double *stage = dsg_lds + DSG_HEAD;        // DSG_SC columns of DSG_SP
  double *part = stage + DSG_SC * DSG_SP;    // 32 (row tile, l4) partial sums x DSG_SC columns
  const int r = t & 127, hf = t >> 7;        // staging: row r of the hole, columns hf * 16 .. hf * 16 + 15 of the step
  const bool rl = r < s;
  const double *prow = P + (size_t)(rl ? ridx[r] : 0);
  double v[16];
  auto load = [&](int b0) {
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int b = b0 + hf * 16 + u;
      v[u] = (rl && b < T) ? prow[(size_t)b * ld] : 0.0;
    }
  };
  load(0);
  double g = 0.0;
  for (int b0 = 0; b0 < T; b0 += DSG_SC) {
#pragma unroll
    for (int u = 0; u < 16; u++) stage[(hf * 16 + u) * DSG_SP + r] = v[u];
    __syncthreads();
    if (b0 + DSG_SC < T) load(b0 + DSG_SC);
    dsg_d4 aA0 = {0.0, 0.0, 0.0, 0.0}, aA1 = aA0, aB0 = aA0, aB1 = aA0;
    const double *c0 = stage + l15 * DSG_SP + l4, *c1 = c0 + 16 * DSG_SP;
#pragma unroll
    for (int kt = 0; kt < 32; kt++) {
      if (kt < nkB) {
        const double p0 = c0[kt * 4], p1 = c1[kt * 4];
        aB0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[kt], p0, aB0, 0, 0, 0);
        aB1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[kt], p1, aB1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int kt = 0; kt < 16; kt++) {
      if (kt < nkA) {
        const double p0 = c0[kt * 4], p1 = c1[kt * 4];
        aA0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[kt], p0, aA0, 0, 0, 0);
        aA1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[kt], p1, aA1, 0, 0, 0);
      }
    }
    // the lane holds Z of rows rt * 16 + l4 + 4 q (q = 0..3), column ct * 16 + l15
    double sA0 = 0.0, sA1 = 0.0, sB0 = 0.0, sB1 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      sA0 = fma(aA0[q], aA0[q], sA0); sA1 = fma(aA1[q], aA1[q], sA1);
      sB0 = fma(aB0[q], aB0[q], sB0); sB1 = fma(aB1[q], aB1[q], sB1);
    }
    part[(rtA * 4 + l4) * DSG_SC + l15] = sA0; part[(rtA * 4 + l4) * DSG_SC + 16 + l15] = sA1;
    part[(rtB * 4 + l4) * DSG_SC + l15] = sB0; part[(rtB * 4 + l4) * DSG_SC + 16 + l15] = sB1;
    __syncthreads();
    if (w == 0) {
      const int col = lane & (DSG_SC - 1), b = b0 + col;
      double tot = 0.0;
#pragma unroll 8
      for (int e = 0; e < 32; e++) tot += part[e * DSG_SC + col];
      const bool own = lane < DSG_SC && b < T;
      if (own && red) red[(size_t)b + (size_t)h * ldr] = tot;
      const double wv = own ? (wt ? wt[b] * tot : tot) : 0.0;
#pragma unroll
      for (int j = 0; j < DSG_SC; j++) g += __shfl(wv, j);
    }
    __syncthreads();
  }
  if (t == 0) gain[h] = g;
}

static size_t dsg_score_lds(int s) {
  const size_t a = (size_t)s * DSG_RP + DSG_MAX, b = (size_t)DSG_SC * DSG_SP + 32 * DSG_SC;
  return sizeof(double) * (DSG_HEAD + (a > b ? a : b));
}

template <bool kEmitX>
static void dsg_launch_score(hipStream_t st, int device, const double *P, long ld, int T, const int *rows, const int *offs,
                             const int *live, int n_live, int max_size, double noise, const double *wt, double *gain,
                             double *red, long ldr, int *info, double *Xout) {
  // more than 64 KiB of dynamic LDS needs the opt-in, once per kernel and per device
  {
    static std::atomic<unsigned long long> done_mask{0};
    const unsigned long long bit = 1ull << (device & 63);
    if (!(done_mask.load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gpak_design_score_f64<kEmitX>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)dsg_score_lds(DSG_MAX));
      done_mask.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(gpak_design_score_f64<kEmitX>, dim3(n_live), dim3(256), dsg_score_lds(max_size), st, P, ld, T, rows, offs,
                     live, noise, wt, gain, red, ldr, info, Xout);
}

extern "C" int gpak_dev_design_score(void *stream, const double *P, long ld, int T, const int *rows, const int *offs,
                                     const int *live, int n_live, double noise, const double *wt, double *gain,
                                     double *reduction, long ldr, int *info) {
  if (!P || !rows || !offs || !gain || !info || T < 1 || n_live < 1 || ld <= T || (reduction && ldr < T)) return GPAK_EINVAL;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return GPAK_EHIP;
  dsg_launch_score<false>((hipStream_t)stream, device, P, ld, T, rows, offs, live, n_live, DSG_MAX, noise, wt, gain, reduction,
                          ldr, info, nullptr);
  return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP;
}

// C[Tp + c, b] = C[b, Tp + c] for b < Tp, c < Mcp: the target x candidate block, filled above the diagonal, to where the
// lower storage keeps it.  32 x 32 tiles through LDS (pitch 33): reads and writes both run along a column.
__global__ __launch_bounds__(256) void gpak_design_transpose_f64(double *C, long ld, int Tp) {
  __shared__ double tile[32][33];
  const int b0 = blockIdx.x * 32, c0 = blockIdx.y * 32, x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
  for (int y = y0; y < 32; y += 8) tile[y][x] = C[(size_t)(b0 + x) + (size_t)(Tp + c0 + y) * ld];   // [c][b]
  __syncthreads();
  for (int y = y0; y < 32; y += 8) C[(size_t)(Tp + c0 + x) + (size_t)(b0 + y) * ld] = tile[x][y];
}

// out[b] = C[b, b], b < n
__global__ void gpak_design_diag_f64(const double *__restrict__ C, long ld, int n, double *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n) out[b] = C[(size_t)b + (size_t)b * ld];
}

// G[r, k] = P(r, rows[k]) for every stacked row r < S and k < m, zero for m <= k < 128, from the lower storage C: the
// element itself where r >= rows[k], its transpose C[rows[k], r] where r lies above -- every target row does, targets
// precede candidates.  One workgroup per 32 rows x 32 columns: the transposed side is read with the lanes along k (a
// contiguous hole reads along a column of C) and turned through LDS, the direct side with the lanes along r.
__global__ __launch_bounds__(256) void gpak_design_gather_f64(const double *__restrict__ C, long ld, const int *__restrict__ rows,
                                                              int m, double *__restrict__ G, long ldg) {
  __shared__ double tile[32][33];
  __shared__ int rk[32];
  const int r0 = blockIdx.x * 32, k0 = blockIdx.y * 32, x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
  if (threadIdx.x < 32) rk[threadIdx.x] = k0 + (int)threadIdx.x < m ? rows[k0 + threadIdx.x] : -1;
  __syncthreads();
  for (int y = y0; y < 32; y += 8) {         // lane x = column k0 + x, row r0 + y
    const int ck = rk[x], r = r0 + y;
    if (ck > r) tile[y][x] = C[(size_t)ck + (size_t)r * ld];
  }
  __syncthreads();
  for (int y = y0; y < 32; y += 8) {         // lane x = row r0 + x, column k0 + y
    const int ck = rk[y], r = r0 + x;
    G[(size_t)r + (size_t)(k0 + y) * ldg] = ck < 0 ? 0.0 : ck > r ? tile[x][y] : C[(size_t)r + (size_t)ck * ld];
  }
}

// the fills + transpose, the substitution, the SYRK, the first score pass and the last pick's downdate of the context's
// last gpak_design, in ms.  Not part of the C-ABI (no header declares it): tools/time_design.py reads it through the
// shared object.
extern "C" int gpak_design_last_split(gpak_ctx *ctx, double *ms5) {
  if (!ctx || !ms5 || ctx->multi) return GPAK_EINVAL;
  for (int k = 0; k < 5; k++) ms5[k] = ctx->design_ms[k];
  return GPAK_OK;
}

// gpak_design on a single-GPU context whose factor and alpha are current and whose arguments api.hip has checked: perm =
// the candidate points sorted by (hole, point), offs = where each hole starts in it (H + 1 entries)
int gpak_design_impl(gpak_ctx *ctx, const double *Xt, long T, int nd, const double *Xc, long Mc, const int *perm,
                     const int *offs, int H, const double *wt, int k, double *gain, double *reduction, double *var,
                     int *picked, double *pick_gain, double *var_after, gpak_design_summary *summary) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, d = ctx->d;
  KernParams kp = ctx->kp;
  kp.d = d;
  const int Tp = (int)((T + 255) / 256 * 256), Mcp = (int)((Mc + 255) / 256 * 256), S = Tp + Mcp;
  const int nT = (int)T, nC = (int)Mc;
  const long Tn = T * nd;
  long ld = 0;
  int rc = gpak_joint_reserve(ctx, S, (size_t)nd * Tp + Mcp, kp.nterms, &ld);
  if (rc) return rc;
  double *W = ctx->dWt, *C = ctx->dC;
  // scratch in the gradient's partial-sum buffer: G and U (S x 128 each), X* (128 x 128), the first round's reduction,
  // the two gain vectors, the weights, the diagonal; then the index lists
  const size_t nRed = reduction ? (size_t)T * H : 0, nH = (size_t)H;
  const size_t n_dbl = 2 * (size_t)S * DSG_MAX + (size_t)DSG_MAX * DSG_MAX + nRed + 2 * nH + 2 * (size_t)T;
  const size_t n_int = (size_t)Mc + nH + 1 + nH + 1;
  if ((rc = gpak_grad_scratch(ctx, n_dbl + (n_int + 1) / 2))) return rc;
  double *dG = ctx->dGpart, *dU = dG + (size_t)S * DSG_MAX, *dX = dU + (size_t)S * DSG_MAX, *dRed = dX + DSG_MAX * DSG_MAX;
  double *dGain = dRed + nRed, *dGain2 = dGain + nH, *dWgt = dGain2 + nH, *dDiag = dWgt + T;
  int *dRows = reinterpret_cast<int *>(dDiag + T), *dOffs = dRows + Mc, *dLive = dOffs + nH + 1, *dInfo = dLive + nH;

  int max_size = 0;
  std::vector<int> hrows((size_t)Mc);
  for (long i = 0; i < Mc; i++) hrows[(size_t)i] = Tp + perm[i];   // the candidate's row of the stack
  for (int h = 0; h < H; h++) max_size = std::max(max_size, offs[h + 1] - offs[h]);
  const int info0 = INT_MAX;
  GPAK_HIP(hipMemcpyAsync(dRows, hrows.data(), sizeof(int) * Mc, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dOffs, offs, sizeof(int) * (nH + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dInfo, &info0, sizeof(int), hipMemcpyHostToDevice, st));
  if (wt) GPAK_HIP(hipMemcpyAsync(dWgt, wt, sizeof(double) * T, hipMemcpyHostToDevice, st));
  const double *dW = wt ? dWgt : nullptr;

  hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[6], e2 = ctx->ev[7], e3 = ctx->ev[8], e4 = ctx->ev[9];
  GPAK_HIP(hipEventRecord(e0, st));
  // pooled mean over the training set, all T * nd target points and all Mc candidate points
  double s2[4] = {0, 0, 0, 0};
  for (int c = 0; c < d; c++) {
    for (long i = 0; i < Tn; i++) s2[c] += Xt[i + (size_t)c * Tn];
    for (long i = 0; i < Mc; i++) s2[c] += Xc[i + (size_t)c * Mc];
  }
  gpak_pooled_mean(ctx->xsum, N, s2, Tn + Mc, kp.mu);
  gpak_launch_transform(st, ctx->dX, Np, N, kp, ctx->Upred);

  // raw columns: the targets' (stride Tn), then the candidates' (stride Mc); transformed: the targets point-major with
  // cap Tp, then the candidates, which as blocks of one point with cap Mcp are a DevPoints of the same layout
  double *xT = ctx->dXblk, *xC = ctx->dXblk + 4 * (size_t)Tn;
  for (int c = 0; c < d; c++) {
    GPAK_HIP(hipMemcpyAsync(xT + (size_t)c * Tn, Xt + (size_t)c * Tn, sizeof(double) * Tn, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(xC + (size_t)c * Mc, Xc + (size_t)c * Mc, sizeof(double) * Mc, hipMemcpyHostToDevice, st));
  }
  double *pT = ctx->dTblk;
  DevPoints Q;
  Q.base = ctx->dTblk + (size_t)GPAK_PT * kp.nterms * nd * Tp;
  Q.cap = Mcp;
  gpak_launch_transform_blocks(st, xT, Tn, nT, nd, Tp, kp, pT);
  gpak_launch_transform(st, xC, nC, nC, kp, Q);
  gpak_launch_fill_blocks(st, pT, Tp, nT, nd, ctx->Upred, Tp, Np, kp, W, ld);
  gpak_launch_fill_blocks(st, Q.base, Mcp, nC, 1, ctx->Upred, Mcp, Np, kp, W + Tp, ld);
  gpak_launch_fill_block_pairs(st, pT, Tp, nT, nd, kp, kp.white / nd, C, ld);
  gpak_launch_fill_block_pairs(st, Q.base, Mcp, nC, 1, kp, 0.0, C + Tp + (size_t)Tp * ld, ld);
  gpak_launch_fill_blocks(st, pT, Tp, nT, nd, Q, Tp, Mcp, kp, C + (size_t)Tp * ld, ld);
  hipLaunchKernelGGL(gpak_design_transpose_f64, dim3(Tp / 32, Mcp / 32), dim3(256), 0, st, C, ld, Tp);
  GPAK_HIP(hipEventRecord(e1, st));
  gpak_joint_forward_subst(ctx, S, ld);
  GPAK_HIP(hipEventRecord(e2, st));
  gpak_launch_gemm_nt(st, S / 128, S / 128, Np, -1.0 / ctx->sn2, W, ld, W, ld, 1.0, C, ld, 0, 0, true, false);
  GPAK_HIP(hipEventRecord(e3, st));

  const double noise = ctx->sn2 + kp.white;
  std::vector<double> hgain(nH), hdiag((size_t)T);
  int info = 0;
  hipLaunchKernelGGL(gpak_design_diag_f64, dim3((nT + 255) / 256), dim3(256), 0, st, C, ld, nT, dDiag);
  GPAK_HIP(hipMemcpyAsync(hdiag.data(), dDiag, sizeof(double) * T, hipMemcpyDeviceToHost, st));
  dsg_launch_score<false>(st, ctx->device, C, ld, nT, dRows, dOffs, nullptr, H, max_size, noise, dW, dGain,
                          reduction ? dRed : nullptr, T, dInfo, nullptr);
  GPAK_HIP(hipEventRecord(e4, st));
  GPAK_HIP(hipMemcpyAsync(hgain.data(), dGain, sizeof(double) * nH, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipMemcpyAsync(&info, dInfo, sizeof(int), hipMemcpyDeviceToHost, st));
  if (reduction) GPAK_HIP(hipMemcpyAsync(reduction, dRed, sizeof(double) * nRed, hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipStreamSynchronize(st));
  GPAK_HIP(hipGetLastError());
  float part[4] = {0, 0, 0, 0};
  GPAK_HIP(hipEventElapsedTime(&part[0], e0, e1));
  GPAK_HIP(hipEventElapsedTime(&part[1], e1, e2));
  GPAK_HIP(hipEventElapsedTime(&part[2], e2, e3));
  GPAK_HIP(hipEventElapsedTime(&part[3], e3, e4));
  double total_ms = (double)part[0] + part[1] + part[2] + part[3];
  for (int c = 0; c < 4; c++) ctx->design_ms[c] = part[c];
  ctx->design_ms[4] = 0.0;

  auto weighted = [&](const std::vector<double> &v) {   // sum_b wt_b v_b, b ascending
    double acc = 0.0;
    for (long b = 0; b < T; b++) acc += wt ? wt[b] * v[(size_t)b] : v[(size_t)b];
    return acc;
  };
  for (int h = 0; h < H; h++) gain[h] = hgain[(size_t)h];
  if (var) for (long b = 0; b < T; b++) var[b] = hdiag[(size_t)b];
  if (var_after) for (long b = 0; b < T; b++) var_after[b] = hdiag[(size_t)b];
  const double var_before = weighted(hdiag);
  if (summary) {
    summary->var_before = summary->var_after = var_before;
    summary->ms = total_ms;
    summary->holes = H; summary->max_size = max_size; summary->picks = 0;
  }
  ctx->times.predict_ms = total_ms;
  auto failed = [&](int done) {
    ctx->err = "gpak_design: A_h = P_II + (sn2 + white) I of hole " + std::to_string(info - 1) +
               " is not positive definite" + (done ? " after " + std::to_string(done) + " pick(s)" : std::string());
    return GPAK_ENOTPD;
  };
  if (info != INT_MAX) return failed(0);

  // the greedy plan: one host synchronisation per pick
  std::vector<int> live((size_t)H);
  for (int h = 0; h < H; h++) live[(size_t)h] = h;
  for (int p = 0; p < k; p++) {
    size_t best = 0;
    for (size_t j = 1; j < live.size(); j++)   // ascending h, strict >: a tie goes to the smallest h
      if (hgain[(size_t)live[j]] > hgain[(size_t)live[best]]) best = j;
    const int hs = live[best], m = offs[hs + 1] - offs[hs];
    picked[p] = hs;
    pick_gain[p] = hgain[(size_t)hs];
    live.erase(live.begin() + (long)best);
    GPAK_HIP(hipEventRecord(e0, st));
    GPAK_HIP(hipMemcpyAsync(dLive, &hs, sizeof(int), hipMemcpyHostToDevice, st));
    dsg_launch_score<true>(st, ctx->device, C, ld, nT, dRows, dOffs, dLive, 1, m, noise, nullptr, nullptr, nullptr, 0, dInfo, dX);
    hipLaunchKernelGGL(gpak_design_gather_f64, dim3(S / 32, DSG_MAX / 32), dim3(256), 0, st, C, ld, dRows + offs[hs], m, dG,
                       (long)S);
    gpak_launch_gemm_nt(st, S / 128, 1, DSG_MAX, 1.0, dG, S, dX, DSG_MAX, 0.0, dU, S, 0, 0, false, false);
    gpak_launch_gemm_nt(st, S / 128, S / 128, DSG_MAX, -1.0, dU, S, dU, S, 1.0, C, ld, 0, 0, true, false);
    GPAK_HIP(hipEventRecord(e1, st));
    if (p + 1 < k) {
      GPAK_HIP(hipMemcpyAsync(dLive, live.data(), sizeof(int) * live.size(), hipMemcpyHostToDevice, st));
      dsg_launch_score<false>(st, ctx->device, C, ld, nT, dRows, dOffs, dLive, (int)live.size(), max_size, noise, dW, dGain2,
                              nullptr, 0, dInfo, nullptr);
      GPAK_HIP(hipMemcpyAsync(hgain.data(), dGain2, sizeof(double) * nH, hipMemcpyDeviceToHost, st));
      GPAK_HIP(hipMemcpyAsync(&info, dInfo, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    GPAK_HIP(hipEventRecord(e2, st));
    GPAK_HIP(hipStreamSynchronize(st));
    GPAK_HIP(hipGetLastError());
    float down = 0, both = 0;
    GPAK_HIP(hipEventElapsedTime(&down, e0, e1));
    GPAK_HIP(hipEventElapsedTime(&both, e0, e2));
    ctx->design_ms[4] = down;
    total_ms += both;
    if (summary) { summary->picks = p + 1; summary->ms = total_ms; }
    ctx->times.predict_ms = total_ms;
    if (info != INT_MAX) return failed(p + 1);
  }
  if (k > 0) {
    hipLaunchKernelGGL(gpak_design_diag_f64, dim3((nT + 255) / 256), dim3(256), 0, st, C, ld, nT, dDiag);
    GPAK_HIP(hipMemcpyAsync(hdiag.data(), dDiag, sizeof(double) * T, hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipStreamSynchronize(st));
    if (var_after) for (long b = 0; b < T; b++) var_after[b] = hdiag[(size_t)b];
    if (summary) summary->var_after = weighted(hdiag);
  }
  return GPAK_OK;
}
