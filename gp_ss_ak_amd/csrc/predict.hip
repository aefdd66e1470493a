// predict.hip -- predictive mean / variance and multi-right-hand-side solve_chol for gfx950.
//
// Replaces GP_utils::_ComputeK_NewData / _postMean / _postVar (GP_Utils.cpp:943-1004).
// The reference materialises kX (N x M) and runs two dtrtrs with M right-hand sides; here
//   mean  = fused Gram-matvec (kX never stored),
//   var_t = kD - (1/sn2) * | L^-1 k*_t |^2       (one forward substitution, not two),
// streamed over test batches.  The cross-kernel is kept TEST-MAJOR (Wt = kX^T, batch x N) so
// that both steps of the blocked forward substitution are the same A*B^T MFMA kernel as the
// Cholesky:   Wt[:, j] := Wt[:, j] * inv(L_jj)^T ;  Wt[:, rest] -= Wt[:, j] * L[rest, j]^T.
#include <algorithm>
#include <cstdlib>

#include "gpak_internal.h"

#define PB 128

// part[split][t] = sum over the split's columns of V[t, c]^2
__global__ __launch_bounds__(256) void gpak_rowsumsq_part_f64(const double *__restrict__ V, long ldv, int rows,
                                                               int cols, int cols_per_split,
                                                               double *__restrict__ part, int part_ld) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= rows) return;
  const int c0 = blockIdx.y * cols_per_split;
  const int c1 = min(cols, c0 + cols_per_split);
  double s0 = 0.0, s1 = 0.0;
  int c = c0;
  for (; c + 1 < c1; c += 2) {
    double a = V[t + (size_t)c * ldv], b = V[t + (size_t)(c + 1) * ldv];
    s0 = fma(a, a, s0);
    s1 = fma(b, b, s1);
  }
  if (c < c1) { double a = V[t + (size_t)c * ldv]; s0 = fma(a, a, s0); }
  part[(size_t)blockIdx.y * part_ld + t] = s0 + s1;
}

// part[split][t] = sum over the split's columns of V[t, c] * x[c], columns in ascending order
__global__ __launch_bounds__(256) void gpak_rowdot_part_f64(const double *__restrict__ V, long ldv, int rows, int cols,
                                                             int cols_per_split, const double *__restrict__ x,
                                                             double *__restrict__ part, int part_ld) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= rows) return;
  const int c0 = blockIdx.y * cols_per_split;
  const int c1 = min(cols, c0 + cols_per_split);
  double s = 0.0;
  for (int c = c0; c < c1; c++) s = fma(V[t + (size_t)c * ldv], x[c], s);
  part[(size_t)blockIdx.y * part_ld + t] = s;
}

static int ensure_predict_bufs(gpak_ctx *ctx, int cap, bool want_var) {
  if (ctx->pred_cap < cap) {
    ctx->pred_cap = 0;
    ctx->dXte.release(); ctx->dPv.release(); ctx->dPart.release();   // all three go before the first comes back
    if (!ctx->dXte.reserve(4 * (size_t)cap) || !ctx->dPv.reserve(2 * (size_t)cap) || !ctx->dPart.reserve(64 * (size_t)cap)) {
      ctx->err = "device allocation failed for prediction buffers";
      return GPAK_ENOMEM;
    }
    int rc = gpak_alloc_points(ctx, ctx->Tq, cap);
    if (rc) return rc;
    ctx->pred_cap = cap;
  }
  int rc = gpak_alloc_points(ctx, ctx->Upred, ctx->Np);
  if (rc) return rc;
  // (pred_cap + skew) x Np: the batch is stored with a skewed leading dimension (gpak_predict_impl)
  size_t need = want_var ? ((size_t)ctx->pred_cap + 64 * (size_t)std::max(0, ctx->sched.pred_ld_skew)) * ctx->Np : 0;
  if (!ctx->dWt.reserve(need)) {
    ctx->err = "device allocation failed for the cross-kernel batch";
    return GPAK_ENOMEM;
  }
  return GPAK_OK;
}

// the raw (4 columns) and the transformed coordinates of `points` discretisation points under nterms terms (the block and
// the joint calls)
static int ensure_block_points(gpak_ctx *ctx, size_t points, int nterms) {
  if (ctx->blk_points >= points && ctx->blk_terms >= nterms) return GPAK_OK;
  ctx->blk_points = 0;
  ctx->dXblk.release(); ctx->dTblk.release();
  if (!ctx->dXblk.reserve(4 * points) || !ctx->dTblk.reserve(GPAK_PT * nterms * points)) {
    ctx->err = "device allocation failed for the blocks' discretisation points";
    return GPAK_ENOMEM;
  }
  ctx->blk_points = points; ctx->blk_terms = nterms;
  return GPAK_OK;
}

// blocked forward substitution on the test-major batch: Wt (mbp x Np, ld ldw) := Wt * L^-T.
// A ladder of block widths like the fp32 path below (GpakSchedule::fs_levels, 128 / 512 / 2048 / 8192): a block of width
// lv[k] is solved by its children of width lv[k-1], each followed by ONE K = lv[k-1] update of the rest of the block.
// Round 3: the two-level form (128-column steps inside 512 columns, then a K = 512 update of everything to the
// right) left 75 % of the flops in K = 512 products (70.7 TFLOP/s alone); with the ladder they sit in K = 8192 / 2048
// products (75.7): 72.0 -> 73.1 TFLOP/s for the whole fp64 variance pass in a same-box A/B (the pass is within 5 % of
// the package power limit either way); same sums to 13 digits.
static void fs_block_f64(gpak_ctx *ctx, double *Wt, long ldw, int mt, int J0, int W, const std::vector<int> &lv, int k) {
  hipStream_t st = ctx->stream;
  const long ld = ctx->ld;
  if (k == 0) {   // W == 128: product with the explicit inverse of the diagonal block
    const double *inv = ctx->dInv + (size_t)(J0 / PB) * 2 * PB * PB;
    double *Wj = Wt + (size_t)J0 * ldw;
    gpak_launch_gemm_nt(st, mt, 1, PB, 1.0, Wj, ldw, inv, PB, 0.0, Wj, ldw, 0, 0, false, false);
    return;
  }
  const int cw = lv[k - 1];
  for (int j0 = J0; j0 < J0 + W; j0 += cw) {
    const int w = std::min(cw, J0 + W - j0);
    fs_block_f64(ctx, Wt, ldw, mt, j0, w, lv, k - 1);
    const int nrest = (J0 + W - j0 - w) / PB;
    if (nrest > 0)
      gpak_launch_gemm_nt(st, mt, nrest, w, -1.0, Wt + (size_t)j0 * ldw, ldw, ctx->dM + (j0 + w) + (size_t)j0 * ld, ld, 1.0,
                          Wt + (size_t)(j0 + w) * ldw, ldw, 0, 0, false, false);
  }
}
static void forward_subst_batch(gpak_ctx *ctx, double *Wt, long ldw, int mbp) {
  std::vector<int> lv;
  for (int v : ctx->sched.fs_levels) if (v > 0) lv.push_back(v);
  if (lv.empty()) lv = {PB, 512};
  lv.push_back(ctx->Np > lv.back() ? ctx->Np : lv.back() + 1);   // the whole matrix is the top block
  fs_block_f64(ctx, Wt, ldw, mbp / PB, 0, ctx->Np, lv, (int)lv.size() - 1);
}

// the cap x cap covariance of the joint calls (leading dimension ldc), its inverted 128-blocks and its info word
static int ensure_joint_cov(gpak_ctx *ctx, int cap, long ldc) {
  if (ctx->joint_cap >= cap && ctx->dC.n >= (size_t)ldc * cap) return GPAK_OK;
  ctx->joint_cap = 0;
  ctx->dC.release(); ctx->dCinv.release();
  if (!ctx->dCinfo.reserve(4) || !ctx->dC.reserve((size_t)ldc * cap) || !ctx->dCinv.reserve((size_t)(cap / PB) * 2 * PB * PB)) {
    ctx->err = "device allocation failed for the joint covariance of the blocks";
    return GPAK_ENOMEM;
  }
  ctx->joint_cap = cap;
  return GPAK_OK;
}

// what gpak_design_impl (design.hip) shares with the joint calls: their buffers for a stack of `cap` rows and `points`
// discretisation points, sized and skewed as gpak_joint_impl sizes them (*ld = the leading dimension of dWt and dC), and
// the substitution dWt := dWt L^-T on the context's stream
int gpak_joint_reserve(gpak_ctx *ctx, int cap, size_t points, int nterms, long *ld) {
  int rc = ensure_predict_bufs(ctx, cap, true);
  if (rc) return rc;
  if ((rc = ensure_block_points(ctx, points, nterms))) return rc;
  *ld = cap + 32L * std::max(0, ctx->sched.pred_ld_skew);
  return ensure_joint_cov(ctx, cap, *ld);
}
void gpak_joint_forward_subst(gpak_ctx *ctx, int cap, long ldw) { forward_subst_batch(ctx, ctx->dWt, ldw, cap); }
// the substitution of the prediction path on any test-major batch: Wt (rows x Np, rows a multiple of 128, leading dimension
// ldw) := Wt L^-T on the context's stream
void gpak_forward_subst_rows(gpak_ctx *ctx, double *Wt, long ldw, int rows) { forward_subst_batch(ctx, Wt, ldw, rows); }
// what gpak_condition_impl (condition.hip) shares with the block path: its buffers, sized and skewed as
// gpak_predict_block_impl sizes them; the cross-kernel batch only where the comparison path asks for it
int gpak_block_reserve(gpak_ctx *ctx, int cap, size_t points, int nterms, bool want_wt, long *ldw) {
  int rc = ensure_predict_bufs(ctx, cap, want_wt);
  if (rc) return rc;
  *ldw = cap + 32L * std::max(0, ctx->sched.pred_ld_skew);
  return ensure_block_points(ctx, points, nterms);
}

// fp32 images of the factor for a GPAK_F32 context (rebuilt when the factor changes)
static int ensure_f32_factor(gpak_ctx *ctx) {
  if (ctx->state.image) return GPAK_OK;
  const int Np = ctx->Np, T = Np / PB;
  // k-columns 128 KiB apart (Np = 32768 floats) would all fall on the same L2 channel / HBM bank group: skew the
  // leading dimension by 256 B like the fp64 matrix (gpak_set_train)
  ctx->ldLf = Np + 64L * std::max(0, ctx->sched.pred_ld_skew);
  // allocated once per training set (release_train, api.hip)
  if (!ctx->dLf.reserve((size_t)ctx->ldLf * Np) || !ctx->dInvf.reserve((size_t)T * 2 * PB * PB)) {
    ctx->err = "device allocation failed for the fp32 factor image";
    return GPAK_ENOMEM;
  }
  gpak_launch_lower_to_f32(ctx->stream, ctx->dM, ctx->ld, Np, ctx->dLf, ctx->ldLf);
  gpak_launch_vec_to_f32(ctx->stream, ctx->dInv, (size_t)T * 2 * PB * PB, ctx->dInvf);
  ctx->state.image_built();
  return GPAK_OK;
}

// The forward substitution in fp32 (v_mfma_f32_16x16x4_f32), MULTI-level: a block of width lv[k] is solved child by
// child (width lv[k-1]); after each child ONE product of K = lv[k-1] updates the rest of the block.  Wider products
// move less (each level reads and writes the batch at most 3 times) and keep the MFMA pipe fed longer per launch, but
// with plain fp32 accumulation they cost accuracy: the terms of a product mostly share a sign, a running fp32 sum
// grows ~linearly with K and is rounded at that magnitude K/4 times -- measured at N = 32768, M = 65536 against the
// fp64 context: ladder 128/512 6.8e-6 of the largest variance, 128/512/2048 2.5e-5, 128/512/2048/8192 7e-5
// (profiles/r03_f32_accumulation.txt).  The products therefore run on gpak_gemm_nt_f32_rsw (fp32 chunks of K = 128
// summed in fp64, gemm_f32.hip): 7.4e-7 whatever the ladder, which is then chosen for speed alone.
// GPAK_FS_LEVELS_F32="128,512" restores the two-level scheme (A/B runs).
static void fs_block_f32(const GpakFsF32 &f, float *Wt, long ldw, int mt, int J0, int W, const std::vector<int> &lv, int k) {
  hipStream_t st = f.stream;
  if (k == 0) {   // W == 128: product with the explicit inverse of the diagonal block
    const float *inv = f.invf + (size_t)(J0 / PB) * 2 * PB * PB;
    float *Wj = Wt + (size_t)J0 * ldw;
    gpak_launch_gemm_nt_f32(st, mt, 1, PB, 1.f, Wj, ldw, inv, PB, 0.f, Wj, ldw);
    return;
  }
  const int cw = lv[k - 1];
  for (int j0 = J0; j0 < J0 + W; j0 += cw) {
    const int w = std::min(cw, J0 + W - j0);
    fs_block_f32(f, Wt, ldw, mt, j0, w, lv, k - 1);
    const int nrest = (J0 + W - j0 - w) / PB;
    if (nrest > 0)
      gpak_launch_gemm_nt_f32(st, mt, nrest, w, -1.f, Wt + (size_t)j0 * ldw, ldw, f.Lf + (j0 + w) + (size_t)j0 * f.ldLf, f.ldLf,
                              1.f, Wt + (size_t)(j0 + w) * ldw, ldw);
  }
}
void gpak_forward_subst_f32(const GpakFsF32 &f, float *Wt, long ldw, int mrows, int Np, std::vector<int> lv) {
  if (lv.empty()) lv = {PB, 512};
  lv.push_back(Np > lv.back() ? Np : lv.back() + 1);   // the whole matrix is the top block
  // the top block's width need not be a multiple of its children's: fs_block_f32 clips the last child
  fs_block_f32(f, Wt, ldw, mrows / PB, 0, Np, lv, (int)lv.size() - 1);
}

// pool_sum / pool_M: column sums and count of the WHOLE test set when Xte is a slice of it (multi-GPU prediction
// shards the test points; the pooled mean of Kernel.cpp:1391-1392 is over all of them), or nullptr
int gpak_predict_impl(gpak_ctx *ctx, const double *Xte, long M, double *mean, double *var, const double *pool_sum,
                      long pool_M) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np;
  // test points per batch, measured at N=32768: 4096 -> 58 (f64) / 91 (f32) TFLOP/s, 16384 -> 71.6 / 115.4,
  // 32768 -> 71.7 / 118.7, 65536 -> 71.8 / 119.7: the fp32 path takes the larger batch
  const bool f32 = ctx->precision == GPAK_F32;
  int batch = f32 ? 65536 : 16384;
  if (ctx->sched.pred_batch > 0) batch = std::max(2 * PB, ctx->sched.pred_batch / (2 * PB) * (2 * PB));
  // keep the cross-kernel batch under ~8 GiB
  while (batch > 2 * PB && (size_t)batch * Np * (f32 ? sizeof(float) : sizeof(double)) > ((size_t)8 << 30)) batch /= 2;
  batch = batch / (2 * PB) * (2 * PB);
  long Mp = (M + 2 * PB - 1) / (2 * PB) * (2 * PB);   // 256-row granularity: the fp32 GEMM's workgroup tile
  const int cap = (int)std::min<long>(Mp, batch);
  int rc = ensure_predict_bufs(ctx, cap, var != nullptr);
  if (rc) return rc;
  if (f32 && var && (rc = ensure_f32_factor(ctx))) return rc;
  hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[6];
  GPAK_HIP(hipEventRecord(e0, st));

  // pooled mean over train u (all) test points: Kernel.cpp:1391-1392 with X1 = Xinp, X2 = Xin
  double s2[4] = {0, 0, 0, 0};
  for (int k = 0; k < ctx->d; k++)
    for (long i = 0; i < M; i++) s2[k] += Xte[i + (size_t)k * M];
  KernParams kp = ctx->kp;
  kp.d = ctx->d;
  if (pool_sum) gpak_pooled_mean(ctx->xsum, N, pool_sum, pool_M, kp.mu);
  else gpak_pooled_mean(ctx->xsum, N, s2, M, kp.mu);
  gpak_launch_transform(st, ctx->dX, Np, N, kp, ctx->Upred);

  const double kD = ctx->kdiag;  // diag_Compute of the composition, Kernel.cpp:127-136, 780-783, 328-332
  kp.white = 0.0;                // Kern_White contributes nothing to a train x test block (Kernel.cpp:260-262)
  double *dMean = ctx->dPv, *dSq = ctx->dPv + cap;
  std::vector<double> hsq;
  for (long b0 = 0; b0 < M; b0 += cap) {
    const int mb = (int)std::min<long>(cap, M - b0);
    const int mbp = (mb + 2 * PB - 1) / (2 * PB) * (2 * PB);
    GPAK_HIP(hipMemsetAsync(ctx->dXte, 0, sizeof(double) * 4 * (size_t)cap, st));
    for (int k = 0; k < ctx->d; k++)
      GPAK_HIP(hipMemcpyAsync(ctx->dXte + (size_t)k * cap, Xte + (size_t)k * M + b0, sizeof(double) * mb,
                              hipMemcpyHostToDevice, st));
    gpak_launch_transform(st, ctx->dXte, cap, mb, kp, ctx->Tq);
    // _postMean: mu_t = Alpha . kX(:,t)
    int splits = gpak_kmatvec_splits(N, mb);
    gpak_launch_kmatvec(st, ctx->Upred, 0, N, ctx->dAlpha, ctx->Tq, kp, ctx->dPart, splits, dMean);
    GPAK_HIP(hipMemcpyAsync(mean + b0, dMean, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    if (var) {
      // test-major batch, k-columns `ldw` apart: a power-of-two stride (cap = 65536 floats = 256 KiB) puts every k-column
      // of a row tile on the same L2 channel -- skewed by 256 B like the fp64 matrix
      const long ldw = cap + (f32 ? 64L : 32L) * std::max(0, ctx->sched.pred_ld_skew);
      int vs = std::max(1, std::min(64, Np / 512));
      int cps = (Np + vs - 1) / vs;
      if (f32) {
        // fp32 arithmetic for the M-proportional work (cross-kernel, substitution, row sums);
        // the cross-kernel uses the direct distance form (cancellation form is meaningless in fp32)
        float *Wf = reinterpret_cast<float *>(ctx->dWt.p);
        gpak_launch_fill_f32(st, ctx->Tq, ctx->Upred, mbp, Np, kp, Wf, ldw);
        const GpakFsF32 fs = {st, ctx->dLf, ctx->ldLf, ctx->dInvf};
        std::vector<int> lv;
        for (int v : ctx->sched.fs_levels) if (v > 0) lv.push_back(v);
        gpak_forward_subst_f32(fs, Wf, ldw, mbp, Np, lv);
        gpak_launch_rowsumsq_f32(st, Wf, ldw, mbp, Np, vs, ctx->dPart, cap);
      } else {
        gpak_launch_fill(st, ctx->Tq, ctx->Upred, mbp, Np, kp, 1.0, 0.0, 0.0, 0, ctx->dWt, ldw, nullptr);
        forward_subst_batch(ctx, ctx->dWt, ldw, mbp);
        hipLaunchKernelGGL(gpak_rowsumsq_part_f64, dim3((mbp + 255) / 256, vs), dim3(256), 0, st, ctx->dWt, ldw,
                           mbp, Np, cps, ctx->dPart, cap);
      }
      gpak_launch_sum_splits(st, ctx->dPart, cap, vs, mb, dSq);
      hsq.resize(mb);
      GPAK_HIP(hipMemcpyAsync(hsq.data(), dSq, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
      GPAK_HIP(hipStreamSynchronize(st));
      // varSigma = kD - sum(LKs % kX) with LKs = sW . B^-1 . sW kX   (GP_Utils.cpp:985-999)
      for (int i = 0; i < mb; i++) var[b0 + i] = kD - hsq[i] / ctx->sn2;
    }
  }
  GPAK_HIP(hipEventRecord(e1, st));
  GPAK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, e0, e1));
  ctx->times.predict_ms = ms;
  return GPAK_OK;
}

// Block-support prediction (gpak_predict_block / gpak_block_cross): block b = the nd points Xd[b * nd .. b * nd + nd).
//   kbar_b = (1/nd) sum_a k(X, x_{b,a})                       the averaged fill, test-major like the point path's batch
//   mean_b = kbar_b . alpha                                   from the stored batch, before the substitution overwrites it
//   var_b  = max(0, kbb_b - |L^-1 kbar_b|^2 / sn2) [+ sn2/nd]  ONE substitution per block, not one per point
// Same batch loop, buffers, substitution and row sums as gpak_predict_impl; everything fp64 whatever the context's
// precision.  Kbar_host (N x M, column-major) set: only the averaged fill runs and its batches are copied out.
int gpak_predict_block_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, double *mean, double *var, int flags,
                            double *Kbar_host) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, d = ctx->d;
  KernParams kp = ctx->kp;
  kp.d = d;
  int batch = 16384;   // blocks per batch
  if (ctx->sched.pred_batch > 0) batch = std::max(2 * PB, ctx->sched.pred_batch / (2 * PB) * (2 * PB));
  while (batch > 2 * PB && (size_t)batch * Np * sizeof(double) > ((size_t)8 << 30)) batch /= 2;
  // raw (4) and transformed (GPAK_PT per term) coordinates of the batch's points: about 1 GiB at most
  const size_t per_block = sizeof(double) * (size_t)nd * (4 + GPAK_PT * (size_t)kp.nterms);
  while (batch > 2 * PB && (size_t)batch * per_block > ((size_t)1 << 30)) batch /= 2;
  batch = batch / (2 * PB) * (2 * PB);
  const long Mp = (M + 2 * PB - 1) / (2 * PB) * (2 * PB);
  const int cap = (int)std::min<long>(Mp, batch);
  if ((size_t)cap * nd > ((size_t)1 << 30)) { ctx->err = "too many discretisation points per block"; return GPAK_EINVAL; }
  int rc = ensure_predict_bufs(ctx, cap, true);
  if (rc) return rc;
  if ((rc = ensure_block_points(ctx, (size_t)cap * nd, kp.nterms))) return rc;
  hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[6];
  GPAK_HIP(hipEventRecord(e0, st));

  // pooled mean over the training set and all M * nd points, as gpak_predict on the flattened set
  const long Mn = M * nd;
  double s2[4] = {0, 0, 0, 0};
  for (int k = 0; k < d; k++)
    for (long i = 0; i < Mn; i++) s2[k] += Xd[i + (size_t)k * Mn];
  gpak_pooled_mean(ctx->xsum, N, s2, Mn, kp.mu);
  gpak_launch_transform(st, ctx->dX, Np, N, kp, ctx->Upred);

  const bool latent = flags & GPAK_BLOCK_LATENT;
  const long ldw = cap + 32L * std::max(0, ctx->sched.pred_ld_skew);
  const int vs = std::max(1, std::min(64, Np / 512));
  const int cps = (Np + vs - 1) / vs;
  double *dMean = ctx->dPv, *dSq = ctx->dPv + cap, *dKbb = ctx->dXte;   // dXte (4 x cap) is free on this path
  std::vector<double> hsq, hkbb, hK;
  for (long b0 = 0; b0 < M; b0 += cap) {
    const int mb = (int)std::min<long>(cap, M - b0);
    const int mbp = (mb + 2 * PB - 1) / (2 * PB) * (2 * PB);
    const long xs = (long)mb * nd;
    for (int k = 0; k < d; k++)
      GPAK_HIP(hipMemcpyAsync(ctx->dXblk + (size_t)k * xs, Xd + (size_t)k * Mn + (size_t)b0 * nd, sizeof(double) * xs,
                              hipMemcpyHostToDevice, st));
    gpak_launch_transform_blocks(st, ctx->dXblk, xs, mb, nd, cap, kp, ctx->dTblk);
    gpak_launch_fill_blocks(st, ctx->dTblk, cap, mb, nd, ctx->Upred, mbp, Np, kp, ctx->dWt, ldw);
    if (Kbar_host) {
      hK.resize((size_t)mb * N);
      GPAK_HIP(hipMemcpy2DAsync(hK.data(), sizeof(double) * mb, ctx->dWt, sizeof(double) * ldw, sizeof(double) * mb, N,
                                hipMemcpyDeviceToHost, st));
      GPAK_HIP(hipStreamSynchronize(st));
      for (int i = 0; i < mb; i++)
        for (int j = 0; j < N; j++) Kbar_host[j + (size_t)(b0 + i) * N] = hK[i + (size_t)j * mb];
      continue;
    }
    hipLaunchKernelGGL(gpak_rowdot_part_f64, dim3((mb + 255) / 256, vs), dim3(256), 0, st, ctx->dWt, ldw, mb, N, cps,
                       ctx->dAlpha, ctx->dPart, cap);   // columns >= N are padding
    gpak_launch_sum_splits(st, ctx->dPart, cap, vs, mb, dMean);
    GPAK_HIP(hipMemcpyAsync(mean + b0, dMean, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    if (var) {
      forward_subst_batch(ctx, ctx->dWt, ldw, mbp);
      hipLaunchKernelGGL(gpak_rowsumsq_part_f64, dim3((mbp + 255) / 256, vs), dim3(256), 0, st, ctx->dWt, ldw, mbp, Np,
                         cps, ctx->dPart, cap);
      gpak_launch_sum_splits(st, ctx->dPart, cap, vs, mb, dSq);
      gpak_launch_block_self(st, ctx->dTblk, cap, mb, nd, kp, dKbb);
      hsq.resize(mb); hkbb.resize(mb);
      GPAK_HIP(hipMemcpyAsync(hsq.data(), dSq, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
      GPAK_HIP(hipMemcpyAsync(hkbb.data(), dKbb, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
      GPAK_HIP(hipStreamSynchronize(st));
      for (int i = 0; i < mb; i++) {
        const double lat = std::max(0.0, hkbb[i] - hsq[i] / ctx->sn2);
        var[b0 + i] = latent ? lat : lat + ctx->sn2 / nd;
      }
    }
  }
  GPAK_HIP(hipEventRecord(e1, st));
  GPAK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, e0, e1));
  ctx->times.predict_ms = ms;
  return GPAK_OK;
}

// ---------------------------------------------------------------------------------------
// Joint posterior of M blocks and conditional simulation (gpak_predict_joint / gpak_sample_joint).  The block path's
// steps, unchanged, up to and including the means, with ALL M blocks in one batch (cap = M rounded up to 256):
//   points -> gpak_transform_blocks_f64 -> averaged fill into dWt -> row dots with alpha = the means;
// then W = Kbar^T L^-T by forward_subst_batch, the prior covariance between the block averages into dC
// (gpak_fillblk_pair_f64, gram.hip), and ONE product dC -= W W^T / sn2 over the lower tiles (the padding rows of dWt are
// zero, so the padding of dC keeps its identity).  The lower triangle is copied out and mirrored on the host:
// cov_host is symmetric by construction.
// Sampling: the nugget rides on the pair fill's diagonal term; dC is factored in place by the right-looking loop a
// rank of the 1-D multi-GPU schedule runs on its columns -- gpak_factor_panel (512 columns, clipped) and a K = W update
// of the lower tiles to its right -- with inverse blocks and an info word of its own; then Z = mean 1^T + Lc Xi by
// gpak_joint_trmm_f64 below.  Everything is queued on the context's stream; one host synchronisation per copy-out.
// ---------------------------------------------------------------------------------------
#define JOINT_SCOLS 8   // realisations per thread of the triangular product
// Z[i, s] = mean[i] + sum_{k <= i} Lc[i, k] Xi[k, s]: one thread per row (coalesced reads of a column of Lc; Xi[k, s] is
// wave-uniform), JOINT_SCOLS realisations per thread, k ascending in one fma chain per (i, s).  M^2 S flops on the
// vector unit: noise beside the N-proportional work of the call.
__global__ __launch_bounds__(256) void gpak_joint_trmm_f64(const double *__restrict__ Lc, long ld, int M,
                                                            const double *__restrict__ Xi, const double *__restrict__ mean,
                                                            int S, double *__restrict__ Z) {
  const int i = blockIdx.x * 256 + threadIdx.x, s0 = blockIdx.y * JOINT_SCOLS;
  if (i >= M) return;
  double acc[JOINT_SCOLS];
#pragma unroll
  for (int u = 0; u < JOINT_SCOLS; u++) acc[u] = 0.0;
  for (int k = 0; k <= i; k++) {
    const double l = Lc[i + (size_t)k * ld];
#pragma unroll
    for (int u = 0; u < JOINT_SCOLS; u++)
      if (s0 + u < S) acc[u] = fma(l, Xi[k + (size_t)(s0 + u) * M], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < JOINT_SCOLS; u++)
    if (s0 + u < S) Z[i + (size_t)(s0 + u) * M] = mean[i] + acc[u];
}

int gpak_joint_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, double *mean, double *cov_host, int flags,
                    const double *Xi, int S, double nugget, double *Z) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, d = ctx->d;
  KernParams kp = ctx->kp;
  kp.d = d;
  const long Mp = (M + 2 * PB - 1) / (2 * PB) * (2 * PB);
  // the block path's budget for the raw and transformed points of a batch, here of the one batch there is
  const size_t per_block = sizeof(double) * (size_t)nd * (4 + GPAK_PT * (size_t)kp.nterms);
  if (Mp > (1L << 24) || (size_t)Mp * per_block > ((size_t)1 << 30)) {
    ctx->err = "the blocks' discretisation points exceed the 1 GiB point budget of one batch (the joint calls hold all M blocks at once)";
    return GPAK_EINVAL;
  }
  const int cap = (int)Mp;
  const bool sample = Xi != nullptr, prior = !sample && (flags & GPAK_JOINT_PRIOR);
  const bool want_c = sample || cov_host;
  int rc = ensure_predict_bufs(ctx, cap, true);
  if (rc) return rc;
  if ((rc = ensure_block_points(ctx, (size_t)cap * nd, kp.nterms))) return rc;
  const long ldw = cap + 32L * std::max(0, ctx->sched.pred_ld_skew), ldc = ldw;   // the same 256-byte skew
  if (want_c && (rc = ensure_joint_cov(ctx, cap, ldc))) return rc;
  if (sample && ctx->dZ.n < (size_t)M * S) {   // dZ comes last: where it stands, dXi does
    ctx->dXi.release(); ctx->dZ.release();
    if (!ctx->dXi.reserve((size_t)M * S) || !ctx->dZ.reserve((size_t)M * S)) {
      ctx->err = "device allocation failed for the normals and the realisations";
      return GPAK_ENOMEM;
    }
  }
  hipEvent_t e0 = ctx->ev[5], e1 = ctx->ev[6];
  GPAK_HIP(hipEventRecord(e0, st));

  // pooled mean over the training set and all M * nd points, as gpak_predict_block
  const long Mn = M * nd;
  double s2[4] = {0, 0, 0, 0};
  for (int k = 0; k < d; k++)
    for (long i = 0; i < Mn; i++) s2[k] += Xd[i + (size_t)k * Mn];
  gpak_pooled_mean(ctx->xsum, N, s2, Mn, kp.mu);
  gpak_launch_transform(st, ctx->dX, Np, N, kp, ctx->Upred);

  const int mb = (int)M;
  const int vs = std::max(1, std::min(64, Np / 512));
  const int cps = (Np + vs - 1) / vs;
  double *dMean = ctx->dPv;
  for (int k = 0; k < d; k++)
    GPAK_HIP(hipMemcpyAsync(ctx->dXblk + (size_t)k * Mn, Xd + (size_t)k * Mn, sizeof(double) * Mn, hipMemcpyHostToDevice, st));
  gpak_launch_transform_blocks(st, ctx->dXblk, Mn, mb, nd, cap, kp, ctx->dTblk);
  gpak_launch_fill_blocks(st, ctx->dTblk, cap, mb, nd, ctx->Upred, cap, Np, kp, ctx->dWt, ldw);
  hipLaunchKernelGGL(gpak_rowdot_part_f64, dim3((mb + 255) / 256, vs), dim3(256), 0, st, ctx->dWt, ldw, mb, N, cps,
                     ctx->dAlpha, ctx->dPart, cap);   // columns >= N are padding
  gpak_launch_sum_splits(st, ctx->dPart, cap, vs, mb, dMean);
  if (mean) GPAK_HIP(hipMemcpyAsync(mean, dMean, sizeof(double) * mb, hipMemcpyDeviceToHost, st));

  int info = 0;
  const int init = 0x7fffffff;
  if (want_c) {
    const bool latent = flags & GPAK_JOINT_LATENT;
    const double diag = kp.white / nd + (latent ? 0.0 : ctx->sn2 / nd) + (sample ? nugget : 0.0);
    gpak_launch_fill_block_pairs(st, ctx->dTblk, cap, mb, nd, kp, diag, ctx->dC, ldc);
    if (!prior) {
      forward_subst_batch(ctx, ctx->dWt, ldw, cap);
      // the SYRK: dC -= W W^T / sn2 on the lower 128-tiles
      gpak_launch_gemm_nt(st, cap / PB, cap / PB, Np, -1.0 / ctx->sn2, ctx->dWt, ldw, ctx->dWt, ldw, 1.0, ctx->dC, ldc, 0, 0,
                          true, false);
    }
  }
  if (cov_host) {
    // rows [c, M) of column c; mirrored below
    GPAK_HIP(hipMemcpy2DAsync(cov_host, sizeof(double) * M, ctx->dC, sizeof(double) * ldc, sizeof(double) * M, M,
                              hipMemcpyDeviceToHost, st));
  }
  if (sample) {
    GPAK_HIP(hipMemcpyAsync(ctx->dCinfo, &init, sizeof(int), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(ctx->dXi, Xi, sizeof(double) * (size_t)M * S, hipMemcpyHostToDevice, st));
    for (int J = 0; J < cap; J += 512) {
      const int W = std::min(512, cap - J), c0 = J + W, mt = (cap - c0) / PB;
      gpak_factor_panel(st, ctx->dC, ldc, cap, J, W, ctx->dCinv, ctx->dCinfo, true, false, ctx->sched.potrf_co);
      if (mt > 0) {
        const double *P = ctx->dC + c0 + (size_t)J * ldc;
        gpak_launch_gemm_nt(st, mt, mt, W, -1.0, P, ldc, P, ldc, 1.0, ctx->dC + c0 + (size_t)c0 * ldc, ldc, 0, 0, true, false);
      }
    }
    hipLaunchKernelGGL(gpak_joint_trmm_f64, dim3((mb + 255) / 256, (S + JOINT_SCOLS - 1) / JOINT_SCOLS), dim3(256), 0, st,
                       ctx->dC, ldc, mb, ctx->dXi, dMean, S, ctx->dZ);
    GPAK_HIP(hipMemcpyAsync(&info, ctx->dCinfo, sizeof(int), hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipMemcpyAsync(Z, ctx->dZ, sizeof(double) * (size_t)M * S, hipMemcpyDeviceToHost, st));
  }
  GPAK_HIP(hipEventRecord(e1, st));
  GPAK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, e0, e1));
  ctx->times.predict_ms = ms;
  if (cov_host)
    for (long c = 0; c < M; c++)
      for (long r = c + 1; r < M; r++) cov_host[c + (size_t)r * M] = cov_host[r + (size_t)c * M];
  if (sample && info != init) {
    ctx->err = "C + nugget I of the blocks is not positive definite: its factorisation fails at column " + std::to_string(info) +
               " (raise the nugget)";
    return GPAK_ENOTPD;
  }
  return GPAK_OK;
}

// solve_chol with k right-hand sides held on the host (GP_Utils.cpp:841-845)
int gpak_solve_chol_impl(gpak_ctx *ctx, double *X_host, int k) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np;
  double *w0 = ctx->dWork, *w1 = ctx->dWork + Np, *w2 = ctx->dWork + 2 * (size_t)Np;
  ctx->state.work_vectors_overwritten();
  for (int c = 0; c < k; c++) {
    GPAK_HIP(hipMemsetAsync(w0, 0, sizeof(double) * Np, st));
    GPAK_HIP(hipMemcpyAsync(w0, X_host + (size_t)c * N, sizeof(double) * N, hipMemcpyHostToDevice, st));
    gpak_launch_trsv_fwd(st, Np, ctx->dM, ctx->ld, ctx->dInv, w0, w1);
    gpak_backsolve(ctx, st, w1, w2, ctx->dWork + 3 * (size_t)Np);
    GPAK_HIP(hipMemcpyAsync(X_host + (size_t)c * N, w2, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  }
  GPAK_HIP(hipStreamSynchronize(st));
  return GPAK_OK;
}

