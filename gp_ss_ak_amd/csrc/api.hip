// api.hip -- the C-ABI of libgpak_hip.so (see include/gpak.h for the contract and the
// reference members each entry point replaces).  Orchestration only; kernels live in
// gram.hip / gemm.hip / potrf.hip / solve.hip / predict.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../include/gpak_cv_folds.h"
#include "../../include/gpak_cv_folds_grad.h"
#include "../../include/gpak_cv_groups_grad.h"
#include "multi.h"

#define GPAK_MULTI_ERR(rc_) do { int v_ = (rc_); if (v_) ctx->err = gpak_multi_error(ctx->multi); return v_; } while (0)

static std::string g_global_err;

// ---- the two tuning sets (GpakSchedule in potrf_plan.h: copied by every context; GpakKernelTuning in gpak_internal.h:
// process-wide): defaults, overridden once by the GPAK_* environment ------------------
struct Tuning {
  GpakSchedule sched;
  GpakKernelTuning kern;
};
static Tuning read_tuning_env() {
  Tuning tn;
  GpakSchedule &t = tn.sched;
  GpakKernelTuning &k = tn.kern;
  auto geti = [](const char *name, int &v) { if (const char *e = getenv(name)) v = atoi(e); };
  auto getb = [](const char *name, bool &v) { if (const char *e = getenv(name)) v = atoi(e) != 0; };
  geti("GPAK_NB_OUTER", t.nb_outer);
  geti("GPAK_NB_WIDE", t.nb_wide); t.nb_wide = t.nb_wide / GPAK_TILE * GPAK_TILE;
  geti("GPAK_NB_WIDE_ROWS", t.nb_wide_rows);
  geti("GPAK_NB_XWIDE", t.nb_xwide); t.nb_xwide = t.nb_xwide / GPAK_TILE * GPAK_TILE;
  geti("GPAK_NB_XWIDE_ROWS", t.nb_xwide_rows);
  getb("GPAK_FIRST_NARROW", t.first_narrow);
  geti("GPAK_TAIL_ROWS", t.tail_rows);
  geti("GPAK_TAIL_MAX_NP", t.tail_queue_max_np);
  getb("GPAK_SUB_NEXT", t.sub_next);
  geti("GPAK_NEXT_SPLIT_ROWS", t.next_split_rows);
  getb("GPAK_INV512", t.inv512);
  geti("GPAK_BWD_FUSED", t.bwd_fused);
  geti("GPAK_SBASE_ROWS", k.sbase_rows);
  geti("GPAK_BWD_BLOCK", t.bwd_block);
  getb("GPAK_LOOKAHEAD", t.lookahead);
  getb("GPAK_FWD_IN_FACTOR", t.fwd_in_factor);
  geti("GPAK_POTRF_CO", t.potrf_co); k.potrf_co = t.potrf_co;
  geti("GPAK_TAIL_MASK", t.tail_mask);
  geti("GPAK_TAIL_MASK_STRIDE", t.tail_mask_stride);
  getb("GPAK_BULK_QUEUE", t.bulk_queue);
  if (const char *e = getenv("GPAK_LD_PAD")) t.ld_pad = atol(e) / 2 * 2;
  geti("GPAK_GEMM_SMALL", k.gemm_small);
  geti("GPAK_GEMM_SMALL_ROWS", k.gemm_small_rows);
  geti("GPAK_SUPER_LR", k.super_lr);
  getb("GPAK_BULK_TICKETS", t.bulk_tickets);
  geti("GPAK_BULK_SURPLUS", t.bulk_surplus);
  getb("GPAK_FILL_FAST", k.fill_fast);
  getb("GPAK_KMV_SYM", k.kmv_sym);
  if (const char *e = getenv("GPAK_F32_ACC")) k.f32_wide = strcmp(e, "plain") != 0;
  geti("GPAK_F32_RSD", k.f32_rsd);
  geti("GPAK_F32_TILE", k.f32_tile);
  geti("GPAK_PRED_BATCH", t.pred_batch);
  geti("GPAK_PRED_LD_SKEW", t.pred_ld_skew);
  if (const char *e = getenv("GPAK_FS_LEVELS_F32")) {   // "128,512,...": ascending, each a multiple of the one before
    int n = 0, lv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const char *p = e; *p && n < 8;) {
      const int v = atoi(p);
      if (v >= GPAK_TILE && v % GPAK_TILE == 0 && (n == 0 ? v == GPAK_TILE : v > lv[n - 1] && v % lv[n - 1] == 0)) lv[n++] = v;
      while (*p && *p != ',') p++;
      if (*p == ',') p++;
    }
    if (n > 0) memcpy(t.fs_levels, lv, sizeof(lv));
  }
  return tn;
}
static Tuning &tuning_storage() {
  static Tuning t = read_tuning_env();
  return t;
}
const GpakKernelTuning &gpak_tuning() { return tuning_storage().kern; }
extern "C" void gpak_reload_tuning(void) { tuning_storage() = read_tuning_env(); }

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

int gpak_alloc_points(gpak_ctx *ctx, DevPointsBuf &p, int cap) {
  if (p.reserve(cap)) return GPAK_OK;
  ctx->err = "hipMalloc(points) failed";
  return GPAK_ENOMEM;
}

// sigInv = Rot * lambda * Rot^T, Kernel.cpp:1399-1425 (host, 3x3)
void gpak_build_siginv(const double *e, double *A) {
  const double lam[3] = {e[1], e[3], e[5]};
  double R[3][3];
  gpak_rot_tables(e, R, nullptr);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += R[r][k] * lam[k] * R[c][k];
      A[r + c * 3] = s;
    }
}

// HybKerns composition -> KernParams (Kernel.cpp:140-154 and the children's parameter lists; shared by gpak_set_kernel
// and by the distributed paths, which carry the composition as one serialized array: gpak_dev.h GPAK_DIST_HYB)
int gpak_build_kp(int nterms, const int *kinds, const double *pars, double bias, double white, int dist_mode,
                  KernParams *out, double *kdiag_out) {
  KernParams kp;
  memset(&kp, 0, sizeof(kp));
  if (nterms < 1 || nterms > GPAK_MAX_TERMS) return GPAK_EINVAL;
  kp.nterms = nterms;
  double kdiag = bias + white;
  const double *p = pars;
  for (int t = 0; t < nterms; t++) {
    KernTerm &T = kp.term[t];
    if (kinds[t] == GPAK_KERN_EXPANS) {
      gpak_build_siginv(p, T.A);
      T.a33 = p[7];
      T.var2 = p[6] * p[6]; T.profile = GPAK_PROFILE_EXPSQRT;
      p += 8;
    } else if (kinds[t] == GPAK_KERN_EXP) {   // {Hayper_Euc_Exp, Sigma_Exp}, Kernel.cpp:576-600
      const double s = 1.0 / p[0];             // mlA: X * hyp^-2 on one side == both sides scaled by 1/hyp
      T.A[0] = T.A[4] = T.A[8] = T.a33 = s;  // EuclDist treats every input column alike (Kernel.cpp:1356-1362)
      T.var2 = p[1] * p[1]; T.profile = GPAK_PROFILE_EXPSQRT;
      p += 2;
    } else if (kinds[t] == GPAK_KERN_RBF) {   // {Hayper_Euc_RBF, inverseWidth_RBF, Sigma_RBF}, Kernel.cpp:411-428
      const double s = 1.0 / p[0];
      T.A[0] = T.A[4] = T.A[8] = T.a33 = s;
      T.iw = p[1]; T.var2 = p[2] * p[2]; T.profile = GPAK_PROFILE_RBF;
      p += 3;
    } else {
      return GPAK_EINVAL;
    }
    kdiag += T.var2;
  }
  kp.bias = bias; kp.white = white; kp.mode = dist_mode;
  *out = kp;
  if (kdiag_out) *kdiag_out = kdiag;
  return GPAK_OK;
}

// pooled mean of X1 u X2 exactly as Kernel.cpp:1391-1392 computes it
void gpak_pooled_mean(const double *s1, long n, const double *s2, long m, double *mu) {
  for (int k = 0; k < 4; k++) {  // s1, s2, mu hold four column sums (the 4th is 0 for 3-D inputs)
    double mX1 = (double)n / (double)(n + m) * s1[k] / (double)n;
    mu[k] = (double)m / (double)(n + m) * s2[k] / (double)m + mX1;
  }
}

// The buffers that go with a training set: sized by N, and meaningless under another one.  The prediction buffers, the
// reduction scratch and the ticket ring are kept: they only grow.
static void release_train(gpak_ctx *ctx) {
  for (DevBuf<double> *b : {&ctx->dX, &ctx->dy, &ctx->dM, &ctx->dInv, &ctx->dInv512, &ctx->dT512, &ctx->dAlpha, &ctx->dWork, &ctx->dF,
                            &ctx->dG, &ctx->dBinv, &ctx->dGpart, &ctx->dLoo})
    b->release();
  ctx->U.release();
  ctx->dLf.release();
  ctx->dInvf.release();
  ctx->N = ctx->Np = 0;
  ctx->state.new_training_set();
}

// events and streams, after the buffers of the context have freed themselves.  A group's context has none of either.
gpak_queues::~gpak_queues() {
  for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
  for (auto e : ev_pool) hipEventDestroy(e);
  for (auto e : ev_sync) hipEventDestroy(e);
  for (auto e : ev_cvf) hipEventDestroy(e);
  for (hipStream_t s : {stream_hi, stream_fs, stream_x, stream_tail, stream_bulk, stream}) if (s) hipStreamDestroy(s);
}

extern "C" {

const char *gpak_global_error(void) { return g_global_err.c_str(); }

int gpak_create(gpak_ctx **out, int device, int precision) {
  if (!out) return GPAK_EINVAL;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_global_err = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                   " (libgpak_hip has no CPU fallback)";
    return GPAK_EHIP;
  }
  if (device < 0 || device >= count) { g_global_err = "device ordinal out of range"; return GPAK_EINVAL; }
  if (precision != GPAK_F64 && precision != GPAK_F32) { g_global_err = "precision must be GPAK_F64 or GPAK_F32"; return GPAK_EINVAL; }
  if ((e = hipSetDevice(device)) != hipSuccess) { g_global_err = hipGetErrorString(e); return GPAK_EHIP; }
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) { g_global_err = hipGetErrorString(e); return GPAK_EHIP; }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    g_global_err = std::string("device is ") + prop.gcnArchName + ", libgpak_hip is built for gfx950 only";
    return GPAK_EHIP;
  }
  gpak_ctx *ctx = new gpak_ctx();
  ctx->sched = tuning_storage().sched;
  ctx->device = device;
  ctx->precision = precision;
  memset(&ctx->times, 0, sizeof(ctx->times));
  int prio_lo = 0, prio_hi = 0;
  hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // numerically lower = higher priority
  if ((e = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_lo)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&ctx->stream_hi, hipStreamNonBlocking, prio_hi)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&ctx->stream_fs, hipStreamNonBlocking, prio_hi)) != hipSuccess) {
    g_global_err = hipGetErrorString(e); delete ctx; return GPAK_EHIP;
  }
  ctx->cu_count = prop.multiProcessorCount;
  // ORDER OF CREATION MATTERS: the two CU-masked queues below are made before the side stream, so that they are the
  // device's 4th and 5th queue.  Measured (profiles/r06_tail_before.txt): whichever of them was the
  // 6th queue of the process handed work over in 60-800 us instead of 13 (the bulk queue until round 5: N = 32768
  // 2 ms slower than without any tail queue; the tail queue when the two are swapped: N = 8192 twice as slow).
  // a copy of the main stream that may not use the first GPAK_TAIL_MASK (default 8) compute units; the bulk
  // updates of the chain-bound tail of the factorisation go there so that the panel chain finds idle CUs
  {
    const int skip = ctx->sched.tail_mask;           // 0 switches it off; measured: 8 CUs, rows <= 12288: 183.4 -> 181.2 ms
    if (skip > 0 && skip < prop.multiProcessorCount) {
      std::vector<uint32_t> mask((prop.multiProcessorCount + 31) / 32, 0xffffffffu);
      const int stride = ctx->sched.tail_mask_stride;
      for (int c = 0; c < skip; c++) { const int bit = (c * stride) % prop.multiProcessorCount; mask[bit / 32] &= ~(1u << (bit % 32)); }
      if (hipExtStreamCreateWithCUMask(&ctx->stream_tail, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        ctx->stream_tail = nullptr;
        (void)hipGetLastError();
      }
    }
  }
  // The bulk trailing updates get a queue of their own, created through the same call as the tail's but with every CU
  // enabled.  Measured, not understood: on the context's ordinary low-priority stream the dependants of "bulk update b
  // done" (update b+1 in the same stream, the next column's update in the panel stream) start 75-125 us after it in
  // the middle of the factorisation with nothing else running, on a queue created by hipExtStreamCreateWithCUMask
  // 23 us: 175.1 -> 172.8 ms per factorisation at N = 32768 (same-box A/B).  The same for the panel stream (which then
  // loses its priority): 203 ms; for the forward-substitution or the main stream: +1.3 ms.  GPAK_BULK_QUEUE=0: off.
  if (ctx->sched.bulk_queue) {
    std::vector<uint32_t> mask((prop.multiProcessorCount + 31) / 32, 0xffffffffu);
    if (hipExtStreamCreateWithCUMask(&ctx->stream_bulk, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
      ctx->stream_bulk = nullptr;
      (void)hipGetLastError();
    }
  }
  // the side stream (GPAK_SUB_NEXT, GPAK_NEXT_SPLIT_ROWS: unused by the default schedule) comes last
  if ((e = hipStreamCreateWithPriority(&ctx->stream_x, hipStreamNonBlocking, prio_hi)) != hipSuccess) {
    g_global_err = hipGetErrorString(e); delete ctx; return GPAK_EHIP;
  }
  for (int i = 0; i < 10; i++) hipEventCreate(&ctx->ev[i]);
  if (!ctx->dRed.reserve(64) || !ctx->dInfo.reserve(4)) {
    g_global_err = "device allocation failed for the context's reduction scratch"; delete ctx; return GPAK_ENOMEM;
  }
  *out = ctx;
  return GPAK_OK;
}

int gpak_create_multi(gpak_ctx **out, int n_gpus, const int *devices, int precision) {
  if (!out || n_gpus < 1) return GPAK_EINVAL;
  *out = nullptr;
  if (precision != GPAK_F64 && precision != GPAK_F32) { g_global_err = "precision must be GPAK_F64 or GPAK_F32"; return GPAK_EINVAL; }
  gpak_multi *g = nullptr;
  int rc = gpak_multi_create(&g, n_gpus, devices, precision, g_global_err, nullptr);
  if (rc) return rc;
  gpak_ctx *ctx = new gpak_ctx();
  ctx->multi = g;
  ctx->precision = precision;
  memset(&ctx->times, 0, sizeof(ctx->times));
  *out = ctx;
  return GPAK_OK;
}

// TEST entry point (gpak_dist.h): the same group -- one host thread per rank, the in-process transport, the gpak_ctx
// surface of logLikelihood / alpha / gradient -- over caller-supplied engines, so that the thread-per-GPU host logic
// can be exercised (and run under ThreadSanitizer / AddressSanitizer) on a box without a GPU.
int gpak_create_multi_with_engines(gpak_ctx **out, int n_ranks, const gpak_dist_engine *const *engines) {
  if (!out || n_ranks < 1 || !engines) return GPAK_EINVAL;
  *out = nullptr;
  for (int r = 0; r < n_ranks; r++) if (!engines[r]) return GPAK_EINVAL;
  gpak_multi *g = nullptr;
  int rc = gpak_multi_create(&g, n_ranks, nullptr, GPAK_F64, g_global_err, engines);
  if (rc) return rc;
  gpak_ctx *ctx = new gpak_ctx();
  ctx->multi = g;
  ctx->precision = GPAK_F64;
  memset(&ctx->times, 0, sizeof(ctx->times));
  *out = ctx;
  return GPAK_OK;
}

void gpak_destroy(gpak_ctx *ctx) {
  if (!ctx) return;
  if (ctx->multi) { gpak_multi_destroy(ctx->multi); delete ctx; return; }
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  release_train(ctx);   // first, as ever; the other buffers go with the context, and its streams after them
  delete ctx;
}

const char *gpak_last_error(const gpak_ctx *ctx) { return ctx ? ctx->err.c_str() : g_global_err.c_str(); }

int gpak_set_option(gpak_ctx *ctx, int option, long value) {
  if (!ctx) return GPAK_EINVAL;
  if (ctx->multi) return GPAK_OK;   // schedule options of the single-GPU factorisation: nothing to set on a group
  switch (option) {
    case GPAK_OPT_MEMOISE: ctx->state.set_memoise(value != 0); return GPAK_OK;
    case GPAK_OPT_NB_OUTER:
      if (value < 128 || value % 128) { ctx->err = "nb_outer must be a positive multiple of 128"; return GPAK_EINVAL; }
      ctx->sched.nb_outer = (int)value;
      return GPAK_OK;
    case GPAK_OPT_PROFILE: ctx->profile = value != 0; return GPAK_OK;
    case GPAK_OPT_LOOKAHEAD: ctx->sched.lookahead = value != 0; return GPAK_OK;
    case GPAK_OPT_NB_WIDE:
      if (value < 0 || value % 128) { ctx->err = "nb_wide must be 0 or a multiple of 128"; return GPAK_EINVAL; }
      ctx->sched.nb_wide = (int)value;
      return GPAK_OK;
    case GPAK_OPT_NB_WIDE_ROWS: ctx->sched.nb_wide_rows = (int)value; return GPAK_OK;
    case GPAK_OPT_TAIL_ROWS: ctx->sched.tail_rows = (int)value; return GPAK_OK;
    case GPAK_OPT_FIRST_NARROW: ctx->sched.first_narrow = value != 0; return GPAK_OK;
    case GPAK_OPT_INV512: ctx->sched.inv512 = value != 0; return GPAK_OK;
    case GPAK_OPT_POTRF_CO:
      if (value < 0 || value > 2) { ctx->err = "potrf_co must be 0, 1 or 2"; return GPAK_EINVAL; }
      ctx->sched.potrf_co = (int)value;
      return GPAK_OK;
    case GPAK_OPT_PRED_BATCH: ctx->sched.pred_batch = (int)value; return GPAK_OK;
    case GPAK_OPT_TAIL_MAX_NP:
      if (value < 0) { ctx->err = "tail_queue_max_np must be 0 (no limit) or a size"; return GPAK_EINVAL; }
      ctx->sched.tail_queue_max_np = (int)value;
      return GPAK_OK;
    case GPAK_OPT_BWD_FUSED:
      if (value < 0 || value > 2) { ctx->err = "bwd_fused must be 0, 1 or 2"; return GPAK_EINVAL; }
      ctx->sched.bwd_fused = (int)value;
      return GPAK_OK;
    case GPAK_OPT_LOO_ROWS:
      if (value < 0 || value % 128) { ctx->err = "loo_rows must be 0 (the default) or a positive multiple of 128"; return GPAK_EINVAL; }
      ctx->loo_rows = (int)std::min(value, 1L << 30);
      return GPAK_OK;
  }
  ctx->err = "unknown option";
  return GPAK_EINVAL;
}

int gpak_set_train(gpak_ctx *ctx, const double *X, const double *y, int N, int d) {
  if (!ctx || !X || !y || N <= 0) return GPAK_EINVAL;
  if (ctx->multi) {   // N and d change only once the group has accepted the set: a refused call leaves the context as it was
    int v = gpak_multi_set_train(ctx->multi, X, y, N, d);
    if (v) { ctx->err = gpak_multi_error(ctx->multi); return v; }
    ctx->N = N; ctx->d = d;
    return GPAK_OK;
  }
  // d = 3: x, y, z; d = 4: + rock-type column with its own inverse width (Kernel.cpp:1411-1424)
  if (d != 3 && d != 4) { ctx->err = "inputs must have 3 or 4 columns"; return GPAK_ENOTIMPL; }
  GPAK_HIP(hipSetDevice(ctx->device));
  release_train(ctx);   // from here to the last line the context holds no training set: a failure leaves it that way
  const int Np = round_up(N, GPAK_TILE);
  long pad = Np >= 1024 ? 32 : 0;
  if (ctx->sched.ld_pad >= 0) pad = ctx->sched.ld_pad;
  const long ld = Np + pad;
  const int T = Np / GPAK_TILE;
  // width of the back substitution's explicit diagonal-block inverses (fixed per training set: it sizes dInv512)
  int bw = ctx->sched.bwd_block;
  if (bw != 512 && bw != 1024 && bw != 2048) bw = 512;
  const size_t nbw = (size_t)((Np + bw - 1) / bw);
  if (!ctx->dX.reserve(4 * (size_t)Np) || !ctx->dy.reserve(Np) || !ctx->dM.reserve((size_t)ld * Np) ||
      !ctx->dInv.reserve((size_t)T * 2 * GPAK_TILE * GPAK_TILE) || !ctx->dInv512.reserve(nbw * bw * bw) ||
      !ctx->dT512.reserve(2 * nbw * bw * bw) || !ctx->dAlpha.reserve(Np) || !ctx->dF.reserve(Np) ||
      // 70 Np doubles of vectors + the back substitution's scratch for the widest block ((8 + bw / 32) * bw for the
      // three-launch step, 34 * bw for the fused one: solve.hip)
      !ctx->dWork.reserve(70 * (size_t)Np + (size_t)std::max(8 + bw / 32, 34) * bw)) {
    ctx->err = "device allocation failed for the training set";
    release_train(ctx);
    return GPAK_ENOMEM;
  }
  int rc = gpak_alloc_points(ctx, ctx->U, Np);
  if (rc) { release_train(ctx); return rc; }
  GPAK_HIP(hipMemsetAsync(ctx->dX, 0, sizeof(double) * 4 * (size_t)Np, ctx->stream));
  GPAK_HIP(hipMemsetAsync(ctx->dy, 0, sizeof(double) * (size_t)Np, ctx->stream));
  // the inverse blocks are triangular: zero once, potrf128 only writes inside the triangles
  GPAK_HIP(hipMemsetAsync(ctx->dInv, 0, sizeof(double) * (size_t)T * 2 * GPAK_TILE * GPAK_TILE, ctx->stream));
  GPAK_HIP(hipMemsetAsync(ctx->dAlpha, 0, sizeof(double) * (size_t)Np, ctx->stream));
  for (int k = 0; k < d; k++)
    GPAK_HIP(hipMemcpyAsync(ctx->dX + (size_t)k * Np, X + (size_t)k * N, sizeof(double) * N,
                            hipMemcpyHostToDevice, ctx->stream));
  GPAK_HIP(hipMemcpyAsync(ctx->dy, y, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream));
  GPAK_HIP(hipStreamSynchronize(ctx->stream));
  // everything is in place: the context now holds the set
  ctx->N = N; ctx->Np = Np; ctx->ld = (int)ld; ctx->d = d;
  ctx->bwd_bw = bw;
  ctx->hX.assign(X, X + (size_t)N * d);
  ctx->xsum[3] = 0.0;
  for (int k = 0; k < d; k++) {
    double s = 0.0;
    for (int i = 0; i < N; i++) s += X[i + (size_t)k * N];
    ctx->xsum[k] = s;
  }
  memset(&ctx->times, 0, sizeof(ctx->times));
  ctx->times.n = N; ctx->times.n_padded = Np;
  return GPAK_OK;
}

int gpak_set_params(gpak_ctx *ctx, const double *expans, double bias, double sn2, int dist_mode) {
  if (!ctx || !expans) return GPAK_EINVAL;
  if (dist_mode != GPAK_DIST_EXPANSION && dist_mode != GPAK_DIST_DIRECT) { ctx->err = "bad dist_mode"; return GPAK_EINVAL; }
  if (ctx->multi) { ctx->sn2 = sn2; GPAK_MULTI_ERR(gpak_multi_set_params(ctx->multi, expans, bias, sn2, dist_mode)); }
  // "same" compares with what gpak_set_kernel stores too: the stored kernel must be the one this call builds (one ExpAns
  // term, no White), or a composition's factor and alpha would pass for this kernel's
  const bool same = ctx->have_params && ctx->expans_only && ctx->kp.white == 0.0 &&
                    memcmp(expans, ctx->expans, sizeof(double) * 8) == 0 && bias == ctx->bias && sn2 == ctx->sn2 &&
                    dist_mode == ctx->dist_mode;
  // Memoised: nothing is stored, every value being identical by the definition of "same" -- and kp.mu / kp.d, which
  // gpak_build_kp zeroes and gpak_ensure_U refills only when it rebuilds U, must stand with the U that is kept.
  if (same && ctx->state.memoise) { ctx->state.same_kernel(); return GPAK_OK; }
  // The one-ExpAns composition without White.  kdiag comes out as (bias + 0.0) + var2 where this function used to compute
  // var2 + bias: the same bits (x + 0.0 == x but for x = -0.0, and -0.0 + var2 == +0.0 + var2 for every var2 >= +0.0).
  const int kind = GPAK_KERN_EXPANS;
  return gpak_set_kernel(ctx, 1, &kind, expans, bias, 0.0, sn2, dist_mode);
}

// general composition: kinds[t] in {GPAK_KERN_EXPANS, GPAK_KERN_EXP, GPAK_KERN_RBF}, pars = the children's
// parameters concatenated in the reference's order (8 / 2 / 3 values)
int gpak_set_kernel(gpak_ctx *ctx, int nterms, const int *kinds, const double *pars, double bias, double white,
                    double sn2, int dist_mode) {
  if (!ctx || !kinds || !pars || nterms < 1 || nterms > GPAK_MAX_TERMS) return GPAK_EINVAL;
  if (dist_mode != GPAK_DIST_EXPANSION && dist_mode != GPAK_DIST_DIRECT) { ctx->err = "bad dist_mode"; return GPAK_EINVAL; }
  KernParams kp;
  double kdiag = 0.0;
  int rc = gpak_build_kp(nterms, kinds, pars, bias, white, dist_mode, &kp, &kdiag);
  if (rc) { ctx->err = "unknown kernel kind"; return rc; }   // before a group stores anything: a refused call changes nothing
  if (ctx->multi) { ctx->sn2 = sn2; GPAK_MULTI_ERR(gpak_multi_set_kernel(ctx->multi, nterms, kinds, pars, bias, white, sn2, dist_mode)); }
  {
    const double *p = pars;
    for (int t = 0; t < nterms; t++) {
      if (kinds[t] == GPAK_KERN_EXPANS) memcpy(ctx->expans, p, sizeof(double) * 8);  // the (single) ExpAns child, wherever it sits
      const int np = kinds[t] == GPAK_KERN_EXPANS ? 8 : kinds[t] == GPAK_KERN_EXP ? 2 : 3;
      memcpy(ctx->tpars[t], p, sizeof(double) * np);
      p += np;
      ctx->kinds[t] = kinds[t];
    }
  }
  ctx->kp = kp;
  ctx->kdiag = kdiag;
  ctx->expans_only = (nterms == 1 && kinds[0] == GPAK_KERN_EXPANS && white == 0.0);
  ctx->bias = bias; ctx->sn2 = sn2; ctx->dist_mode = dist_mode;
  ctx->have_params = true;
  ctx->state.new_kernel();
  return GPAK_OK;
}

}  // extern "C"

// transformed training points for the train x train Gram (pooled mean of X u X)
int gpak_ensure_U(gpak_ctx *ctx) {
  if (!ctx->N) { ctx->err = "no training set (gpak_set_train)"; return GPAK_ESTATE; }
  if (!ctx->have_params) { ctx->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
  if (ctx->state.points) return GPAK_OK;
  gpak_pooled_mean(ctx->xsum, ctx->N, ctx->xsum, ctx->N, ctx->kp.mu);
  ctx->kp.d = ctx->d;
  gpak_launch_transform(ctx->stream, ctx->dX, ctx->Np, ctx->N, ctx->kp, ctx->U);
  ctx->state.points_built();
  return GPAK_OK;
}

static int ensure_factor(gpak_ctx *ctx) {
  if (ctx->state.has(CtxState::FACTOR)) return GPAK_OK;
  int rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  GPAK_HIP(hipEventRecord(ctx->ev[0], st));
  // B = I + (sW sW') % K  with W = 1/sn2  (GP_Utils.cpp:898-902); lower tiles only
  gpak_launch_fill(st, ctx->U, ctx->U, ctx->Np, ctx->Np, ctx->kp, 1.0 / ctx->sn2, 1.0, 1.0, 1, ctx->dM,
                   ctx->ld, nullptr);
  ctx->state.factorisation_started();   // dM is about to hold another factor: nothing derived from the old one stands
  if (ctx->sched.fwd_in_factor) gpak_launch_scale(st, ctx->Np, ctx->dy, 1.0 / ctx->sn2, ctx->dWork);  // rhs = y/sn2
  GPAK_HIP(hipEventRecord(ctx->ev[1], st));
  rc = gpak_potrf_blocked(ctx);
  GPAK_HIP(hipEventRecord(ctx->ev[2], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[2]));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->times.gram_ms = ms;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
  ctx->times.factor_ms = ms;
  ctx->times.accumulated_ms[0] += ctx->times.gram_ms;
  ctx->times.accumulated_ms[1] += ctx->times.factor_ms;
  ctx->times.gram_bytes = 8.0 * ((double)ctx->Np * (ctx->Np + GPAK_TILE) / 2.0);
  if (rc == GPAK_ENOTPD)   // gpak_potrf_blocked has told ctx->state
    ctx->err = "B = I + K/sn2 is not positive definite at column " + std::to_string(ctx->state.failed_col);
  if (rc) return rc;
  // how a context substitutes backwards is settled here, by the options it factored under
  ctx->state.factorisation_succeeded(ctx->sched.fwd_in_factor, ctx->sched.inv512, ctx->sched.bwd_fused);
  return GPAK_OK;
}

static int ensure_alpha(gpak_ctx *ctx) {
  int rc = ensure_factor(ctx);
  if (rc) return rc;
  if (ctx->state.has(CtxState::ALPHA)) return GPAK_OK;
  hipStream_t st = ctx->stream;
  double *w0 = ctx->dWork, *w1 = ctx->dWork + ctx->Np;
  GPAK_HIP(hipEventRecord(ctx->ev[3], st));
  // alpha = (K + sn2 I)^-1 y = B^-1 (y / sn2)
  if (!ctx->state.z) {
    gpak_launch_scale(st, ctx->Np, ctx->dy, 1.0 / ctx->sn2, w0);
    gpak_launch_trsv_fwd(st, ctx->Np, ctx->dM, ctx->ld, ctx->dInv, w0, w1);
  }
  ctx->state.work_vectors_overwritten();  // the back substitution consumes w1
  gpak_backsolve(ctx, st, w1, ctx->dAlpha, ctx->dWork + 2 * (size_t)ctx->Np);
  GPAK_HIP(hipEventRecord(ctx->ev[4], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[4]));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
  ctx->times.solve_ms = ms;
  ctx->times.accumulated_ms[2] += ms;
  ctx->state.alpha_built();
  return GPAK_OK;
}

static int ensure_nlz(gpak_ctx *ctx) {
  int rc = ensure_alpha(ctx);
  if (rc) return rc;
  if (ctx->state.has(CtxState::NLZ)) return GPAK_OK;
  hipStream_t st = ctx->stream;
  double *f = ctx->dF;
  double *scratch = ctx->dWork + 4 * (size_t)ctx->Np;  // 64 * Np doubles available
  GPAK_HIP(hipEventRecord(ctx->ev[5], st));
  int splits = gpak_kmatvec_splits(ctx->N, ctx->N);
  gpak_launch_kmatvec(st, ctx->U, 0, ctx->N, ctx->dAlpha, ctx->U, ctx->kp, scratch, splits, f, 64);  // f = K*Alpha
  GPAK_HIP(hipEventRecord(ctx->ev[8], st));
  if (ctx->kp.white != 0.0) gpak_launch_axpy(st, ctx->N, ctx->kp.white, ctx->dAlpha, f);  // Kern_White diagonal
  gpak_launch_logdet(st, ctx->N, ctx->dM, ctx->ld, ctx->dRed);
  gpak_launch_nlz_terms(st, ctx->N, ctx->dy, f, ctx->dAlpha, ctx->sn2, ctx->dRed);
  double red[3];
  GPAK_HIP(hipMemcpyAsync(red, ctx->dRed, sizeof(red), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipEventRecord(ctx->ev[6], st));
  GPAK_HIP(hipEventSynchronize(ctx->ev[6]));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[6]));
  ctx->times.nlz_ms = ms;
  ctx->times.accumulated_ms[3] += ms;
  GPAK_HIP(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[8]));
  ctx->times.kmatvec_ms = ms;
  ctx->logdet = red[0]; ctx->quad = red[1]; ctx->sumlp = red[2];
  ctx->nlz = ctx->quad - ctx->sumlp + ctx->logdet;  // GP_Utils.cpp:1159
  ctx->state.nlz_built();
  return GPAK_OK;
}

// multi.hip: a context of a group takes over the factor its device's rank already holds as packed panels (the
// result of the group's distributed logLikelihood() for the CURRENT parameters) instead of factoring again:
// device-to-device copies of N^2/2 doubles where ensure_factor would spend N^3/3 flops.  The context must hold the
// same training set and parameters (multi.hip's ensure_replica); afterwards it is in the state ensure_nlz leaves.
int gpak_import_factor(gpak_ctx *ctx, const gpak_dist_factor_view *v) {
  if (!ctx || !v) return GPAK_EINVAL;
  if (!ctx->N || v->N != ctx->N || v->Np != ctx->Np || !ctx->have_params) {
    ctx->err = "gpak_import_factor: the context does not hold the group's training set / parameters";
    return GPAK_ESTATE;
  }
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int Np = ctx->Np;
  const long ld = ctx->ld;
  for (int b = 0; b < v->nJ; b++) {
    const int J = b * v->nb, W = std::min(v->nb, Np - J), rows = Np - J;
    GPAK_HIP(hipMemcpy2DAsync(ctx->dM + J + (size_t)J * ld, sizeof(double) * ld, v->panels[b], sizeof(double) * rows,
                              sizeof(double) * rows, W, hipMemcpyDeviceToDevice, st));
    GPAK_HIP(hipMemcpyAsync(ctx->dInv + (size_t)(J / GPAK_TILE) * 2 * GPAK_TILE * GPAK_TILE, v->invs[b],
                            sizeof(double) * (W / GPAK_TILE) * 2 * GPAK_TILE * GPAK_TILE, hipMemcpyDeviceToDevice, st));
  }
  GPAK_HIP(hipMemcpyAsync(ctx->dAlpha, v->alpha, sizeof(double) * Np, hipMemcpyDeviceToDevice, st));
  GPAK_HIP(hipMemcpyAsync(ctx->dF, v->f, sizeof(double) * Np, hipMemcpyDeviceToDevice, st));
  GPAK_HIP(hipStreamSynchronize(st));
  ctx->state.factor_imported();   // in particular the 512-block inverses were not imported: back substitutions use the 128-blocks
  ctx->quad = v->quad; ctx->sumlp = v->sumlp; ctx->logdet = v->logdet; ctx->nlz = v->nlz;
  return GPAK_OK;
}

// copy an n x m block (ld) of a device matrix to a dense host column-major array
static int copy_out(gpak_ctx *ctx, const double *dsrc, long ld, int n, int m, double *host) {
  GPAK_HIP(hipMemcpy2DAsync(host, sizeof(double) * n, dsrc, sizeof(double) * ld, sizeof(double) * n, m,
                            hipMemcpyDeviceToHost, ctx->stream));
  GPAK_HIP(hipStreamSynchronize(ctx->stream));
  return GPAK_OK;
}

static int ensure(gpak_ctx *ctx, CtxState::Rung rung) {
  return rung == CtxState::NLZ ? ensure_nlz(ctx) : rung == CtxState::ALPHA ? ensure_alpha(ctx) : rung == CtxState::FACTOR ? ensure_factor(ctx) : GPAK_OK;
}

// The prologue of a call built for the single-GPU context, in the order every such call has had it: a group is refused;
// then a training set, parameters, and (cols set: "test points" / "block points") d columns like the training set's, each
// where the call requires it; then the context is brought up to `rung` (NONE: the caller has more to refuse first).
static int single_gpu_call(gpak_ctx *ctx, const char *name, bool train, bool params, CtxState::Rung rung, int d = 0,
                           const char *cols = nullptr) {
  if (ctx->multi) {
    ctx->err = std::string(name) + " is built for the single-GPU context (gpak_create) only";
    return GPAK_ENOTIMPL;
  }
  if (train && !ctx->N) { ctx->err = "no training set (gpak_set_train)"; return GPAK_ESTATE; }
  if (params && !ctx->have_params) { ctx->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
  if (cols && d != ctx->d) { ctx->err = std::string(cols) + " must have as many columns as the training set"; return GPAK_EINVAL; }
  return ensure(ctx, rung);
}

// what a call answers when the training factor failed (as gpak_nlz: GP_Utils.cpp:1145-1146); p may be null
static void fill_nan(double *p, size_t n) {
  for (size_t i = 0; p && i < n; i++) p[i] = std::numeric_limits<double>::quiet_NaN();
}
static void nan_summary(gpak_loo_summary *s) {
  if (!s) return;
  s->mse = s->mssr = s->log_pl = std::numeric_limits<double>::quiet_NaN();
  s->ms = 0.0; s->passes = 0;
}

extern "C" {

int gpak_gram(gpak_ctx *ctx, double *K_host, double *D2_host) {
  if (!ctx) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_on_replica0(ctx->multi, [&](gpak_ctx *c) { return gpak_gram(c, K_host, D2_host); }, false));
  GPAK_HIP(hipSetDevice(ctx->device));
  int rc = gpak_ensure_U(ctx);
  if (rc) return rc;
  DevBuf<double> dD2;
  if (D2_host && !dD2.reserve((size_t)ctx->ld * ctx->Np)) {
    ctx->err = "device allocation failed for D2";
    return GPAK_ENOMEM;
  }
  // the matrix buffer is reused: whatever factor it held is gone
  ctx->state.matrix_overwritten();
  gpak_launch_fill(ctx->stream, ctx->U, ctx->U, ctx->Np, ctx->Np, ctx->kp, 1.0, 0.0, 0.0, 0, ctx->dM, ctx->ld,
                   dD2);
  rc = GPAK_OK;
  if (K_host) rc = copy_out(ctx, ctx->dM, ctx->ld, ctx->N, ctx->N, K_host);
  if (!rc && D2_host) rc = copy_out(ctx, dD2, ctx->ld, ctx->N, ctx->N, D2_host);
  GPAK_HIP(hipStreamSynchronize(ctx->stream));
  return rc;
}

int gpak_compute_k(gpak_ctx *ctx, const double *X1, int n, const double *X2, int m, int d, double *K_host,
                   double *D2_host) {
  if (!ctx || !X1 || !X2 || n <= 0 || m <= 0) return GPAK_EINVAL;
  if (ctx->multi)
    GPAK_MULTI_ERR(gpak_multi_on_replica0(ctx->multi, [&](gpak_ctx *c) { return gpak_compute_k(c, X1, n, X2, m, d, K_host, D2_host); }, false));
  if (d != 3 && d != 4) { ctx->err = "inputs must have 3 or 4 columns"; return GPAK_ENOTIMPL; }
  if (!ctx->have_params) { ctx->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
  GPAK_HIP(hipSetDevice(ctx->device));
  const int np = round_up(n, GPAK_TILE), mp = round_up(m, GPAK_TILE);
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int k = 0; k < d; k++) {
    for (int i = 0; i < n; i++) s1[k] += X1[i + (size_t)k * n];
    for (int i = 0; i < m; i++) s2[k] += X2[i + (size_t)k * m];
  }
  KernParams kp = ctx->kp;
  kp.d = d;
  gpak_pooled_mean(s1, n, s2, m, kp.mu);
  if (!(X1[0] == X2[0] && n == m)) kp.white = 0.0;  // Kern_White::computeK, Kernel.cpp:260-262
  DevBuf<double> dD2, dK, dx;   // freed last-declared first: P, Q, dx, dK, dD2 as ever
  DevPointsBuf Q, P;
  int rc = gpak_alloc_points(ctx, P, np);
  if (!rc) rc = gpak_alloc_points(ctx, Q, mp);
  if (!rc && (!dx.reserve(4 * (size_t)(np + mp)) || !dK.reserve((size_t)np * mp) || (D2_host && !dD2.reserve((size_t)np * mp)))) {
    ctx->err = "device allocation failed in gpak_compute_k";
    rc = GPAK_ENOMEM;
  }
  if (!rc) {
    hipStream_t st = ctx->stream;
    hipMemsetAsync(dx, 0, sizeof(double) * 4 * (size_t)(np + mp), st);
    double *dx2 = dx + 4 * (size_t)np;
    for (int k = 0; k < d; k++) {
      hipMemcpyAsync(dx + (size_t)k * np, X1 + (size_t)k * n, sizeof(double) * n, hipMemcpyHostToDevice, st);
      hipMemcpyAsync(dx2 + (size_t)k * mp, X2 + (size_t)k * m, sizeof(double) * m, hipMemcpyHostToDevice, st);
    }
    gpak_launch_transform(st, dx, np, n, kp, P);
    gpak_launch_transform(st, dx2, mp, m, kp, Q);
    gpak_launch_fill(st, P, Q, np, mp, kp, 1.0, 0.0, 0.0, 0, dK, np, dD2);
    if (K_host) rc = copy_out(ctx, dK, np, n, m, K_host);
    if (!rc && D2_host) rc = copy_out(ctx, dD2, np, n, m, D2_host);
    hipStreamSynchronize(st);
  }
  return rc;
}

int gpak_factor(gpak_ctx *ctx) {
  if (!ctx) return GPAK_EINVAL;
  if (ctx->multi) { double v; GPAK_MULTI_ERR(gpak_multi_nlz(ctx->multi, &v, nullptr, nullptr, nullptr)); }
  return ensure_factor(ctx);
}

int gpak_failed_column(const gpak_ctx *ctx) {
  if (!ctx) return 0;
  return ctx->multi ? gpak_multi_failed_column(ctx->multi) : ctx->state.failed_col;
}
int gpak_n_gpus(const gpak_ctx *ctx) { return !ctx ? 0 : (ctx->multi ? gpak_multi_n(ctx->multi) : 1); }
const char *gpak_transport(const gpak_ctx *ctx) { return !ctx ? "" : (ctx->multi ? gpak_multi_transport(ctx->multi) : "none"); }
int gpak_group_rank_stats(gpak_ctx *ctx, int rank, gpak_dist_stats *out) {
  if (!ctx || !out || !ctx->multi) return GPAK_EINVAL;
  return gpak_multi_stats(ctx->multi, rank, out);
}

int gpak_get_chol_upper(gpak_ctx *ctx, double *R_host) {
  if (!ctx || !R_host) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_on_replica0(ctx->multi, [&](gpak_ctx *c) { return gpak_get_chol_upper(c, R_host); }, true));
  int rc = ensure_factor(ctx);
  if (rc) return rc;
  const int N = ctx->N;
  std::vector<double> tmp((size_t)N * N);
  rc = copy_out(ctx, ctx->dM, ctx->ld, N, N, tmp.data());
  if (rc) return rc;
  for (int j = 0; j < N; j++)
    for (int i = 0; i < N; i++) R_host[i + (size_t)j * N] = i <= j ? tmp[j + (size_t)i * N] : 0.0;  // R = L^T
  return GPAK_OK;
}

int gpak_solve_alpha(gpak_ctx *ctx, double *alpha_host) {
  if (!ctx) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_alpha(ctx->multi, alpha_host));
  int rc = ensure_alpha(ctx);
  if (rc) return rc;
  if (alpha_host) {
    GPAK_HIP(hipMemcpyAsync(alpha_host, ctx->dAlpha, sizeof(double) * ctx->N, hipMemcpyDeviceToHost, ctx->stream));
    GPAK_HIP(hipStreamSynchronize(ctx->stream));
  }
  return GPAK_OK;
}

int gpak_solve_chol(gpak_ctx *ctx, double *X_host, int k) {
  if (!ctx || !X_host || k <= 0) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_on_replica0(ctx->multi, [&](gpak_ctx *c) { return gpak_solve_chol(c, X_host, k); }, true));
  int rc = ensure_factor(ctx);
  if (rc) return rc;
  return gpak_solve_chol_impl(ctx, X_host, k);
}

int gpak_nlz(gpak_ctx *ctx, double *nlz) {
  if (!ctx || !nlz) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_nlz(ctx->multi, nlz, nullptr, nullptr, nullptr));
  int rc = ensure_nlz(ctx);
  if (rc) {
    *nlz = std::numeric_limits<double>::quiet_NaN();  // GP_Utils.cpp:1146, 1157
    return rc;
  }
  *nlz = ctx->nlz;
  return GPAK_OK;
}

int gpak_nlz_terms(gpak_ctx *ctx, double *quad, double *sumlp, double *logdet) {
  if (!ctx) return GPAK_EINVAL;
  if (ctx->multi) { double v; GPAK_MULTI_ERR(gpak_multi_nlz(ctx->multi, &v, quad, sumlp, logdet)); }
  int rc = ensure_nlz(ctx);
  if (rc) return rc;
  if (quad) *quad = ctx->quad;
  if (sumlp) *sumlp = ctx->sumlp;
  if (logdet) *logdet = ctx->logdet;
  return GPAK_OK;
}

int gpak_predict(gpak_ctx *ctx, const double *Xte, long M, int d, double *mean, double *var, int compat_flags) {
  if (!ctx || !Xte || !mean || M <= 0) return GPAK_EINVAL;
  int rc;
  if (ctx->multi) {
    rc = gpak_multi_predict(ctx->multi, Xte, M, d, mean, var);
    if (rc) { ctx->err = gpak_multi_error(ctx->multi); return rc; }
  } else {
    // _postVar calls logLikelihood() (GP_Utils.cpp:980); _postMean calls updateAlpha() (:961)
    rc = single_gpu_call(ctx, "gpak_predict", true, false, CtxState::NLZ, d, "test points");
    if (rc) return rc;
    rc = gpak_predict_impl(ctx, Xte, M, mean, var, nullptr, 0);
    if (rc) return rc;
  }
  if (var) {
    if (compat_flags & GPAK_COMPAT_VARCLAMP) {
      // GP_Utils.cpp:1002-1003: `uvec ind = varSigma < 0; varSigma.elem(ind) = 0` -- the 0/1
      // mask is an index list, so element 0 is zeroed when any entry is >= 0 and element 1
      // when any entry is < 0.
      bool any_neg = false, any_nonneg = false;
      for (long i = 0; i < M; i++) { if (var[i] < 0) any_neg = true; else any_nonneg = true; }
      if (any_nonneg) var[0] = 0.0;
      if (any_neg && M > 1) var[1] = 0.0;
    } else {
      for (long i = 0; i < M; i++) if (var[i] < 0) var[i] = 0.0;
    }
    if (!((compat_flags & GPAK_COMPAT_SN2SKIP) && ctx->sn2 == 1.0))  // GP_Utils.cpp:1036-1040
      for (long i = 0; i < M; i++) var[i] += ctx->sn2;
  }
  return GPAK_OK;
}

int gpak_grad(gpak_ctx *ctx, double *g) {
  if (!ctx || !g) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_grad(ctx->multi, g));
  if (!ctx->expans_only) { ctx->err = "gpak_grad handles the ExpAns(+Bias) composition only"; return GPAK_ENOTIMPL; }
  int rc = ensure_nlz(ctx);  // GradLL re-enters logLikelihood(): GP_Utils.cpp:1173-1174
  if (rc) return rc;
  return gpak_grad_impl(ctx, g, 10);
}

int gpak_grad_hyb(gpak_ctx *ctx, double *g, int ng) {
  if (!ctx || !g) return GPAK_EINVAL;
  if (ctx->multi) GPAK_MULTI_ERR(gpak_multi_grad_hyb(ctx->multi, g, ng));
  int rc = ensure_nlz(ctx);
  if (rc) return rc;
  return gpak_grad_impl(ctx, g, ng);
}

int gpak_grad_exact(gpak_ctx *ctx, double *g, int ng) {
  if (!ctx || !g) return GPAK_EINVAL;
  int rc = single_gpu_call(ctx, "gpak_grad_exact", false, false, CtxState::NLZ);
  if (ctx->multi) ctx->err += "; a multi-GPU context has gpak_grad / gpak_grad_hyb";
  if (rc) return rc;
  return gpak_grad_exact_impl(ctx, g, ng);
}

int gpak_loo(gpak_ctx *ctx, double *mean, double *var, gpak_loo_summary *summary) {
  if (!ctx) return GPAK_EINVAL;
  int rc = single_gpu_call(ctx, "gpak_loo", false, false, CtxState::NLZ);
  if (rc == GPAK_OK) rc = gpak_loo_impl(ctx, mean, var, summary);
  if (rc == GPAK_ENOTPD) {
    fill_nan(mean, ctx->N);
    fill_nan(var, ctx->N);
    nan_summary(summary);
  }
  return rc;
}

int gpak_loo_grad(gpak_ctx *ctx, double *g, int ng, gpak_loo_summary *summary) {
  if (!ctx || !g) return GPAK_EINVAL;
  // what the call refuses is refused before anything is factored
  int rc = single_gpu_call(ctx, "gpak_loo_grad", true, true, CtxState::NONE);
  if (rc == GPAK_OK) rc = gpak_loo_grad_layout(ctx, ng);
  if (rc) return rc;
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK) rc = gpak_loo_grad_impl(ctx, g, ng, summary);
  if (rc == GPAK_ENOTPD) {
    fill_nan(g, ng);
    nan_summary(summary);
  }
  return rc;
}

// The labels of gpak_cv_groups / gpak_cv_folds (`who`, with its colon), checked, and the samples sorted by (group, sample)
// with a counting sort: perm, and offs = where each group starts in it.  max_group: the largest group allowed (0: any)
// The words of the one check: the labelled items, their count and the groups, as the call's documentation names them
struct LabelWords { const char *arg, *count, *n, *item, *items, *group; };
static const LabelWords kSampleWords = {"group", "n_groups", "N", "sample", "samples", "group"};
static const LabelWords kHoleWords = {"hole", "H", "Mc", "point", "points", "hole"};
static int group_lists(gpak_ctx *ctx, const std::string &who, const int *group, int n_groups, int max_group,
                       std::vector<int> &perm, std::vector<int> &offs, int n_items = -1, const LabelWords &wd = kSampleWords) {
  const int N = n_items < 0 ? ctx->N : n_items;
  if (!group) { ctx->err = who + wd.arg + " is NULL"; return GPAK_EINVAL; }
  if (n_groups < 1 || n_groups > N) {
    ctx->err = who + wd.count + " = " + std::to_string(n_groups) + " is outside [1, " + wd.n + " = " + std::to_string(N) + "]";
    return GPAK_EINVAL;
  }
  offs.assign((size_t)n_groups + 1, 0);
  perm.resize((size_t)N);
  for (int i = 0; i < N; i++) {
    if (group[i] < 0 || group[i] >= n_groups) {
      ctx->err = who + wd.item + " " + std::to_string(i) + " has label " + std::to_string(group[i]) + ", outside [0, " +
                 std::to_string(n_groups) + ")";
      return GPAK_EINVAL;
    }
    if (++offs[(size_t)group[i] + 1] == max_group + 1 && max_group > 0) {
      ctx->err = who + wd.group + " " + std::to_string(group[i]) + " has more than " + std::to_string(max_group) + " " +
                 wd.items + " (" + wd.item + " " + std::to_string(i) + " is one too many)";
      return GPAK_EINVAL;
    }
  }
  for (int g = 0; g < n_groups; g++) {
    if (offs[(size_t)g + 1] == 0) { ctx->err = who + "label " + std::to_string(g) + " is not used"; return GPAK_EINVAL; }
    offs[(size_t)g + 1] += offs[g];
  }
  std::vector<int> at(offs.begin(), offs.end() - 1);
  for (int i = 0; i < N; i++) perm[(size_t)at[group[i]]++] = i;
  return GPAK_OK;
}

// what the grouped calls answer when the training factor failed: their own summary type, written out
static void nan_cv_summary(gpak_cv_groups_summary *summary, int n_groups) {
  if (!summary) return;
  summary->mse = summary->mssr = summary->msmd = summary->log_pl = std::numeric_limits<double>::quiet_NaN();
  summary->ms = 0.0; summary->groups = n_groups; summary->max_size = 0;
}

// gpak_cv_groups and gpak_cv_folds (folds: no limit on a group, and flags): what the call refuses is refused before
// anything is factored
static int cv_call(gpak_ctx *ctx, const char *name, bool folds, const int *group, int n_groups, double *mean, double *var,
                   double *group_logp, gpak_cv_groups_summary *summary, int flags) {
  if (!ctx) return GPAK_EINVAL;
  int rc = single_gpu_call(ctx, name, true, true, CtxState::NONE);
  if (rc) return rc;
  const int N = ctx->N;
  const std::string who = std::string(name) + ": ";
  std::vector<int> offs, perm;
  if ((rc = group_lists(ctx, who, group, n_groups, folds ? 0 : GPAK_CV_GROUP_MAX, perm, offs))) return rc;
  if (flags & ~GPAK_CV_FOLDS_NO_BATCH) {
    ctx->err = who + "flags = " + std::to_string(flags) + " has bits other than GPAK_CV_FOLDS_NO_BATCH";
    return GPAK_EINVAL;
  }
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK)
    return folds ? gpak_cv_folds_impl(ctx, perm.data(), offs.data(), n_groups, mean, var, group_logp, summary, flags)
                 : gpak_cv_groups_impl(ctx, perm.data(), offs.data(), n_groups, mean, var, group_logp, summary);
  if (rc == GPAK_ENOTPD) {   // the training factor
    fill_nan(mean, N);
    fill_nan(var, N);
    fill_nan(group_logp, n_groups);
    nan_cv_summary(summary, n_groups);
  }
  return rc;
}

int gpak_cv_groups(gpak_ctx *ctx, const int *group, int n_groups, double *mean, double *var, double *group_logp,
                   gpak_cv_groups_summary *summary) {
  return cv_call(ctx, "gpak_cv_groups", false, group, n_groups, mean, var, group_logp, summary, 0);
}

int gpak_cv_groups_grad(gpak_ctx *ctx, const int *group, int n_groups, double *g, int ng, gpak_cv_groups_summary *summary) {
  if (!ctx || !g) return GPAK_EINVAL;
  // what the call refuses is refused before anything is factored: the context, the composition, then the labels with
  // gpak_cv_groups' own check
  int rc = single_gpu_call(ctx, "gpak_cv_groups_grad", true, true, CtxState::NONE);
  if (rc == GPAK_OK) rc = gpak_cv_groups_grad_layout(ctx, ng);
  if (rc) return rc;
  std::vector<int> offs, perm;
  if ((rc = group_lists(ctx, "gpak_cv_groups_grad: ", group, n_groups, GPAK_CV_GROUP_MAX, perm, offs))) return rc;
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK) return gpak_cv_groups_grad_impl(ctx, perm.data(), offs.data(), n_groups, g, ng, summary);
  if (rc == GPAK_ENOTPD) {   // the training factor
    fill_nan(g, ng);
    nan_cv_summary(summary, n_groups);
  }
  return rc;
}

int gpak_cv_folds(gpak_ctx *ctx, const int *group, int n_groups, double *mean, double *var, double *group_logp,
                  gpak_cv_groups_summary *summary, int flags) {
  return cv_call(ctx, "gpak_cv_folds", true, group, n_groups, mean, var, group_logp, summary, flags);
}

int gpak_cv_folds_grad(gpak_ctx *ctx, const int *group, int n_groups, double *g, int ng, gpak_cv_groups_summary *summary,
                       int flags) {
  if (!ctx) return GPAK_EINVAL;
  // what the call refuses is refused before anything is factored: the context, the arguments, the composition, then the
  // labels with gpak_cv_folds' own check
  const std::string who = "gpak_cv_folds_grad: ";
  int rc = single_gpu_call(ctx, "gpak_cv_folds_grad", true, true, CtxState::NONE);
  if (rc == GPAK_ESTATE) ctx->err = who + ctx->err;
  if (rc) return rc;
  if (!g) { ctx->err = who + "g is NULL"; return GPAK_EINVAL; }
  if ((rc = gpak_cv_folds_grad_layout(ctx, ng))) return rc;
  std::vector<int> offs, perm;
  if ((rc = group_lists(ctx, who, group, n_groups, 0, perm, offs))) return rc;
  if (flags & ~GPAK_CV_FOLDS_NO_BATCH) {
    ctx->err = who + "flags = " + std::to_string(flags) + " has bits other than GPAK_CV_FOLDS_NO_BATCH";
    return GPAK_EINVAL;
  }
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK) return gpak_cv_folds_grad_impl(ctx, perm.data(), offs.data(), n_groups, g, ng, summary, flags);
  if (rc == GPAK_ENOTPD) {   // the training factor
    fill_nan(g, ng);
    nan_cv_summary(summary, n_groups);
  }
  return rc;
}

static int block_call(gpak_ctx *ctx, const char *name, const double *Xd, long M, int nd, int d, double *mean, double *var,
                      int flags, double *Kbar_host) {
  int rc = single_gpu_call(ctx, name, true, false, CtxState::NLZ, d, "block points");
  if (rc == GPAK_OK) rc = gpak_predict_block_impl(ctx, Xd, M, nd, mean, var, flags, Kbar_host);
  if (rc == GPAK_ENOTPD) {
    fill_nan(mean, M);
    fill_nan(var, M);
    fill_nan(Kbar_host, (size_t)M * ctx->N);
  }
  return rc;
}

int gpak_block_cross(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, double *Kbar_host) {
  if (!ctx || !Xd || !Kbar_host || M <= 0 || nd <= 0) return GPAK_EINVAL;
  return block_call(ctx, "gpak_block_cross", Xd, M, nd, d, nullptr, nullptr, 0, Kbar_host);
}

int gpak_predict_block(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, double *mean, double *var, int flags) {
  if (!ctx || !Xd || !mean || M <= 0 || nd <= 0) return GPAK_EINVAL;
  return block_call(ctx, "gpak_predict_block", Xd, M, nd, d, mean, var, flags, nullptr);
}

static int joint_call(gpak_ctx *ctx, const char *name, const double *Xd, long M, int nd, int d, double *mean, double *cov_host,
                      int flags, const double *Xi, int S, double nugget, double *Z) {
  int rc = single_gpu_call(ctx, name, true, false, CtxState::NLZ, d, "block points");
  if (rc == GPAK_ENOTPD) {   // the training factor: as gpak_predict_block
    ctx->err = "the training factor failed (B = I + K/sn2 is not positive definite at column " + std::to_string(ctx->state.failed_col) + ")";
    fill_nan(mean, M);
    fill_nan(cov_host, (size_t)M * M);
    fill_nan(Z, (size_t)M * S);
    return rc;
  }
  if (rc == GPAK_OK) rc = gpak_joint_impl(ctx, Xd, M, nd, mean, cov_host, flags, Xi, S, nugget, Z);
  if (rc == GPAK_ENOTPD) fill_nan(Z, (size_t)M * S);   // C + nugget I: the mean stands
  return rc;
}

int gpak_predict_joint(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, double *mean, double *cov_host, int flags) {
  if (!ctx || !Xd || !mean || M <= 0 || nd <= 0) return GPAK_EINVAL;
  return joint_call(ctx, "gpak_predict_joint", Xd, M, nd, d, mean, cov_host, flags, nullptr, 0, 0.0, nullptr);
}

int gpak_sample_joint(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, const double *Xi, int S, double nugget,
                      double *Z, double *mean, int flags) {
  if (!ctx || !Xd || !Xi || !Z || M <= 0 || nd <= 0 || S <= 0 || !(nugget >= 0.0)) return GPAK_EINVAL;
  return joint_call(ctx, "gpak_sample_joint", Xd, M, nd, d, mean, nullptr, flags, Xi, S, nugget, Z);
}

// gpak_design (include/gpak_design.h): what the call refuses is refused before anything is factored
int gpak_design(gpak_ctx *ctx, const double *Xt, long T, int nd, const double *Xc, long Mc, int d, const int *hole, int H,
                const double *wt, int k, double *gain, double *reduction, double *var, int *picked, double *pick_gain,
                double *var_after, gpak_design_summary *summary) {
  if (!ctx) return GPAK_EINVAL;
  const std::string who = "gpak_design: ";
  int rc = single_gpu_call(ctx, "gpak_design", true, true, CtxState::NONE);
  if (rc) return rc;
  auto refuse = [&](const std::string &what) { ctx->err = who + what; return GPAK_EINVAL; };
  if (T <= 0 || nd <= 0 || Mc <= 0)
    return refuse("T = " + std::to_string(T) + ", nd = " + std::to_string(nd) + ", Mc = " + std::to_string(Mc) + " must all be positive");
  if (d != ctx->d) return refuse("target and candidate points must have as many columns as the training set");
  if (!Xt || !Xc || !gain) return refuse(std::string(!Xt ? "Xt" : !Xc ? "Xc" : "gain") + " is NULL");
  // the block path's budget for the raw and transformed points, here of the one batch there is (gpak_joint_impl)
  const long Tp = (T + 255) / 256 * 256, Mcp = (Mc + 255) / 256 * 256;
  const size_t per_point = sizeof(double) * (4 + GPAK_PT * (size_t)ctx->kp.nterms);
  if (Tp + Mcp > (1L << 24) || (double)Tp * nd + (double)Mcp > (double)((size_t)1 << 30) / (double)per_point)
    return refuse("the targets' discretisation points and the candidates exceed the 1 GiB point budget of one batch (the stack is held at once)");
  std::vector<int> offs, perm;
  if ((rc = group_lists(ctx, who, hole, H, GPAK_CV_GROUP_MAX, perm, offs, (int)Mc, kHoleWords))) return rc;
  for (long b = 0; wt && b < T; b++)
    if (!(wt[b] >= 0.0) || !std::isfinite(wt[b]))
      return refuse("weight " + std::to_string(b) + " is negative or not finite");
  if (k < 0 || k > H) return refuse("k = " + std::to_string(k) + " is outside [0, H = " + std::to_string(H) + "]");
  if (k > 0 && (!picked || !pick_gain)) return refuse(std::string(!picked ? "picked" : "pick_gain") + " is NULL with k > 0");
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK)
    return gpak_design_impl(ctx, Xt, T, nd, Xc, Mc, perm.data(), offs.data(), H, wt, k, gain, reduction, var, picked, pick_gain,
                            var_after, summary);
  if (rc == GPAK_ENOTPD) {
    ctx->err = who + "the training factor failed (B = I + K/sn2 is not positive definite at column " +
               std::to_string(ctx->state.failed_col) + ")";
    fill_nan(gain, H);
    fill_nan(reduction, (size_t)T * H);
    fill_nan(var, T);
    fill_nan(pick_gain, k);
    fill_nan(var_after, T);
    if (summary) {
      summary->var_before = summary->var_after = std::numeric_limits<double>::quiet_NaN();
      summary->ms = 0.0; summary->holes = H; summary->max_size = 0; summary->picks = 0;
    }
  }
  return rc;
}

// gpak_condition / gpak_sample_path (include/gpak_condition.h): the block calls' prologue and their answer to a failed factor
static int condition_call(gpak_ctx *ctx, const char *name, const double *Xd, long M, int nd, int d, const double *Ysim,
                          const double *Fsim, int S, double *Z, double *mean, int flags, gpak_condition_summary *summary,
                          const GpakPathPrior *prior) {
  int rc = single_gpu_call(ctx, name, true, false, CtxState::NONE, d, "block points");
  if (rc) return rc;
  if (flags & ~GPAK_COND_UNFUSED) {
    ctx->err = std::string(name) + ": flags = " + std::to_string(flags) + " has bits other than GPAK_COND_UNFUSED";
    return GPAK_EINVAL;
  }
  if (prior) {
    if (!ctx->have_params) { ctx->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
    for (int f = 0; f < prior->nfeat; f++)
      if (prior->feat_term[f] < 0 || prior->feat_term[f] >= ctx->kp.nterms) {
        ctx->err = std::string(name) + ": feature " + std::to_string(f) + " names term " + std::to_string(prior->feat_term[f]) +
                   ", outside the composition's " + std::to_string(ctx->kp.nterms);
        return GPAK_EINVAL;
      }
    if (!prior->b0 && ctx->kp.bias != 0.0) { ctx->err = std::string(name) + ": b0 is NULL and the constant is not 0"; return GPAK_EINVAL; }
  }
  rc = ensure_nlz(ctx);
  if (rc == GPAK_OK) rc = gpak_condition_impl(ctx, Xd, M, nd, Ysim, Fsim, S, Z, mean, flags, summary, prior);
  if (rc == GPAK_ENOTPD) {
    fill_nan(Z, (size_t)M * S);
    fill_nan(mean, M);
  }
  if (rc != GPAK_OK && summary) {
    summary->solve_ms = summary->prior_ms = summary->product_ms = 0.0;
    summary->batches = 0; summary->fused = (flags & GPAK_COND_UNFUSED) ? 0 : 1;
  }
  return rc;
}

int gpak_condition(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, const double *Ysim, const double *Fsim, int S, double *Z,
                   double *mean, int flags, gpak_condition_summary *summary) {
  if (!ctx || !Xd || !Ysim || !Z || M <= 0 || nd <= 0 || S <= 0) return GPAK_EINVAL;
  return condition_call(ctx, "gpak_condition", Xd, M, nd, d, Ysim, Fsim, S, Z, mean, flags, summary, nullptr);
}

int gpak_sample_path(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, int nfeat, const int *feat_term, const double *omega,
                     const double *ab, const double *b0, const double *E, int S, double *Z, double *mean, int flags,
                     gpak_condition_summary *summary) {
  if (!ctx || !Xd || !Z || M <= 0 || nd <= 0 || S <= 0 || nfeat <= 0 || !feat_term || !omega || !ab || !E) return GPAK_EINVAL;
  const GpakPathPrior prior = {nfeat, feat_term, omega, ab, b0, E};
  return condition_call(ctx, "gpak_sample_path", Xd, M, nd, d, nullptr, nullptr, S, Z, mean, flags, summary, &prior);
}

int gpak_timing(gpak_ctx *ctx, gpak_phase_times *out) {
  if (!ctx || !out) return GPAK_EINVAL;
  if (ctx->multi) return gpak_multi_timing(ctx->multi, out);
  *out = ctx->times;
  out->evaluations = ctx->state.factorisations;
  return GPAK_OK;
}

int gpak_calibrate(gpak_ctx *ctx, double *mfma_f64_tflops, double *hbm_write_gbs) {
  if (!ctx || !mfma_f64_tflops || !hbm_write_gbs) return GPAK_EINVAL;
  if (ctx->multi)
    GPAK_MULTI_ERR(gpak_multi_on_replica0(ctx->multi, [&](gpak_ctx *c) { return gpak_calibrate(c, mfma_f64_tflops, hbm_write_gbs); }, false));
  GPAK_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)4 << 30;
  DevBuf<double> scratch;
  if (!scratch.reserve(bytes / sizeof(double))) { ctx->err = "calibration scratch allocation failed"; return GPAK_ENOMEM; }
  return gpak_calibrate_impl(ctx, scratch, bytes, mfma_f64_tflops, hbm_write_gbs);
}

}  // extern "C"
