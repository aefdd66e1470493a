// local.hip -- moving-neighbourhood kriging for gfx950 (include/gpak_local.h, include/gpak_dev_local.h): M independent
// dense problems of at most 128 x 128, each filled from the covariance function, factored and solved without leaving the CU.
//
// Per node b with the s <= k listed samples I (noise = sn2 + white):
//   K_II = k(x_i, x_j) + bias + noise delta_ij,  kbar_i = (1/nd) sum_a k(p_a, x_i) + bias,  kbb = the block's prior variance
//   mean = kbar^T K_II^-1 y_I = (L^-1 kbar) . (L^-1 y),   var = kbb - |L^-1 kbar|^2 [+ (noise - white) / nd],   K_II = L L^T
// The LDS image of a node is the lower triangle of K_II in s rows of pitch smax + 1 (odd: a column and a row are both
// conflict-free) with TWO MORE ROWS under it, y_I^T and kbar^T.  The right-looking Cholesky runs over all s + 2 rows: what
// it leaves in the two extra rows is (L^-1 y)^T and (L^-1 kbar)^T -- the forward substitution with both right-hand sides
// is the factorisation's own trailing update, and no back substitution is needed.
// Tiers, chosen per launch from k (gpak_local_tier): smax = 16 / 32 one wave per node and four nodes per workgroup (no
// workgroup barrier at all), smax = 64 / 128 one workgroup of 256 threads per node.  ONE kernel serves all of them, the
// tier being run-time arguments, so that a node's arithmetic is literally the same code in every tier: every element of
// K_II, kbar and kbb is evaluated by one thread in one order, every element update of the factorisation is one fma per
// eliminated column in ascending column order, and the two final dot products are summed by the first 64 threads of the
// node -- element j by lane j mod 64 in ascending j, then one xor-butterfly over the 64 lanes.  Nothing depends on the
// grid, on the batch or on the node's neighbours in it.
//
// Ordinary kriging (include/gpak_local_ok.h, include/gpak_dev_local_ok.h) is the same kernel body with OKM = true: a THIRD
// extra row, the ones vector, under y_I^T and kbar^T, so that the factorisation leaves w_1 = L^-1 1 beside w_y and w_k, three
// more dot products summed by the same scheme, and an epilogue of one lane (the order is stated in gpak_dev_local_ok.h).
// The fill, the gather and the factorisation loop are shared; the simple-kriging instantiation is the code it was.
// The LDS image is NOT larger: the gathered coordinates q are dead once K_II and kbar are filled, so the third row is
// written after the fill, where a full list (s = smax) lets it run into the head of q; a shorter list keeps it inside the
// smax + 2 rows.  Ordinary kriging therefore has simple kriging's LDS size and occupancy in every tier.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/gpak_dev.h"
#include "../../include/gpak_dev_local.h"
#include "../../include/gpak_local.h"
#include "../../include/gpak_dev_local_ok.h"
#include "../../include/gpak_local_ok.h"
#include "gpak_internal.h"

#define PARR GPAK_PARR
#define LOC_NC 4          // coordinate arrays gathered per term: u0, u1, u2, u3 (the direct form reads no |u|^2)
#define LOC_WAVE_NODES 4  // nodes per workgroup in the one-wave tiers

// the barrier of a node's threads: the workgroup's, or -- one wave per node -- only the order of its own LDS accesses
__device__ __forceinline__ void loc_sync(bool wave_nodes) {
  if (wave_nodes) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}
// the sum over the 64 lanes of a wave, the same bytes in every lane
__device__ __forceinline__ double loc_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool OKM>
__global__ __launch_bounds__(256) void gpak_local_krige_f64(const double *__restrict__ P, int cap, int nB, int nd,
                                                             const double *__restrict__ U, int capU, int nU,
                                                             const double *__restrict__ ys, KernParams kp, double inv_nd,
                                                             double white_nd, double noise, double var_add,
                                                             const int *__restrict__ nbr, int k, int smax, int wave_nodes,
                                                             int region, double *__restrict__ mean, double *__restrict__ var,
                                                             double *__restrict__ mu, int *info, int *nfail) {
  constexpr int XR = OKM ? 3 : 2;   // the rows under the triangle: y_I^T, kbar^T and, for ordinary kriging, 1^T
  static_assert(LOC_NC >= 2, "the third row of a full list lies in the first smax + 1 doubles of q");
  extern __shared__ double loc_lds[];
  const int t = threadIdx.x;
  const bool wn = wave_nodes != 0;
  const int nt = wn ? 64 : 256, tid = wn ? (t & 63) : t;
  const int b = wn ? (int)blockIdx.x * LOC_WAVE_NODES + (t >> 6) : (int)blockIdx.x;
  if (b >= nB) return;   // a whole wave of a one-wave tier: that tier has no workgroup barrier
  const int nterms = kp.nterms, pitch = smax + 1;
  double *A = loc_lds + (wn ? (size_t)(t >> 6) * region : 0);   // s + XR rows of `pitch`: smax + 2 of them are A's own
  double *q = A + (size_t)(smax + 2) * pitch;                   // [term][LOC_NC][smax]; dead after the fill
  int *ridx = reinterpret_cast<int *>(q + (size_t)nterms * LOC_NC * smax);

  for (int e = tid; e < k; e += nt) ridx[e] = nbr[e + (size_t)k * b];
  loc_sync(wn);
  int s = 0;   // the list ends at the first entry that names no sample
  while (s < k && (unsigned)ridx[s] < (unsigned)nU) s++;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (OKM && s == 0) {   // no sample, no local mean: not an estimate, and not a failure of the factorisation either
    if (tid == 0) {
      mean[b] = qnan;
      if (var) var[b] = qnan;
      if (mu) mu[b] = qnan;
    }
    return;   // the whole node: every thread of it read the same list
  }
  const int R = s + XR;
  double *yrow = A + (size_t)s * pitch, *krow = yrow + pitch;

  for (int e = tid; e < s * nterms * LOC_NC; e += nt) {
    const int i = e % s, mc = e / s, m = mc / LOC_NC, c = mc % LOC_NC;
    q[(size_t)mc * smax + i] = PARR(U, capU, m, c < 3 ? c : 4)[ridx[i]];
  }
  for (int i = tid; i < s; i += nt) yrow[i] = ys[ridx[i]];
  loc_sync(wn);

  // kbar_i: the nd values in ascending a, terms innermost, scaled once by 1/nd before the bias is added (gpak_fillblk_f64)
  const size_t capP = (size_t)nd * cap;
  for (int i = tid; i < s; i += nt) {
    double acc = 0.0;
    for (int a = 0; a < nd; a++) {
      const size_t o = (size_t)a * cap + b;
      for (int m = 0; m < nterms; m++) {
        const double *qm = q + (size_t)m * LOC_NC * smax + i;
        acc += gpak_profile(gpak_d2(PARR(P, capP, m, 0)[o], PARR(P, capP, m, 1)[o], PARR(P, capP, m, 2)[o], 0.0,
                                    PARR(P, capP, m, 4)[o], qm[0], qm[smax], qm[2 * smax], 0.0, qm[3 * smax], GPAK_DIST_DIRECT),
                            kp.term[m]);
      }
    }
    krow[i] = fma(inv_nd, acc, kp.bias);
  }
  // kbb by the node's first 64 threads: the pairs (a, a') lane, lane + 64, ... in ascending order (gpak_block_self_f64)
  double kbb = 0.0;
  if (tid < 64) {
    const long npair = (long)nd * nd;
    double sacc = 0.0;
    for (long e = tid; e < npair; e += 64) {
      const size_t oa = (size_t)(e / nd) * cap + b, ob = (size_t)(e % nd) * cap + b;
      double kv = kp.bias;
      for (int m = 0; m < nterms; m++)
        kv += gpak_profile(gpak_d2(PARR(P, capP, m, 0)[oa], PARR(P, capP, m, 1)[oa], PARR(P, capP, m, 2)[oa], 0.0,
                                   PARR(P, capP, m, 4)[oa], PARR(P, capP, m, 0)[ob], PARR(P, capP, m, 1)[ob],
                                   PARR(P, capP, m, 2)[ob], 0.0, PARR(P, capP, m, 4)[ob], GPAK_DIST_DIRECT),
                           kp.term[m]);
      sacc += kv;
    }
    kbb = loc_wave_sum(sacc) / ((double)nd * (double)nd) + white_nd;
  }
  // the lower triangle of K_II, element e = i (i + 1) / 2 + j
  const int ntri = s * (s + 1) / 2;
  for (int e = tid; e < ntri; e += nt) {
    int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    if (i * (i + 1) / 2 > e) i--;
    if ((i + 1) * (i + 2) / 2 <= e) i++;
    const int j = e - i * (i + 1) / 2;
    double acc = 0.0;
    for (int m = 0; m < nterms; m++) {
      const double *qi = q + (size_t)m * LOC_NC * smax + i, *qj = q + (size_t)m * LOC_NC * smax + j;
      acc += gpak_profile(gpak_d2(qi[0], qi[smax], qi[2 * smax], 0.0, qi[3 * smax], qj[0], qj[smax], qj[2 * smax], 0.0,
                                  qj[3 * smax], GPAK_DIST_DIRECT),
                          kp.term[m]);
    }
    acc += kp.bias;
    A[i * pitch + j] = i == j ? acc + noise : acc;
  }
  loc_sync(wn);
  if (OKM) {   // the ones row, only now: with s = smax it lies where q was, and q has been read for the last time
    for (int i = tid; i < s; i += nt) krow[pitch + i] = 1.0;
    loc_sync(wn);
  }

  // right-looking Cholesky over the s + XR rows; the diagonal itself is not needed afterwards and is left as the pivot
  bool ok = true;
  for (int j = 0; j < s; j++) {
    const double dj = A[j * pitch + j];   // every thread of the node reads the same value: the branch is uniform
    if (!(dj > 0.0)) { ok = false; break; }
    const double ri = 1.0 / sqrt(dj);
    for (int i = j + 1 + tid; i < R; i += nt) A[i * pitch + j] *= ri;
    loc_sync(wn);
    for (int c = j + 1 + (tid >> 4); c < s; c += nt / 16) {   // column c of the trailing block, rows c .. R - 1, 16 lanes each
      const double acj = A[c * pitch + j];
      for (int i = c + (tid & 15); i < R; i += 16)
        A[i * pitch + c] = fma(-A[i * pitch + j], acj, A[i * pitch + c]);
    }
    loc_sync(wn);
  }
  if (!ok) {
    if (tid == 0) {
      mean[b] = qnan;
      if (var) var[b] = qnan;
      if (OKM && mu) mu[b] = qnan;
      atomicMin(info, b + 1);
      if (nfail) atomicAdd(nfail, 1);   // an integer count: the same whatever the order
    }
    return;
  }
  if (tid < 64) {
    double macc = 0.0, qacc = 0.0;
    for (int j = tid; j < s; j += 64) {
      const double w = krow[j];
      macc = fma(w, yrow[j], macc);
      qacc = fma(w, w, qacc);
    }
    macc = loc_wave_sum(macc);
    qacc = loc_wave_sum(qacc);
    if (!OKM) {
      if (tid == 0) {
        mean[b] = macc;
        if (var) var[b] = (kbb - qacc) + var_add;
      }
    } else {
      const double *orow = krow + pitch;   // w_1 = L^-1 1
      double aacc = 0.0, byacc = 0.0, bkacc = 0.0;
      for (int j = tid; j < s; j += 64) {
        const double w = orow[j];
        aacc = fma(w, w, aacc);
        byacc = fma(w, yrow[j], byacc);
        bkacc = fma(w, krow[j], bkacc);
      }
      aacc = loc_wave_sum(aacc);
      byacc = loc_wave_sum(byacc);
      bkacc = loc_wave_sum(bkacc);
      if (tid == 0) {   // the epilogue, in the order gpak_dev_local_ok.h states
        const double m = byacc / aacc;
        const double r = 1.0 - bkacc;
        const double tq = r / aacc;
        mean[b] = fma(r, m, macc);
        if (var) var[b] = fma(r, tq, kbb - qacc) + var_add;
        if (mu) mu[b] = m;
      }
    }
  }
}

// *info: INT_MAX before the kernel, 0 after it when no node failed; *nfail (may be null): 0 before the kernel
__global__ void gpak_local_info_f64(int *info, int phase, int *nfail) {
  if (phase == 0) { *info = INT_MAX; if (nfail) *nfail = 0; }
  else if (*info == INT_MAX) *info = 0;
}

namespace {
struct LocalTier { int smax; bool wave_nodes; };
LocalTier gpak_local_tier(int k) {
  if (k <= 16) return {16, true};
  if (k <= 32) return {32, true};
  if (k <= 64) return {64, false};
  return {GPAK_LOCAL_MAX, false};
}
int local_region(int smax, int nterms) {   // doubles of one node's LDS image
  return (smax + 2) * (smax + 1) + nterms * LOC_NC * smax + (smax + 1) / 2;
}

// one batch: nB nodes, every argument checked by the caller; OKM: ordinary kriging (mu may be null), else mu is not read
template <bool OKM>
void local_launch(hipStream_t st, int device, const double *P, int cap, int nB, int nd, const DevPoints &Q, const double *ys,
                  KernParams kp, double white, double noise, const int *nbr, int k, int flags, double *mean, double *var,
                  double *mu, int *info, int *nfail) {
  const LocalTier tier = gpak_local_tier(k);
  const int region = local_region(tier.smax, kp.nterms);   // the same image for both estimators
  const size_t lds = sizeof(double) * (size_t)region * (tier.wave_nodes ? LOC_WAVE_NODES : 1);
  {   // more than 64 KiB of dynamic LDS needs the opt-in, once per device
    static std::atomic<unsigned long long> done_mask{0};   // one per instantiation
    const unsigned long long bit = 1ull << (device & 63);
    if (!(done_mask.load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gpak_local_krige_f64<OKM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sizeof(double) * local_region(GPAK_LOCAL_MAX, GPAK_MAX_TERMS)));
      done_mask.fetch_or(bit, std::memory_order_release);
    }
  }
  kp.mode = GPAK_DIST_DIRECT;
  const int grid = tier.wave_nodes ? (nB + LOC_WAVE_NODES - 1) / LOC_WAVE_NODES : nB;
  const double var_add = (flags & GPAK_LOCAL_LATENT) ? 0.0 : (noise - white) / nd;
  hipLaunchKernelGGL(gpak_local_info_f64, dim3(1), dim3(1), 0, st, info, 0, nfail);
  hipLaunchKernelGGL(gpak_local_krige_f64<OKM>, dim3(grid), dim3(256), lds, st, P, cap, nB, nd, Q.base, Q.cap, Q.n, ys, kp, 1.0 / nd,
                     white / nd, noise, var_add, nbr, k, tier.smax, tier.wave_nodes ? 1 : 0, region, mean, var, mu, info, nfail);
  hipLaunchKernelGGL(gpak_local_info_f64, dim3(1), dim3(1), 0, st, info, 1, nfail);
}

struct Timer {   // device ms between two points of a stream, added up over the batches
  hipEvent_t a = nullptr, b = nullptr;
  double ms = 0.0;
  bool ok() { return (a || hipEventCreate(&a) == hipSuccess) && (b || hipEventCreate(&b) == hipSuccess); }
  void start(hipStream_t st) { hipEventRecord(a, st); }
  void stop(hipStream_t st) { hipEventRecord(b, st); }
  void collect() { float v = 0; if (hipEventElapsedTime(&v, a, b) == hipSuccess) ms += v; }
  ~Timer() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

// gpak_dev_local_krige and gpak_dev_local_krige_ok: one body, the estimator a template argument
template <bool OKM>
int dev_local_krige(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n, const double *ys,
                    const double *kern, double bias, int dist_mode, double white, double noise, const int *nbr, int k, int flags,
                    double *mean, double *var, double *mu, int *info) {
  if (!P || !u || !ys || !kern || !nbr || !mean || !info || nB < 1 || nd < 1 || n < 1 || cap < nB || ucap < n || k < 1 ||
      k > GPAK_LOCAL_MAX || (flags & ~GPAK_LOCAL_LATENT) || (size_t)cap * nd > ((size_t)1 << 30))
    return GPAK_EINVAL;
  KernParams kp;
  memset(&kp, 0, sizeof(kp));
  const int d4 = (dist_mode & GPAK_DIST_D4) ? 4 : 3;
  if (dist_mode & GPAK_DIST_HYB) {   // a serialized composition (gpak_dev.h)
    const int nterms = (int)kern[0];
    if (nterms < 1 || nterms > GPAK_MAX_TERMS) return GPAK_EINVAL;
    int kinds[GPAK_MAX_TERMS] = {0, 0, 0};
    for (int t = 0; t < GPAK_MAX_TERMS; t++) kinds[t] = (int)kern[1 + t];
    if (gpak_build_kp(nterms, kinds, kern + 5, bias, white, GPAK_DIST_DIRECT, &kp, nullptr) != GPAK_OK) return GPAK_EINVAL;
  } else {
    const int kinds[1] = {GPAK_KERN_EXPANS};
    if (gpak_build_kp(1, kinds, kern, bias, white, GPAK_DIST_DIRECT, &kp, nullptr) != GPAK_OK) return GPAK_EINVAL;
  }
  kp.d = d4;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return GPAK_EHIP;
  DevPoints Q;
  Q.base = const_cast<double *>(u); Q.n = n; Q.cap = ucap;
  local_launch<OKM>((hipStream_t)stream, device, P, cap, nB, nd, Q, ys, kp, white, noise, nbr, k, flags, mean, var, mu, info,
                    nullptr);
  return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP;
}
}  // namespace

extern "C" {

int gpak_dev_local_krige(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n,
                         const double *ys, const double *kern, double bias, int dist_mode, double white, double noise,
                         const int *nbr, int k, int flags, double *mean, double *var, int *info) {
  return dev_local_krige<false>(stream, P, cap, nB, nd, u, ucap, n, ys, kern, bias, dist_mode, white, noise, nbr, k, flags, mean,
                                var, nullptr, info);
}

int gpak_dev_local_krige_ok(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n,
                            const double *ys, const double *kern, double bias, int dist_mode, double white, double noise,
                            const int *nbr, int k, int flags, double *mean, double *var, double *mu, int *info) {
  return dev_local_krige<true>(stream, P, cap, nB, nd, u, ucap, n, ys, kern, bias, dist_mode, white, noise, nbr, k, flags, mean,
                               var, mu, info);
}

int gpak_local_metric(const gpak_ctx *ctx, int term, double *G) {
  if (!ctx || !G) return GPAK_EINVAL;
  gpak_ctx *c = const_cast<gpak_ctx *>(ctx);   // only the error text is written
  if (ctx->multi) { c->err = "gpak_local_metric is built for the single-GPU context (gpak_create) only"; return GPAK_ENOTIMPL; }
  if (!ctx->have_params) { c->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
  if (term < 0 || term >= ctx->kp.nterms) {
    c->err = "gpak_local_metric: term " + std::to_string(term) + " is outside the composition's " + std::to_string(ctx->kp.nterms);
    return GPAK_EINVAL;
  }
  const KernTerm &t = ctx->kp.term[term];
  for (int i = 0; i < 16; i++) G[i] = 0.0;
  for (int col = 0; col < 3; col++)
    for (int r = 0; r < 3; r++) G[r + 4 * col] = t.A[r + 3 * col];
  G[3 + 4 * 3] = t.a33;
  return GPAK_OK;
}

// the host driver of gpak_predict_local (okm false; mu is not read) and gpak_predict_local_ok (okm true; mu may be NULL)
static int predict_local_driver(gpak_ctx *ctx, const double *Xs, const double *ys, long Ns, int d, const double *Xd, long M,
                                int nd, const int *nbr, int k, double *mean, double *var, double *mu, int flags,
                                gpak_local_summary *summary, bool okm) {
  if (!ctx) return GPAK_EINVAL;
  const std::string who = okm ? "gpak_predict_local_ok: " : "gpak_predict_local: ";
  if (!okm) mu = nullptr;
  auto refuse = [&](int rc, const std::string &what) { ctx->err = who + what; return rc; };
  if (!Xs || !ys || !Xd || !nbr || !mean)
    return refuse(GPAK_EINVAL, std::string(!Xs ? "Xs" : !ys ? "ys" : !Xd ? "Xd" : !nbr ? "nbr" : "mean") + " is NULL");
  if (Ns < 1 || M < 1 || nd < 1 || Ns > (long)INT_MAX - 128)
    return refuse(GPAK_EINVAL, "Ns = " + std::to_string(Ns) + ", M = " + std::to_string(M) + ", nd = " + std::to_string(nd) +
                                   " must all be positive (Ns at most INT_MAX - 128)");
  if (k < 1 || k > GPAK_LOCAL_MAX) return refuse(GPAK_EINVAL, "k = " + std::to_string(k) + " is outside 1..128");
  if (flags & ~GPAK_LOCAL_LATENT)
    return refuse(GPAK_EINVAL, "flags = " + std::to_string(flags) + " has bits other than GPAK_LOCAL_LATENT");
  if (ctx->multi) return refuse(GPAK_ENOTIMPL, "built for the single-GPU context (gpak_create) only");
  if (d != 3 && d != 4) return refuse(GPAK_ENOTIMPL, "d = " + std::to_string(d) + ": the samples have 3 or 4 columns");
  if (ctx->N && d != ctx->d) return refuse(GPAK_ENOTIMPL, "the samples must have as many columns as the context's training set");
  if (!ctx->have_params) { ctx->err = "no parameters (gpak_set_params)"; return GPAK_ESTATE; }
  long empty = 0;
  int max_used = 0;
  for (long b = 0; b < M; b++) {
    const int *l = nbr + (size_t)k * b;
    int s = 0;
    while (s < k && l[s] >= 0) s++;
    for (int e = 0; e < k; e++) {
      if (l[e] < -1 || l[e] >= Ns)
        return refuse(GPAK_EINVAL, "node " + std::to_string(b) + " names sample " + std::to_string(l[e]) + ", outside -1.." +
                                       std::to_string(Ns - 1));
      if (e >= s && l[e] != -1) return refuse(GPAK_EINVAL, "node " + std::to_string(b) + " names a sample after a -1");
    }
    if (!s) empty++;
    max_used = std::max(max_used, s);
  }

  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  KernParams kp = ctx->kp;
  kp.d = d;
  kp.mode = GPAK_DIST_DIRECT;
  for (int c = 0; c < 4; c++) kp.mu[c] = 0.0;
  for (int c = 0; c < d; c++) {   // centred on the samples' column means
    double sum = 0.0;
    for (long i = 0; i < Ns; i++) sum += Xs[i + (size_t)c * Ns];
    kp.mu[c] = sum / (double)Ns;
  }
  const double white = ctx->kp.white, noise = ctx->sn2 + white;
  // the nodes of a batch: GPAK_OPT_PRED_BATCH, the raw and transformed points under 1 GiB as on the block path
  long cap_l = ctx->sched.pred_batch > 0 ? ctx->sched.pred_batch : 16384;
  cap_l = std::min(cap_l, M);
  const size_t per_node = sizeof(double) * (size_t)nd * (4 + GPAK_PT * (size_t)kp.nterms);
  while (cap_l > 1 && (size_t)cap_l * per_node > ((size_t)1 << 30)) cap_l /= 2;
  if ((size_t)cap_l * nd > ((size_t)1 << 30)) return refuse(GPAK_EINVAL, "too many discretisation points per block");
  const int cap = (int)cap_l;
  const int capS = (int)((Ns + GPAK_TILE - 1) / GPAK_TILE * GPAK_TILE);

  // buffers of the call's own: nothing of the context's is touched
  DevPointsBuf Us;
  DevBuf<double> dRaw, dYs, dXblk, dTblk, dOut;
  DevBuf<int> dNbr, dInfo;
  const bool ok = Us.reserve(capS) && dRaw.reserve((size_t)d * Ns) && dYs.reserve((size_t)Ns) &&
                  dXblk.reserve((size_t)d * cap * nd) && dTblk.reserve((size_t)GPAK_PT * kp.nterms * cap * nd) &&
                  dOut.reserve((okm ? 3 : 2) * (size_t)cap) && dNbr.reserve((size_t)k * cap) && dInfo.reserve(2);
  if (!ok) {
    (void)hipGetLastError();
    return refuse(GPAK_ENOMEM, "device allocation failed for the transformed samples (15 doubles each) or a node batch");
  }
  Timer t_all, t_up, t_krige;
  if (!t_all.ok() || !t_up.ok() || !t_krige.ok()) { ctx->err = "hipEventCreate failed"; return GPAK_EHIP; }
  t_all.start(st);
  t_up.start(st);
  GPAK_HIP(hipMemcpyAsync(dRaw, Xs, sizeof(double) * (size_t)d * Ns, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dYs, ys, sizeof(double) * (size_t)Ns, hipMemcpyHostToDevice, st));
  gpak_launch_transform(st, dRaw, (int)Ns, (int)Ns, kp, Us);
  t_up.stop(st);
  GPAK_HIP(hipStreamSynchronize(st));
  dRaw.release();

  double *dMean = dOut, *dVar = dOut + cap, *dMu = okm ? dOut + 2 * (size_t)cap : nullptr;
  const long Mn = M * nd;
  long notpd = 0;
  int batches = 0;
  t_krige.start(st);
  for (long b0 = 0; b0 < M; b0 += cap, batches++) {
    const int mb = (int)std::min<long>(cap, M - b0);
    const long xs = (long)mb * nd;
    for (int c = 0; c < d; c++)
      GPAK_HIP(hipMemcpyAsync(dXblk + (size_t)c * xs, Xd + (size_t)c * Mn + (size_t)b0 * nd, sizeof(double) * xs,
                              hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(dNbr, nbr + (size_t)k * b0, sizeof(int) * (size_t)k * mb, hipMemcpyHostToDevice, st));
    gpak_launch_transform_blocks(st, dXblk, xs, mb, nd, cap, kp, dTblk);
    if (okm)
      local_launch<true>(st, ctx->device, dTblk, cap, mb, nd, Us, dYs, kp, white, noise, dNbr, k, flags, dMean,
                         var ? dVar : nullptr, mu ? dMu : nullptr, dInfo, dInfo + 1);
    else
      local_launch<false>(st, ctx->device, dTblk, cap, mb, nd, Us, dYs, kp, white, noise, dNbr, k, flags, dMean,
                          var ? dVar : nullptr, nullptr, dInfo, dInfo + 1);
    int hinfo[2] = {0, 0};   // the smallest failing node + 1, the number of failing nodes
    GPAK_HIP(hipMemcpyAsync(mean + b0, dMean, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    if (var) GPAK_HIP(hipMemcpyAsync(var + b0, dVar, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    if (mu) GPAK_HIP(hipMemcpyAsync(mu + b0, dMu, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipMemcpyAsync(hinfo, dInfo, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipStreamSynchronize(st));
    GPAK_HIP(hipGetLastError());
    notpd += hinfo[1];
  }
  t_krige.stop(st);
  t_all.stop(st);
  GPAK_HIP(hipStreamSynchronize(st));
  t_all.collect(); t_up.collect(); t_krige.collect();
  ctx->times.predict_ms = t_all.ms;
  if (summary) {
    summary->upload_ms = t_up.ms;
    summary->krige_ms = t_krige.ms;
    summary->nodes = M;
    summary->empty = empty;
    summary->notpd = notpd;
    summary->batches = batches;
    summary->max_used = max_used;
  }
  return GPAK_OK;
}

int gpak_predict_local(gpak_ctx *ctx, const double *Xs, const double *ys, long Ns, int d, const double *Xd, long M, int nd,
                       const int *nbr, int k, double *mean, double *var, int flags, gpak_local_summary *summary) {
  return predict_local_driver(ctx, Xs, ys, Ns, d, Xd, M, nd, nbr, k, mean, var, nullptr, flags, summary, false);
}

int gpak_predict_local_ok(gpak_ctx *ctx, const double *Xs, const double *ys, long Ns, int d, const double *Xd, long M, int nd,
                          const int *nbr, int k, double *mean, double *var, double *mu, int flags,
                          gpak_local_summary *summary) {
  return predict_local_driver(ctx, Xs, ys, Ns, d, Xd, M, nd, nbr, k, mean, var, mu, flags, summary, true);
}

}  // extern "C"
