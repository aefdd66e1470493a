// gpak_internal.h -- shared declarations of libgpak_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/gpak.h"
#include "../../include/gpak_design.h"   // gpak_design_summary (gpak_design_impl)
#include "../../include/gpak_condition.h"   // gpak_condition_summary (gpak_condition_impl)
#include "ctx_state.h"  // CtxState: what of a context's device contents is current (HIP-free)
#include "potrf_plan.h"  // GPAK_TILE, GpakSchedule and the factorisation's schedule (HIP-free)

// The covariance function as the device sees it: a SUM of up to three stationary terms (the
// children of the reference's HybKerns, Kernel.cpp:140-154), a constant and a white-noise diagonal.
//   term t:  k_t(x, x') = var2 * profile( D2_t ),  D2_t = |(x - x') A_t|^2
//   profile 0: exp(-sqrt(D2))        Kern_ExpAnisotropic (A = Rot diag(L) Rot^T, Kernel.cpp:1399-1425)
//                                    Kern_Exponential    (A = I / Hayper_Euc_Exp, Kernel.cpp:1343-1368, 1437-1441)
//   profile 1: exp(-0.5 * iw * D2)   Kern_RBF            (A = I / Hayper_Euc_RBF, Kernel.cpp:482-488)
#define GPAK_MAX_TERMS 3
#define GPAK_PROFILE_EXPSQRT 0
#define GPAK_PROFILE_RBF 1
struct KernTerm {
  double A[9];   // column-major 3x3 metric factor
  double a33;    // factor of a 4th input column (rock type): InversewidthR for ExpAns
                 // (Kernel.cpp:1411-1424, A(3,3) = L_r), the isotropic scale for Exp / RBF (EuclDist)
  double var2;   // Sigma^2
  double iw;     // inverseWidth_RBF (profile 1 only)
  int profile;
};
struct KernParams {
  KernTerm term[GPAK_MAX_TERMS];
  int nterms;
  double mu[4];  // pooled mean used for centring (Kernel.cpp:1391-1397)
  int d;         // input columns: 3, or 4 (x, y, z, rock type)
  double bias;   // Kern_Bias Sigma_Bias (Kernel.cpp:366), added to every entry
  double white;  // Kern_White Sigma_White (Kernel.cpp:256-263), added where i == j of the same set
  int mode;      // GPAK_DIST_*
};

// A transformed point set on the device: for each term u = (x - mu) A_t, SoA, plus |u|^2:
// array c (0..2 = u0,u1,u2; 3 = |u|^2; 4 = u3, the transformed 4th column, zero for 3-D inputs) of
// term t is base + (GPAK_PT * t + c) * cap.
#define GPAK_PT 5
#define GPAK_PARR(base, cap, t, c) ((base) + (size_t)(GPAK_PT * (t) + (c)) * (cap))
// A device allocation and its owner: freed with whatever holds it, never copied.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;   // elements allocated
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  operator T *() const { return p; }
  // room for at least `elems` elements: grows only, contents are not kept.  false: the allocation failed, the buffer is empty
  bool reserve(size_t elems) {
    if (n >= elems) return true;
    release();
    if (hipMalloc(&p, sizeof(T) * elems) != hipSuccess) { p = nullptr; return false; }
    n = elems;
    return true;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr; n = 0;
  }
};

struct DevPoints {
  double *base = nullptr;
  int n = 0;    // valid points
  int cap = 0;  // allocated points (multiple of GPAK_TILE)
};
// A point set with its owner: what a context allocates.  The launchers take the DevPoints it is (dev_api.hip makes such
// views of points it does not own).
struct DevPointsBuf : DevPoints {
  DevBuf<double> mem;
  bool reserve(int points) {   // as DevBuf::reserve
    if (cap >= points) return true;
    release();
    if (!mem.reserve(GPAK_PT * GPAK_MAX_TERMS * (size_t)points)) return false;
    base = mem; cap = points;
    return true;
  }
  void release() { mem.release(); base = nullptr; n = cap = 0; }
};

// ---- tuning, part 2: kernel selection ------------------------------------------------------------------------
// Part 1, the schedule set that a context copies and gpak_set_option changes, is GpakSchedule in potrf_plan.h.
// What the launchers of gemm.hip / gemm_f32.hip / gram.hip / potrf.hip read has no context to live in: this set is
// process-wide and read only through gpak_tuning().  Same rules for the values: the defaults below, overridden once,
// at the first call, by the GPAK_* environment variables of the same names; gpak_reload_tuning() re-reads them.
struct GpakKernelTuning {
  int sbase_rows = 0;          // GPAK_SBASE_ROWS      bulk updates of more rows than this use the scalar-base build of the kernel (0: never;
                               //                      measured slower in situ at every threshold: profiles/r03_scalar_base.txt)
  int gemm_small = 160;        // GPAK_GEMM_SMALL      tile grids up to this size take the latency kernel
  int gemm_small_rows = 16;    // GPAK_GEMM_SMALL_ROWS rows per workgroup of that kernel: 16 / 32 / 64
  int super_lr = 3;            // GPAK_SUPER_LR      bulk update: super-tiles of 2^lr x 2^(6-lr) tiles per XCD (3 = 8 x 8)
  int potrf_co = 1;            // GPAK_POTRF_CO      as GpakSchedule::potrf_co, for panels factored without a context (gpak_dev.h)
  bool fill_fast = true;       // GPAK_FILL_FAST     table exp + in-line sqrt fill / Gram-matvec
  bool kmv_sym = true;         // GPAK_KMV_SYM       symmetric Gram-matvec from 32 macro blocks on
  // fp32 prediction (GPAK_F32 contexts)
  bool f32_wide = true;        // GPAK_F32_ACC=plain switches the fp64 accumulation of the fp32 products off
  int f32_rsd = 4;             // GPAK_F32_RSD       operand prefetch depth of the wide-accumulation kernel: 2 / 4 / 8
  int f32_tile = 128;          // GPAK_F32_TILE      wave tile rows of the plain fp32 kernel: 128 / 64
};
const GpakKernelTuning &gpak_tuning();

struct gpak_multi;   // multi.hip: one process driving several GPUs (gpak_create_multi)

// The streams and events of a context.  A base of gpak_ctx and not members of it, so that they are destroyed AFTER the
// context's buffers have been freed -- the order gpak_destroy has always had: the first hipFree waits for the device.
struct gpak_queues {
  hipStream_t stream = nullptr;     // main stream: fill, bulk trailing updates, solves
  hipStream_t stream_hi = nullptr;  // high-priority stream: panel factorisation (look-ahead)
  hipStream_t stream_tail = nullptr;  // CU-masked copy of the main stream for the tail's bulk updates (optional)
  hipStream_t stream_bulk = nullptr;  // the bulk updates' own queue before the tail: created like stream_tail but with every CU enabled (optional)
  hipStream_t stream_fs = nullptr;  // forward substitution riding along with the factorisation, off the panel chain
  hipStream_t stream_x = nullptr;   // tail: K=128 updates of the next block column, sub-panel by sub-panel
  hipEvent_t ev[10] = {};            // timing
  std::vector<hipEvent_t> ev_pool;   // timing events around the trailing updates
  std::vector<hipEvent_t> ev_sync;   // cross-stream dependencies of the look-ahead pipeline
  std::vector<hipEvent_t> ev_cvf;    // timing: three per one-at-a-time group of gpak_cv_folds
  gpak_queues() = default;
  gpak_queues(const gpak_queues &) = delete;
  ~gpak_queues();   // api.hip.  Nothing of the device for a group's context, which has none of these
};

struct gpak_ctx : gpak_queues {
  gpak_multi *multi = nullptr;   // set: every call is forwarded to the group; the fields below are unused and own nothing
  int device = 0;
  int cu_count = 0;                 // compute units of the device (gpak_potrf_block_co)
  int precision = GPAK_F64;
  std::string err;

  // what of the device contents below is current: every validity fact, changed through its events only
  CtxState state;

  // training set (release_train, api.hip, says which buffers go with it)
  int N = 0, Np = 0, ld = 0, d = 0;
  DevBuf<double> dX;         // raw input columns (3 or 4), SoA with stride Np (4 arrays, the 4th zero for d = 3)
  DevBuf<double> dy;         // Np (padded with 0)
  std::vector<double> hX;    // host copy of X (col-major N x d), for pooled means
  double xsum[4] = {0, 0, 0, 0};

  // parameters
  bool have_params = false;
  double expans[8] = {0};   // ExpAns parameters when the kernel is the reference's default composition
  bool expans_only = true;  // kernel == ExpAns(+Bias): the composition of the fixed-length gpak_grad
  int kinds[GPAK_MAX_TERMS] = {0, 0, 0};  // GPAK_KERN_* of each stationary term
  double tpars[GPAK_MAX_TERMS][8] = {{0}};  // raw parameters of each stationary term, the reference's order (gpak_grad_exact)
  double bias = 0, sn2 = 0;
  int dist_mode = GPAK_DIST_DIRECT;
  KernParams kp;
  double kdiag = 0;          // diag_Compute of the composition (Kernel.cpp:127-136)

  // device state
  DevPointsBuf U;            // transformed training points
  DevBuf<double> dM;         // Np x ld matrix buffer: B then L (lower)
  DevBuf<double> dInv;       // (Np/128) inverted 128x128 diagonal blocks of L
  DevBuf<double> dInv512;    // explicit (L_bb^-1)^T of the bw x bw diagonal blocks (bw = bwd_bw; back substitution)
  int bwd_bw = 512;          // block width dInv512 was sized and is being built for
  DevBuf<double> dT512;      // bwd_fused = 2: per block column the stacked [R_b ; T_b], T_b = L[b, b-1]^T R_b (2 bw x bw: solve.hip)
  DevBuf<double> dAlpha;     // Np
  DevBuf<double> dWork;      // 4*Np scratch vectors
  // (the buffers that outlive a training set are declared in the reverse of the order gpak_destroy has always freed them
  // in: members go last-declared first, and the order of the frees decides which addresses the next context is given)
  DevBuf<unsigned long long> dTickets;   // ticketed bulk updates: 8 list words per bulk launch, zeroed per factorisation
  DevBuf<int> dInfo;         // first failing column (1-based) or 0
  DevBuf<double> dRed;       // small reduction scratch
  double quad = 0, sumlp = 0, logdet = 0, nlz = 0;

  // prediction buffers (grown on demand, kept across calls and training sets; declared in reverse like the three above)
  DevBuf<double> dPart;      // 64 x pred_cap partial sums
  DevBuf<double> dPv;        // 2 x pred_cap: mean, sum of squares
  DevBuf<double> dWt;        // pred_cap x Np cross-kernel, test-major (transposed kX)
  DevBuf<double> dXte;       // 4 x pred_cap raw test columns (SoA)
  DevPointsBuf Tq, Upred;    // test-batch / train points centred on the pooled train+test mean
  int pred_cap = 0;          // dXte, dPv, dPart and Tq grow together on it
  // joint prediction / simulation (gpak_predict_joint, gpak_sample_joint): the joint_cap x joint_cap covariance and then
  // its factor (leading dimension skewed like dWt's), that factor's inverted 128-blocks and failing column, and the
  // normals / realisations
  DevBuf<double> dZ, dXi;
  DevBuf<int> dCinfo;
  DevBuf<double> dCinv, dC;
  int joint_cap = 0;
  // block-support prediction (gpak_predict_block): a batch's discretisation points, raw (4 columns) and transformed
  // point-major (gpak_transform_blocks_f64), blk_points points of blk_terms terms each
  DevBuf<double> dTblk, dXblk;
  size_t blk_points = 0;
  int blk_terms = 0;
  // the fills, the substitution, the SYRK, the first score pass and the last pick's downdate of the last gpak_design, in ms
  double design_ms[5] = {0, 0, 0, 0, 0};
  // gpak_condition / gpak_sample_path (condition.hip), kept across calls: A (Np x (S + 1)) and, for the comparison path, its
  // transpose; Ysim (Np x S) and Ysim^T / sn2 realisation-major for the batched substitution; a batch's Z and F0; the slab partials of the fused product / the GEMMs' output; and of the
  // spectral prior the features of a chunk, W^T, the frequencies, the features' terms and sqrt(c) b0
  DevBuf<double> dCondA, dCondAt, dCondY, dCondYt, dCondZ, dCondF, dCondPart, dCondPhi, dCondW, dCondOm, dCondB0;
  DevBuf<int> dCondFt;
  // fp32 prediction (ctx created with GPAK_F32): fp32 images of L and of the inverse blocks (CtxState::image)
  DevBuf<float> dLf, dInvf;
  long ldLf = 0;             // leading dimension of dLf (Np + skew)

  // gradient buffers (allocated on the first gpak_grad)
  DevBuf<double> dG;         // Np x ld: L^-T (upper triangular)
  DevBuf<double> dBinv;      // Np x ld: B^-1, lower tiles.  Allocated with dG: dG != NULL means that dBinv exists too
  DevBuf<double> dF;         // Np: f = K*alpha of the last logLikelihood()
  DevBuf<double> dGpart;     // per-workgroup partial sums of the pair pass; shared scratch whose contents nobody keeps
  // leave-one-out (gpak_loo): a slab of rows of L^-T of its own when the gradient has not allocated dG; leave-group-out
  // (gpak_cv_groups) holds all of L^-T, in dG when the gradient has allocated it, otherwise here (gpak_loo_workspace)
  DevBuf<double> dLoo;
  int loo_rows = 0;           // GPAK_OPT_LOO_ROWS: rows of L^-T held at once (0: the default, 16384)
  // the substitution, the Gram pass and the solve pass of the last gpak_cv_groups, in ms
  double cvg_ms[3] = {0, 0, 0};
  // k-fold cross-validation (gpak_cv_folds), the groups above GPAK_CV_GROUP_MAX one at a time, sized by the largest such
  // group (m_p = its size rounded up to 128) and kept across calls: the packed rows P of G (m_p x (Np - k0)) and then
  // T = R^-T in its place, S = P P^T and then its factor R (m_p x m_p), R's inverted 128-blocks, the vectors w, e, var
  DevBuf<double> dCvfVec, dCvfInv, dCvfS, dCvfP;
  // gpak_cv_folds_grad: the weight factors Q_I (m_p x m_p each) of all those groups, one after another
  DevBuf<double> dCvfQ;
  // the substitution, the batched small groups, and pack / product / factor + inverse + finish summed over the other
  // groups of the last gpak_cv_folds, in ms
  double cvf_ms[5] = {0, 0, 0, 0, 0};

  // options
  GpakSchedule sched;         // this context's copy of the schedule set (gpak_set_option changes it)
  bool profile = false;

  // timing
  gpak_phase_times times;
};

#define GPAK_HIP(call)                                                                  \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
      return GPAK_EHIP;                                                                 \
    }                                                                                   \
  } while (0)

// ---- device math for the covariance profile ------------------------------------------------
// exp(-sqrt(D2)) costs ~100 instruction slots per matrix element through the device libm (the fill is then
// ALU-bound: 1.57 ms against 0.85 ms for the stores alone); these two cost ~30 and stay within 2 ulp.
#ifdef __HIPCC__
// sqrt(d), d >= 0 finite: v_rsq_f64 + two Goldschmidt steps + one residual correction
__device__ __forceinline__ double gpak_sqrt_nonneg(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  double g = d * y, h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  g = fma(fma(-g, g, d), h, g);
  return d > 0.0 ? g : d;    // d == 0 (rsq(0) = inf) gives 0; a NaN coordinate stays NaN
}
// exp(x), x <= 0 finite: x = n ln2 + r, |r| <= 0.35, Taylor polynomial of degree 13 (remainder 4e-18), ldexp
__device__ __forceinline__ double gpak_exp_nonpos(double x) {
  // n = rint(x log2 e) by the 1.5 * 2^52 trick: the integer sits in the low mantissa bits of t
  const double t = fma(x, 1.4426950408889634074, 6755399441055744.0);
  const double n = t - 6755399441055744.0;
  double r = fma(n, -6.93147180369123816490e-01, x);
  r = fma(n, -1.90821492927058770002e-10, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  // 2^n assembled in the exponent field (n clamped at -1022: results below 2^-1022 are not distinguished)
  int ni = __double2loint(t);
  ni = ni < -1022 ? -1022 : ni;
  return p * __hiloint2double((ni + 1023) << 20, 0);
}
// D2 (Kernel.cpp:1431-1434 / :1365-1367, or the cancellation-free equivalent)
__device__ __forceinline__ double gpak_d2(double p0, double p1, double p2, double ps, double p3, double q0,
                                          double q1, double q2, double qs, double q3, int mode) {
  if (mode == GPAK_DIST_DIRECT) {
    double a = p0 - q0, b = p1 - q1, c = p2 - q2, e = p3 - q3;
    return a * a + b * b + c * c + e * e;  // e == 0 for 3-D inputs: the value is unchanged bit for bit
  }
  double dot = p0 * q0 + p1 * q1 + p2 * q2 + p3 * q3;
  double v = ps + qs - 2.0 * dot;
  return v < 0.0 ? 0.0 : v;
}
// var2 * profile(D2): Kernel.cpp:881 (ExpAns / Exp), :487 (RBF)
__device__ __forceinline__ double gpak_profile(double d2, const KernTerm &t) {
  return t.var2 * gpak_exp_nonpos(t.profile == GPAK_PROFILE_RBF ? -0.5 * t.iw * d2 : -gpak_sqrt_nonneg(d2));
}

// The same function with a 32-entry table of 2^(j/32) (kept in LDS by the caller: 32 doubles span the 64 banks exactly
// once, so any index pattern of a wave is conflict-free): x = (32 m + j) ln2/32 + r, |r| <= ln2/64, Taylor polynomial of
// degree 6 (remainder 3e-18 relative) -- 12 fp64 instructions instead of 19, <= 2 ulp (checked against mpmath on
// 3e4 arguments in [-700, 0]).  Results below 2^-1074 flush to 0 through v_ldexp_f64.
#define GPAK_EXPTAB_N 32
static __constant__ double gpak_exp2_tab[GPAK_EXPTAB_N] = {
    0x1.0000000000000p+0, 0x1.059b0d3158574p+0, 0x1.0b5586cf9890fp+0, 0x1.11301d0125b51p+0, 0x1.172b83c7d517bp+0,
    0x1.1d4873168b9aap+0, 0x1.2387a6e756238p+0, 0x1.29e9df51fdee1p+0, 0x1.306fe0a31b715p+0, 0x1.371a7373aa9cbp+0,
    0x1.3dea64c123422p+0, 0x1.44e086061892dp+0, 0x1.4bfdad5362a27p+0, 0x1.5342b569d4f82p+0, 0x1.5ab07dd485429p+0,
    0x1.6247eb03a5585p+0, 0x1.6a09e667f3bcdp+0, 0x1.71f75e8ec5f74p+0, 0x1.7a11473eb0187p+0, 0x1.82589994cce13p+0,
    0x1.8ace5422aa0dbp+0, 0x1.93737b0cdc5e5p+0, 0x1.9c49182a3f090p+0, 0x1.a5503b23e255dp+0, 0x1.ae89f995ad3adp+0,
    0x1.b7f76f2fb5e47p+0, 0x1.c199bdd85529cp+0, 0x1.cb720dcef9069p+0, 0x1.d5818dcfba487p+0, 0x1.dfc97337b9b5fp+0,
    0x1.ea4afa2a490dap+0, 0x1.f50765b6e4540p+0};
// exp(-s), s >= 0 finite (NaN stays NaN); tab = the table above in LDS
__device__ __forceinline__ double gpak_exp_neg_tab(double s, const double *tab) {
  const double t = fma(s, -0x1.71547652b82fep+5, 6755399441055744.0);   // n = rint(-s * 32/ln2) in the low mantissa bits
  const double n = t - 6755399441055744.0;
  double r = fma(n, -0x1.62e42fefa0000p-6, -s);                         // ln2/32 split so that n * hi is exact
  r = fma(n, -0x1.cf79abc9e3b3ap-45, r);
  double p = 0x1.6c16c16c16c17p-10;                                     // 1/720
  p = fma(p, r, 0x1.1111111111111p-7);
  p = fma(p, r, 0x1.5555555555555p-5);
  p = fma(p, r, 0x1.5555555555555p-3);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const int ni = __double2loint(t);
  return ldexp(tab[ni & (GPAK_EXPTAB_N - 1)] * p, ni >> 5);
}
// sqrt(d) for the argument of exp(-sqrt(d)): v_rsq_f64 + two Goldschmidt steps, no final residual correction (an ulp
// or two in s is an absolute 1e-16 * s in the exponent)
// The argument is clamped at 640000 (s = 800: exp(-s) has flushed to 0 long before, at s = 745) so that the table
// exponent of gpak_exp_neg_tab -- rint(-s 32/ln2) read from 32 mantissa bits -- can never wrap (it did for s > 4.65e7
// and gave +inf), and an overflowed D2 = +inf yields K = bias instead of NaN.  Only the HIGH dword is replaced (one
// v_cmp_gt_f64 + one v_cndmask_b32; whatever the low dword holds, the result still flushes); a NaN coordinate fails
// the comparison and stays NaN.
__device__ __forceinline__ double gpak_sqrt_nonneg_fast(double d) {
  d = __hiloint2double(d > 640000.0 ? 0x41238800 : __double2hiint(d), __double2loint(d));   // 640000.0 = 0x4123880000000000
  const double y = __builtin_amdgcn_rsq(d);
  double g = d * y, h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  return d > 0.0 ? g : d;
}
#endif

// ---- gram.hip ---------------------------------------------------------------------------
// u = (x - mu) A for n points; x SoA with stride xs.
void gpak_launch_transform(hipStream_t st, const double *x, int xs, int n, const KernParams &kp,
                           DevPoints &out);
// Fill C (rows x cols tile grid, ld) with scale*K(P_i,Q_j) + diag*delta_ij; rows/cols beyond
// the valid counts get delta_ij. lower_only skips tiles strictly above the diagonal.
void gpak_launch_fill(hipStream_t st, const DevPoints &P, const DevPoints &Q, int rows_p, int cols_p,
                      const KernParams &kp, double scale, double diag, double pad_diag, int lower_only,
                      double *C, long ld, double *D2out, int col_off = 0);
// Block-support prediction: the points of nb blocks of nd points each, x[k * xs + r * nd + a], transformed into out
// point-major (point a of block r at a * cap + r, arrays nd * cap apart); the block-averaged cross-kernel of those
// blocks against Q, rows_p x cols_p in the fill's layout; kbb[r] = the prior variance of block r's average.
void gpak_launch_transform_blocks(hipStream_t st, const double *x, long xs, int nb, int nd, int cap,
                                  const KernParams &kp, double *out);
void gpak_launch_fill_blocks(hipStream_t st, const double *P, int cap, int nB, int nd, const DevPoints &Q, int rows_p,
                             int cols_p, const KernParams &kp, double *C, long ld);
void gpak_launch_block_self(hipStream_t st, const double *P, int cap, int nB, int nd, const KernParams &kp, double *kbb);
// Joint prediction: the prior covariance between the averages of the same blocks, lower 128 x 64 tiles of the cap x cap
// matrix C; b == b' gets `diag` beside its average, padding rows / columns 0 off the diagonal and 1 on it.
void gpak_launch_fill_block_pairs(hipStream_t st, const double *P, int cap, int nB, int nd, const KernParams &kp,
                                  double diag, double *C, long ld);
// out_j = sum_i w_i K(P_i, Q_j), j < Q.n   (fused Gram-matvec; K never stored).
// scratch holds max(splits, scratch_rows) * Q.cap doubles (scratch_rows: what the caller really has; the symmetric
// kernel for P == Q needs one row per 512 points).
int gpak_kmatvec_splits(int nP, int nQ);
void gpak_launch_kmatvec(hipStream_t st, const DevPoints &P, int p_off, int np, const double *w, const DevPoints &Q,
                         const KernParams &kp, double *scratch, int splits, double *out, int scratch_rows = 0);
void gpak_launch_sum_splits(hipStream_t st, const double *part, int part_ld, int splits, int n, double *out);
int gpak_alloc_points(gpak_ctx *ctx, DevPointsBuf &p, int cap);   // DevPointsBuf::reserve with the context's error text
void gpak_pooled_mean(const double *s1, long n, const double *s2, long m, double *mu);
int gpak_ensure_U(gpak_ctx *ctx);

// ---- gemm.hip ---------------------------------------------------------------------------
// C[mt x nt tiles of 128] = beta*C + alpha * A (m x K) * B (n x K)^T, all column-major.
// lower_skip: skip tile (ti,tj) when row_block0+ti < col_block0+tj.
// trailing=true selects the instantiation gpak_gemm_nt_f64_rs<4, 2, true> (its own line in profiles).
// tickets (the factorisation's bulk update, lower_skip with row_block0 == col_block0): the ticketed tile map -- eight
// zeroed 64-bit list words of this launch's own, surplus_pct % more workgroups than tiles (gemm.hip, TICKET).
void gpak_launch_gemm_nt(hipStream_t st, int mt, int nt, int K, double alpha, const double *A, long lda,
                         const double *B, long ldb, double beta, double *C, long ldc, int row_block0,
                         int col_block0, bool lower_skip, bool trailing, bool k0_by_row = false,
                         unsigned long long *tickets = nullptr, int surplus_pct = 0);

void gpak_launch_gemm_nt_k0map(hipStream_t st, int mt, int nt, int K, double alpha, const double *A, long lda,
                               const double *B, long ldb, double *C, long ldc, int skip_shift, int k0_mul, int k0_add);
int gpak_calibrate_impl(gpak_ctx *ctx, double *scratch, size_t scratch_bytes, double *tflops, double *gbs);
void gpak_launch_gemm_cyclic(hipStream_t st, int mt, int nt, int K, const double *Pv, long ldp, double *Clocal,
                             long ldc, int rt0, int P, int rank, int tpb, int lt0);

// ---- gemm_f32.hip (fp32 prediction path) ---------------------------------------------------
void gpak_launch_gemm_nt_f32(hipStream_t st, int mt, int nt, int K, float alpha, const float *A, long lda,
                             const float *B, long ldb, float beta, float *C, long ldc);
void gpak_launch_lower_to_f32(hipStream_t st, const double *L, long ld, int Np, float *out, long ldo);
void gpak_launch_vec_to_f32(hipStream_t st, const double *in, size_t n, float *out);
void gpak_launch_fill_f32(hipStream_t st, const DevPoints &P, const DevPoints &Q, int rows_p, int cols_p,
                          const KernParams &kp, float *C, long ld);
void gpak_launch_rowsumsq_f32(hipStream_t st, const float *V, long ldv, int rows, int cols, int splits,
                              double *part, int part_ld);
// What the fp32 forward substitution reads beside the batch (predict.hip): the fp32 image of the factor and of the
// inverse diagonal blocks (pairs of 128 x 128, the first image of a pair is used).  A context's own (gpak_predict_impl) or
// a caller's (gpak_dev_fwd_subst_f32).
struct GpakFsF32 {
  hipStream_t stream;
  const float *Lf;
  long ldLf;
  const float *invf;
};
// Wt (mrows x Np, ld ldw) := Wt Lf^-T by the ladder `levels` (ascending block widths, the first 128; empty: 128 / 512)
void gpak_forward_subst_f32(const GpakFsF32 &f, float *Wt, long ldw, int mrows, int Np, std::vector<int> levels);

// ---- potrf.hip --------------------------------------------------------------------------
// Factor the 128x128 block at A (ld) in place (lower), write its inverse to inv (128x128, ld 128).
void gpak_launch_potrf128(hipStream_t st, double *A, long ld, double *inv, int col0, int *info, bool zero_inv,
                          bool co = false, int co_mode = -1);
int gpak_potrf_blocked(gpak_ctx *ctx);
void gpak_factor_panel(hipStream_t st, double *M, long ld, int Np, int J, int W, double *inv_base, int *info,
                       bool zero_inv, bool co = false, int co_mode = -1, hipEvent_t gate = nullptr);

// ---- solve.hip --------------------------------------------------------------------------
// x := L^-1 x ; x := L^-T x  (x has Np entries) using the inverted diagonal blocks.
// x is consumed (overwritten with intermediate values); the solution is written to out.
void gpak_launch_trsv_fwd(hipStream_t st, int Np, const double *L, long ld, const double *inv, double *x,
                          double *out);
// two-level variant: z is read-only, scratch holds 8 * 512 doubles
void gpak_launch_trsv_bwd_block2(hipStream_t st, int Np, int J, int W, const double *L, long ld, const double *inv,
                                 const double *z, double *out, double *scratch, const double *Rinv = nullptr, int NB = 512);
// R = (L_bb^-1)^T of the W x W diagonal block at J (W <= 512), column-major ld 512; seven small GEMM launches
void gpak_launch_diag_inverse(hipStream_t st, int J, int W, const double *L, long ld, const double *inv, double *R,
                              int RL = 512, int extra = 0);
void gpak_launch_trsv_bwd2(hipStream_t st, int Np, const double *L, long ld, const double *inv, const double *z,
                           double *out, double *scratch, const double *RinvB = nullptr, int bw = 512);
// far column dots of the next block column under the diagonal step of this one (solve.hip): scratch 18 * NB doubles,
// OP = per block column R_b (and, with_T, T_b in the rows below it: gpak_launch_diag_inverse with extra = NB)
void gpak_launch_trsv_bwd3(hipStream_t st, int Np, const double *L, long ld, const double *z, double *out, double *scratch,
                           const double *OP, size_t op_stride, int RL, bool with_T, int NB);
// out = L^-T z with whatever the context's current factor supports (CtxState::backsolve); z is read-only, scratch
// holds what the launcher it picks asks for: at most max(8 + bw / 32, 18) * bw doubles, bw = ctx->bwd_bw
void gpak_backsolve(gpak_ctx *ctx, hipStream_t st, const double *z, double *out, double *scratch);
void gpak_launch_trsv_fwd_block(hipStream_t st, int Np, int J, int W, const double *L, long ld,
                                const double *inv, double *x, double *out);
void gpak_launch_trsv_bwd_block(hipStream_t st, int J, int W, const double *L, long ld, const double *inv,
                                double *x, double *out);
void gpak_launch_coldot(hipStream_t st, int Np, int i0, int J, int W, const double *L, long ld, const double *x,
                        double *s);
void gpak_launch_logdiag_block(hipStream_t st, int J, int W, int N, const double *L, long ld, double *out);
// red[0] = sum log L_ii (i < N)
void gpak_launch_logdet(hipStream_t st, int N, const double *L, long ld, double *red);
// red[1] = sum alpha_i * 0.5 f_i ; red[2] = sum lp_i   (GP_Utils.cpp:810, 1159)
void gpak_launch_nlz_terms(hipStream_t st, int N, const double *y, const double *f, const double *alpha,
                           double sn2, double *red);
void gpak_launch_scale(hipStream_t st, int n, const double *in, double s, double *out);
void gpak_launch_axpy(hipStream_t st, int n, double a, const double *x, double *y);  // y += a x

// ---- predict.hip ------------------------------------------------------------------------
// pool_sum / pool_M: column sums and count of the WHOLE test set when Xte is a slice of it, or nullptr
int gpak_predict_impl(gpak_ctx *ctx, const double *Xte, long M, double *mean, double *var, const double *pool_sum,
                      long pool_M);
int gpak_solve_chol_impl(gpak_ctx *ctx, double *X_host, int k);
// gpak_predict_block / gpak_block_cross on a single-GPU context whose factor and alpha are current
int gpak_predict_block_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, double *mean, double *var, int flags,
                            double *Kbar_host);
// gpak_predict_joint (Xi == nullptr: mean and, when asked, cov_host) / gpak_sample_joint (Xi set: Z and the mean) on a
// single-GPU context whose factor and alpha are current.  GPAK_ENOTPD: C + nugget I failed (mean valid, Z untouched).
int gpak_joint_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, double *mean, double *cov_host, int flags,
                    const double *Xi, int S, double nugget, double *Z);

// what gpak_design_impl shares with the joint calls: dWt / dC / dCinv / the point buffers for a stack of `cap` rows (a
// multiple of 256) and `points` discretisation points, sized and skewed as gpak_joint_impl sizes them (*ld = the leading
// dimension of dWt and dC); and the substitution dWt := dWt L^-T over those rows on the context's stream
int gpak_joint_reserve(gpak_ctx *ctx, int cap, size_t points, int nterms, long *ld);
void gpak_joint_forward_subst(gpak_ctx *ctx, int cap, long ldw);

// the block path's buffers for batches of `cap` blocks (a multiple of 256) and `points` discretisation points; want_wt: also
// the cross-kernel batch dWt, *ldw its leading dimension (skewed as gpak_predict_block_impl skews it)
int gpak_block_reserve(gpak_ctx *ctx, int cap, size_t points, int nterms, bool want_wt, long *ldw);
// the substitution of the prediction path on any test-major batch: Wt (rows x Np, rows a multiple of 128, leading dimension
// ldw) := Wt L^-T on the context's stream
void gpak_forward_subst_rows(gpak_ctx *ctx, double *Wt, long ldw, int rows);

// ---- condition.hip ----------------------------------------------------------------------
// the spectral prior of gpak_sample_path as api.hip has checked it (host pointers)
struct GpakPathPrior {
  int nfeat;
  const int *feat_term;
  const double *omega, *ab, *b0, *E;
};
// gpak_condition (prior == nullptr: Ysim and Fsim are the caller's) / gpak_sample_path (prior set: Ysim and Fsim are
// ignored) on a single-GPU context whose factor and alpha are current and whose arguments api.hip has checked
int gpak_condition_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, const double *Ysim, const double *Fsim, int S, double *Z,
                        double *mean, int flags, gpak_condition_summary *summary, const GpakPathPrior *prior);
// Z (nB x S, ldz) = F0 (its first nF columns; null: zeros) + Kbar A by the fused kernel: P the blocks' points point-major
// (gpak_transform_blocks_f64), Q the transformed samples, Np = Q.n rounded up to 128 (it fixes the slabs), scratch
// gpak_kmm_slabs(Np) * nB * S doubles
int gpak_kmm_slab_len(int Np);
int gpak_kmm_slabs(int Np);
void gpak_launch_kmm(hipStream_t st, const double *P, int cap, int nB, int nd, const DevPoints &Q, int Np, const KernParams &kp,
                     const double *A, long lda, int S, const double *F0, long ldf, int nF, double *Z, long ldz, double *scratch);

// ---- design.hip -------------------------------------------------------------------------
// gpak_design on a single-GPU context whose factor and alpha are current and whose arguments api.hip has checked: perm =
// the candidate points sorted by (hole, point), offs = where each hole starts in it (H + 1 entries)
int gpak_design_impl(gpak_ctx *ctx, const double *Xt, long T, int nd, const double *Xc, long Mc, const int *perm,
                     const int *offs, int H, const double *wt, int k, double *gain, double *reduction, double *var,
                     int *picked, double *pick_gain, double *var_after, gpak_design_summary *summary);

// ---- the distributed factor as one rank holds it (dist.hip), handed to a single-GPU context of the SAME device
// (multi.hip: group prediction and solve_chol reuse the factor instead of factoring a replica again) ----
struct gpak_dist;
struct gpak_dist_factor_view {
  int N, Np, nb, nJ;
  const double *const *panels;   // per block column: packed W x (Np - J), leading dimension Np - J, rows from the diagonal block down
  const double *const *invs;     // per block column: W/128 x 2 x 128 x 128 inverted diagonal blocks (inverse, inverse transposed)
  const double *alpha, *f;       // Np each (device)
  double quad, sumlp, logdet, nlz;
};
int gpak_dist_factor_view_get(gpak_dist *h, gpak_dist_factor_view *out);
double gpak_dist_grad_ms(const gpak_dist *h);
int gpak_import_factor(gpak_ctx *ctx, const gpak_dist_factor_view *v);

// ---- api.hip ----------------------------------------------------------------------------
// sigInv = Rot * lambda * Rot^T of the eight ExpAns parameters (Kernel.cpp:1399-1425), column-major 3 x 3
void gpak_build_siginv(const double *e, double *A);
// HybKerns composition -> KernParams (mu and d are the caller's)
int gpak_build_kp(int nterms, const int *kinds, const double *pars, double bias, double white, int dist_mode,
                  KernParams *out, double *kdiag_out);

// ---- grad.hip ---------------------------------------------------------------------------
// gpak_grad / gpak_grad_hyb and gpak_grad_exact on a single-GPU context whose factor and alpha are current
int gpak_grad_impl(gpak_ctx *ctx, double *g, int ng);
int gpak_grad_exact_impl(gpak_ctx *ctx, double *g, int ng);
// gpak_loo on a single-GPU context whose factor and alpha are current; mean, var, summary may each be null
int gpak_loo_impl(gpak_ctx *ctx, double *mean, double *var, gpak_loo_summary *summary);
// gpak_loo_grad on a single-GPU context whose factor and alpha are current; summary may be null
int gpak_loo_grad_impl(gpak_ctx *ctx, double *g, int ng, gpak_loo_summary *summary);
// its refusals, from the composition alone: GPAK_EINVAL for a wrong ng, GPAK_ENOTIMPL for a White child or a second ExpAns child
int gpak_loo_grad_layout(gpak_ctx *ctx, int ng);
// gpak_cv_groups_grad on a single-GPU context whose factor and alpha are current and whose labels api.hip has checked (perm
// and offs as for gpak_cv_groups_impl); summary may be null.  Its refusals from the composition alone: the layout call
int gpak_cv_groups_grad_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *g, int ng,
                             gpak_cv_groups_summary *summary);
int gpak_cv_groups_grad_layout(gpak_ctx *ctx, int ng);
// gpak_cv_folds_grad on a single-GPU context whose factor and alpha are current and whose labels api.hip has checked
int gpak_cv_folds_grad_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *g, int ng,
                            gpak_cv_groups_summary *summary, int flags);
int gpak_cv_folds_grad_layout(gpak_ctx *ctx, int ng);
// Rot (Kernel.cpp:1399-1410) of the ExpAns parameters e; D (optional): D[a] = dRot / d angle_a
void gpak_rot_tables(const double *e, double R[3][3], double (*D)[3][3]);
void gpak_grad_assemble(const KernParams &kp, const int *kinds, const double *expans, int d, int N, double sn2,
                        const double *red, double *g);
// at least `elems` doubles in ctx->dGpart (contents are not kept); G = L^-T of the current factor as one Np x Np matrix
// (leading dimension ldg) on the context's stream
int gpak_grad_scratch(gpak_ctx *ctx, size_t elems);
// room for `elems` doubles of L^-T in ctx->dLoo (gpak_loo, gpak_cv_groups); false: it does not fit (the HIP error is cleared)
bool gpak_loo_workspace(gpak_ctx *ctx, size_t elems);
void gpak_grad_g_full(gpak_ctx *ctx, double *G, long ldg);
// the same driver on any lower factor held as one matrix: T = R^-T (n x n, n a multiple of 128, leading dimension ldt)
// of the factor R at M (leading dimension ld) whose inverted 128-blocks (gpak_factor_panel's) are at inv
void gpak_grad_g_of(hipStream_t st, int n, const double *M, long ld, const double *inv, double *T, long ldt);

// ---- cv_groups.hip ----------------------------------------------------------------------
// gpak_cv_groups on a single-GPU context whose factor and alpha are current and whose labels api.hip has checked: perm =
// the samples sorted by (group, sample), offs = where each group starts in it (n_groups + 1 entries)
int gpak_cv_groups_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *mean, double *var,
                        double *group_logp, gpak_cv_groups_summary *summary);
// its two batched passes on device lists, on the context's stream: S of every group (gpak_cvg_s_elems(size) doubles each,
// at Sbuf + soff[g]), then the group's outputs from its S; every group has at most GPAK_CV_GROUP_MAX samples
long long gpak_cvg_s_elems(int s);
void gpak_cvg_launch_gram(gpak_ctx *ctx, const double *G, long ld, int n_groups, const int *dperm, const int *doffs,
                          const long long *dsoff, double *dS);
void gpak_cvg_launch_solve(gpak_ctx *ctx, int n_groups, int max_size, const double *dS, const long long *dsoff,
                           const int *dperm, const int *doffs, double *dmean, double *dvar, double *dlogp, double *dgsum,
                           int *dinfo);
// the solve pass of gpak_cv_groups_grad: the same outputs, the same bytes, and the weights of the gradient -- e_I scattered
// into dE (Np doubles, zeroed by the caller) and Q_I (Q_I Q_I^T = sn2 S^-1 + e_I e_I^T) row-major with pitch
// GPAK_CV_GROUP_MAX at dQb + dqoff[g]
void gpak_cvg_launch_solve_weights(gpak_ctx *ctx, int n_groups, int max_size, const double *dS, const long long *dsoff,
                                   const int *dperm, const int *doffs, double *dmean, double *dvar, double *dlogp,
                                   double *dgsum, int *dinfo, double *dE, double *dQb, const long long *dqoff);
// the column mix: H[:, dperm[dbstart[b] .. dbstart[b + 1])] times bin b's 128 x 128 row-major matrix at dQb + b * 128^2, in
// place, for every 128-row tile of the Np rows and every bin
void gpak_cvg_launch_mix(gpak_ctx *ctx, double *H, long ld, int n_bins, const int *dperm, const int *dbstart, const double *dQb);
// greedy bins of at most GPAK_CV_GROUP_MAX columns over consecutive groups: first[b] = first group of bin b,
// first[n_bins] = n_groups; returns n_bins
extern "C" int gpak_cvg_pack_bins(const int *sizes, int n_groups, int *first);

// ---- cv_folds.hip -----------------------------------------------------------------------
// P[r, c] = G[rows[r], k0 + c] (r < m; zero rows up to m_p = m rounded up to 128), c < Np - k0: gpak_cvf_pack_f64
void gpak_launch_pack_rows(hipStream_t st, const double *G, long ld, int Np, const int *rows, int m, int k0, double *P,
                           long ldp);
// gpak_cv_folds on a single-GPU context whose factor and alpha are current and whose labels api.hip has checked (perm and
// offs as for gpak_cv_groups_impl)
int gpak_cv_folds_impl(gpak_ctx *ctx, const int *perm, const int *offs, int n_groups, double *mean, double *var,
                       double *group_logp, gpak_cv_groups_summary *summary, int flags);
// what it shares with gpak_cv_folds_grad_impl (grad.hip).  The two kinds of groups of a labelling: the groups of at most
// GPAK_CV_GROUP_MAX samples (unless !batch) as compacted lists for the batched kernels -- sperm / soffs as perm / offs, soff
// the offsets of their S -- and the others, in ascending group number, with what their workspaces must hold
struct gpak_cvf_plan {
  int n_groups = 0, max_size = 0, max_small = 0, mp_max = 0;
  size_t nP = 0, nQ = 0;                 // doubles of the largest P; of the Q of all one-at-a-time groups
  std::vector<int> small_id, large_id, sperm, soffs;
  std::vector<long long> soff;
  std::vector<size_t> qoff;              // where one-at-a-time group k's Q (m_p x m_p, leading dimension m_p) starts in dCvfQ
};
void gpak_cvf_make_plan(const int *perm, const int *offs, int n_groups, int Np, bool batch, gpak_cvf_plan &pl);
// the workspaces of the one-at-a-time groups and their timing events; grad: also dCvfQ, two scalars behind the vectors and
// room for the Np x mp_max result of the column mix in dCvfP (and as much again for its gathered operand when it goes by GEMM).  GPAK_ENOMEM names the one that did not fit, as `who`
int gpak_cvf_reserve(gpak_ctx *ctx, const char *who, const gpak_cvf_plan &pl, bool grad);
// one-at-a-time group k on the context's stream: pack, product, factor, inverse, w, e, var and the group's sums (dlogp one
// double, dgsum three, info one int); dE set (an Np-vector): e_I scattered into it and the group's Q written to dCvfQ
int gpak_cvf_run_group(gpak_ctx *ctx, const gpak_cvf_plan &pl, size_t k, const int *perm, const int *offs, const double *G,
                       const int *dperm, int *info, double *dmean, double *dvar, double *dlogp, double *dgsum, double *dE);
// group_logp and the summary in the caller's numbering from hsum (logp and the three sums of the small groups, then of the
// others) and GPAK_ENOTPD naming the smallest failed group from hinfo ([0] the batched groups, [1 + k] group k)
int gpak_cvf_finish(gpak_ctx *ctx, const char *who, const gpak_cvf_plan &pl, const double *hsum, const int *hinfo, double ms,
                    double *group_logp, gpak_cv_groups_summary *summary);
// the column mix of one-at-a-time group k (cols: its m device column indices) on ctx->dG, through dCvfP: the fused kernel
// or gather + GEMM + scatter, by the group's width; dCvfQ holds its Q as gpak_cvf_run_group wrote it for that choice
void gpak_cvf_mix_group(gpak_ctx *ctx, const gpak_cvf_plan &pl, size_t k, const int *cols, int m);
// H[:, cols] <- H[:, cols] Q through the workspace Z (gpak_dev_mix_cols, include/gpak_dev_cv_mix.h)
void gpak_launch_mix_cols(hipStream_t st, double *H, long ld, int Np, const int *cols, int m, const double *Q, long ldq,
                          double *Z, long ldz);
