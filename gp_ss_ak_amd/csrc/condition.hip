// condition.hip -- conditioning by kriging (gpak_condition) and the spectral prior sampler (gpak_sample_path) for gfx950.
//
//   Z = Fsim + Kbar A,   A = alpha 1^T - (K + white I + sn2 I)^-1 Ysim,   mean = Kbar alpha (one more column of A)
// streamed over node batches like the block path; no M x M matrix exists.  The hot path is "averaged cross-kernel times an
// N x S matrix": gpak_kmm_f64 evaluates Kbar in the A-fragment layout of v_mfma_f64_16x16x4 and never stores it.  The
// comparison path (GPAK_COND_UNFUSED) is the averaged fill into dWt and gpak_launch_gemm_nt against A^T.
#include <algorithm>
#include <cmath>
#include <vector>

#include "gpak_internal.h"

#define PARR GPAK_PARR
#define PB 128

typedef double kmm_d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// The fused product.  One workgroup = 64 nodes (16 per wave) x up to 128 realisations x one slab of samples.
// Per chunk of 32 samples: all four waves stage A[chunk, s0 .. s0 + 128) and the chunk's transformed coordinates in LDS;
// lane (l15, l4) of a wave then evaluates kbar(node l15, sample 4 ks + l4) for the 8 k-steps of the chunk -- the loop over
// the node's nd points outermost, so a point's coordinates are loaded once per chunk; per element the nd values are added
// in ascending a (terms innermost) and the sum is scaled once by 1/nd before the bias is added: the arithmetic of
// gpak_fillblk_f64 -- and hands each value to the MFMA as its A operand for every 16-column tile of realisations: from
// the vector unit to the matrix unit without passing through LDS or HBM.
// LDS image of A: [realisation][sample] with a pitch of 34 doubles.  Staging writes run along the samples (32
// consecutive doubles: conflict-free); a B-fragment read has l15 along the realisations and l4 along the samples, dword
// address 68 s + 2 k: the 32 lanes of a half-wave (16 s x 2 k) fall on 32 distinct bank pairs.
// Every element of a slab's partial is ONE MFMA chain over the slab's samples in ascending order; which samples a slab
// holds depends on N_p alone (gpak_kmm_slab_len).  No atomics.
// ---------------------------------------------------------------------------------------
#define KMM_ROWS 64
#define KMM_SC 128
#define KMM_KC 32
#define KMM_KP 34
__global__ __launch_bounds__(256) void gpak_kmm_f64(const double *__restrict__ P, int cap, int nB, int nd,
                                                     const double *__restrict__ Q, int capQ, int nQ, KernParams kp,
                                                     double inv_nd, const double *__restrict__ A, long lda, int S, int slab_len,
                                                     double *__restrict__ part, size_t part_slab, long ldp) {
  __shared__ double sB[KMM_SC * KMM_KP];
  __shared__ double sQ[GPAK_MAX_TERMS][GPAK_PT][KMM_KC];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int s0 = blockIdx.y * KMM_SC, ns = min(KMM_SC, S - s0), nct = (ns + 15) / 16;
  const int j_lo = blockIdx.z * slab_len, j_hi = min(nQ, j_lo + slab_len);
  const int r = min((int)blockIdx.x * KMM_ROWS + w * 16 + l15, nB - 1);   // rows past the last node repeat it and are not stored
  const size_t capP = (size_t)nd * cap;
  const int nterms = kp.nterms;
  kmm_d4 acc[KMM_SC / 16];
#pragma unroll
  for (int ct = 0; ct < KMM_SC / 16; ct++) acc[ct] = (kmm_d4){0.0, 0.0, 0.0, 0.0};
  for (int j0 = j_lo; j0 < j_hi; j0 += KMM_KC) {
    __syncthreads();   // the previous chunk has been read
    {
      const int k = t & (KMM_KC - 1), j = j0 + k;
#pragma unroll 4
      for (int i = 0; i < KMM_SC / 8; i++) {
        const int s = (t >> 5) + 8 * i;
        sB[s * KMM_KP + k] = (j < j_hi && s < ns) ? A[j + (size_t)(s0 + s) * lda] : 0.0;
      }
      for (int idx = t; idx < nterms * GPAK_PT * KMM_KC; idx += 256) {
        const int m = idx / (GPAK_PT * KMM_KC), c = (idx / KMM_KC) % GPAK_PT, kk = idx & (KMM_KC - 1);
        sQ[m][c][kk] = (j0 + kk < j_hi) ? PARR(Q, capQ, m, c)[j0 + kk] : 0.0;   // a sample past the slab: any finite point, its A is 0
      }
    }
    __syncthreads();
    double kb[KMM_KC / 4];
#pragma unroll
    for (int ks = 0; ks < KMM_KC / 4; ks++) kb[ks] = 0.0;
    for (int a = 0; a < nd; a++) {
      const size_t o = (size_t)a * cap + r;
      for (int m = 0; m < nterms; m++) {
        double p[GPAK_PT];
#pragma unroll
        for (int c = 0; c < GPAK_PT; c++) p[c] = PARR(P, capP, m, c)[o];
#pragma unroll
        for (int ks = 0; ks < KMM_KC / 4; ks++) {
          const int kk = 4 * ks + l4;
          kb[ks] += gpak_profile(gpak_d2(p[0], p[1], p[2], p[3], p[4], sQ[m][0][kk], sQ[m][1][kk], sQ[m][2][kk], sQ[m][3][kk],
                                         sQ[m][4][kk], kp.mode), kp.term[m]);
        }
      }
    }
    const double *bl = sB + l15 * KMM_KP + l4;
#pragma unroll
    for (int ks = 0; ks < KMM_KC / 4; ks++) {
      const double v = fma(inv_nd, kb[ks], kp.bias);
#pragma unroll
      for (int ct = 0; ct < KMM_SC / 16; ct++)
        if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, bl[ct * 16 * KMM_KP + 4 * ks], acc[ct], 0, 0, 0);
    }
  }
  // the lane holds rows l4 + 4 q (q = 0..3) of its wave's 16 nodes, column ct * 16 + l15
  double *out = part + (size_t)blockIdx.z * part_slab;
  const int row0 = blockIdx.x * KMM_ROWS + w * 16 + l4;
#pragma unroll
  for (int ct = 0; ct < KMM_SC / 16; ct++) {
    const int s = s0 + ct * 16 + l15;
    if (ct < nct && s < S) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (row0 + 4 * q < nB) out[(row0 + 4 * q) + (size_t)s * ldp] = acc[ct][q];
    }
  }
}

// Z[i, s] = f0s * F0[i, s] (s < nF) + (sum of the nz partials in ascending order + colc[s]); F0 and colc may be null
__global__ __launch_bounds__(256) void gpak_cond_sum_f64(const double *__restrict__ part, size_t part_slab, long ldp, int nz,
                                                          int rows, const double *__restrict__ F0, long ldf, int nF, double f0s,
                                                          const double *__restrict__ colc, double *__restrict__ Z, long ldz) {
  const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= rows) return;
  const double *p = part + i + (size_t)s * ldp;
  double sum = p[0];
  for (int z = 1; z < nz; z++) sum += p[(size_t)z * part_slab];
  if (colc) sum += colc[s];
  Z[i + (size_t)s * ldz] = (F0 && s < nF) ? f0s * F0[i + (size_t)s * ldf] + sum : sum;
}

// column s of A = alpha - x (x == null: alpha), zero from row N on; At set: the same numbers realisation-major (ldt)
__global__ __launch_bounds__(256) void gpak_cond_acol_f64(const double *__restrict__ alpha, const double *__restrict__ x, int N,
                                                           int Np, double *__restrict__ Acol, double *__restrict__ At, long ldt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Np) return;
  const double v = j < N ? (x ? alpha[j] - x[j] : alpha[j]) : 0.0;
  Acol[j] = v;
  if (At) At[(size_t)j * ldt] = v;
}

// Yt[s, j] = Y[j, s] * scale (s < S, j < N), zero elsewhere in the S_p x N_p batch: Ysim realisation-major, as the batched
// forward substitution of the prediction path takes its right-hand sides
__global__ __launch_bounds__(256) void gpak_cond_yt_f64(const double *__restrict__ Y, int N, int Np, int S, int Sp, double scale,
                                                         double *__restrict__ Yt, long ldw) {
  const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (j >= Np) return;
  Yt[s + (size_t)j * ldw] = (j < N && s < S) ? Y[j + (size_t)s * Np] * scale : 0.0;
}
// v[j] = Yt[s, j]: row s of the substituted batch as the right-hand side of one back substitution
__global__ __launch_bounds__(256) void gpak_cond_row_f64(const double *__restrict__ Yt, long ldw, int Np, double *__restrict__ v) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < Np) v[j] = Yt[(size_t)j * ldw];
}

// The spectral features of a batch of blocks (or of nB points, nd = 1), block-averaged: for feature f0 + g, g < nf,
//   Phi[r, 2 g] = (1/nd) sum_a cos theta,  Phi[r, 2 g + 1] = (1/nd) sum_a sin theta,  theta = omega . u_t(x_{r,a}),
// a ascending; rows from nB on and features from nf on (up to nf_pad) are zeros.  One thread per row and four features.
#define FEAT_PER 4
__global__ __launch_bounds__(256) void gpak_featfill_f64(const double *__restrict__ P, int cap, int nB, int nd,
                                                          const int *__restrict__ fterm, const double *__restrict__ omega,
                                                          int f0, int nf, int d4, double inv_nd, double *__restrict__ Phi,
                                                          long ld, int rows_p) {
  const int r = blockIdx.x * 256 + threadIdx.x, g0 = blockIdx.y * FEAT_PER;
  if (r >= rows_p) return;
  const size_t capP = (size_t)nd * cap;
#pragma unroll
  for (int u = 0; u < FEAT_PER; u++) {
    const int g = g0 + u;
    double c = 0.0, s = 0.0;
    if (r < nB && g < nf) {
      const int f = f0 + g, m = fterm[f];
      const double w0 = omega[4 * (size_t)f], w1 = omega[4 * (size_t)f + 1], w2 = omega[4 * (size_t)f + 2],
                   w3 = d4 ? omega[4 * (size_t)f + 3] : 0.0;
      for (int a = 0; a < nd; a++) {
        const size_t o = (size_t)a * cap + r;
        const double th = fma(w3, PARR(P, capP, m, 4)[o],
                              fma(w2, PARR(P, capP, m, 2)[o], fma(w1, PARR(P, capP, m, 1)[o], w0 * PARR(P, capP, m, 0)[o])));
        double sv, cv;
        sincos(th, &sv, &cv);
        c += cv; s += sv;
      }
      c *= inv_nd; s *= inv_nd;
    }
    Phi[r + (size_t)(2 * g) * ld] = c;
    Phi[r + (size_t)(2 * g + 1) * ld] = s;
  }
}

// Sample slabs of the fused product: a function of N_p alone, so that an element's chain does not depend on the batch
int gpak_kmm_slab_len(int Np) { return std::max(512, (Np / 16 + PB - 1) / PB * PB); }
int gpak_kmm_slabs(int Np) { const int sl = gpak_kmm_slab_len(Np); return (Np + sl - 1) / sl; }

void gpak_launch_kmm(hipStream_t st, const double *P, int cap, int nB, int nd, const DevPoints &Q, int Np, const KernParams &kp,
                     const double *A, long lda, int S, const double *F0, long ldf, int nF, double *Z, long ldz, double *scratch) {
  const int sl = gpak_kmm_slab_len(Np), nz = gpak_kmm_slabs(Np);
  const size_t part_slab = (size_t)nB * S;
  hipLaunchKernelGGL(gpak_kmm_f64, dim3((nB + KMM_ROWS - 1) / KMM_ROWS, (S + KMM_SC - 1) / KMM_SC, nz), dim3(256), 0, st, P, cap,
                     nB, nd, Q.base, Q.cap, Q.n, kp, 1.0 / nd, A, lda, S, sl, scratch, part_slab, (long)nB);
  hipLaunchKernelGGL(gpak_cond_sum_f64, dim3((nB + 255) / 256, S), dim3(256), 0, st, scratch, part_slab, (long)nB, nz, nB, F0, ldf,
                     nF, 1.0, (const double *)nullptr, Z, ldz);
}

// ---------------------------------------------------------------------------------------
// The calls.  Which path runs by default: the fused kernel, for every nd, S and composition.  Measured at N = 32768,
// S = 100 (profiles/path.txt): 65536 points 15.6 ms fused against 17.3 ms for fill + GEMM; 16384 blocks of
// 2 x 2 x 2 10.1 against 8.7 ms, where the comparison path's fill is the table-exp gpak_fillblk1_f64 of the default
// composition (29 fp64 instructions per evaluation against the 47 evaluated here).  That loss is 1.4 ms of a 122 ms call
// whose solves take 111 ms, and the fused path needs no N_p-wide batch buffer; two sizes make no rule in nd, so there is none.
// ---------------------------------------------------------------------------------------
#define FEAT_CHUNK 1024   // features per product of the spectral prior: 2048 columns of Phi

namespace {
struct Timer {   // device ms between two points of the context's stream, added up over the batches
  hipEvent_t a = nullptr, b = nullptr;
  double ms = 0.0;
  bool ok() { return (a || hipEventCreate(&a) == hipSuccess) && (b || hipEventCreate(&b) == hipSuccess); }
  void start(hipStream_t st) { hipEventRecord(a, st); }
  void stop(hipStream_t st) { hipEventRecord(b, st); }
  void collect() { float v = 0; if (hipEventElapsedTime(&v, a, b) == hipSuccess) ms += v; }
  ~Timer() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};
}  // namespace

// f_s at `rows` points or blocks (P, cap, nB, nd): the feature products chunk by chunk into dCondPart, then
// out[i, s] = f0s * F0[i, s] + (sum of the chunks in ascending order + colc[s]), s < S
static void prior_values(gpak_ctx *ctx, const GpakPathPrior &pr, const double *P, int cap, int nB, int nd, int rows_p, int S, int Sp,
                         const double *F0, long ldf, double f0s, double *out, long ldo, int out_rows) {
  hipStream_t st = ctx->stream;
  const int nchunk = (pr.nfeat + FEAT_CHUNK - 1) / FEAT_CHUNK;
  const size_t part_slab = (size_t)rows_p * Sp;
  for (int ch = 0; ch < nchunk; ch++) {
    const int f0 = ch * FEAT_CHUNK, nf = std::min(FEAT_CHUNK, pr.nfeat - f0);
    const int nfp = (nf + 63) / 64 * 64;   // 2 nfp columns: a multiple of 128, the product's K
    hipLaunchKernelGGL(gpak_featfill_f64, dim3((rows_p + 255) / 256, nfp / FEAT_PER), dim3(256), 0, st, P, cap, nB, nd, ctx->dCondFt.p,
                       ctx->dCondOm.p, f0, nf, ctx->d == 4 ? 1 : 0, 1.0 / nd, ctx->dCondPhi.p, (long)rows_p, rows_p);
    // beta = 0 and alpha = 1: the tile is the accumulator chain itself, whichever of the GEMM's kernels the grid selects
    gpak_launch_gemm_nt(st, rows_p / PB, Sp / PB, 2 * nfp, 1.0, ctx->dCondPhi, rows_p, ctx->dCondW + (size_t)2 * f0 * Sp, Sp, 0.0,
                        ctx->dCondPart + (size_t)ch * part_slab, rows_p, 0, 0, false, false);
  }
  hipLaunchKernelGGL(gpak_cond_sum_f64, dim3((out_rows + 255) / 256, S), dim3(256), 0, st, ctx->dCondPart.p, part_slab, (long)rows_p,
                     nchunk, out_rows, F0, ldf, S, f0s, pr.b0 ? ctx->dCondB0.p : (const double *)nullptr, out, ldo);
}

int gpak_condition_impl(gpak_ctx *ctx, const double *Xd, long M, int nd, const double *Ysim, const double *Fsim, int S, double *Z,
                        double *mean, int flags, gpak_condition_summary *summary, const GpakPathPrior *prior) {
  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ctx->N, Np = ctx->Np, d = ctx->d;
  const bool unfused = flags & GPAK_COND_UNFUSED;
  KernParams kp = ctx->kp;
  kp.d = d;
  // the block path's batch: GPAK_OPT_PRED_BATCH, the cross-kernel batch under 8 GiB, the points under 1 GiB
  int batch = 16384;
  if (ctx->sched.pred_batch > 0) batch = std::max(2 * PB, ctx->sched.pred_batch / (2 * PB) * (2 * PB));
  while (batch > 2 * PB && (size_t)batch * Np * sizeof(double) > ((size_t)8 << 30)) batch /= 2;
  const size_t per_block = sizeof(double) * (size_t)nd * (4 + GPAK_PT * (size_t)kp.nterms);
  while (batch > 2 * PB && (size_t)batch * per_block > ((size_t)1 << 30)) batch /= 2;
  batch = batch / (2 * PB) * (2 * PB);
  const long Mp = (M + 2 * PB - 1) / (2 * PB) * (2 * PB);
  const int cap = (int)std::min<long>(Mp, batch);
  if ((size_t)cap * nd > ((size_t)1 << 30)) { ctx->err = "too many discretisation points per block"; return GPAK_EINVAL; }
  const int SA = S + 1;                              // the columns of A: the realisations and alpha
  const int Sp = (S + PB - 1) / PB * PB, SAp = (SA + PB - 1) / PB * PB;
  const int nz = gpak_kmm_slabs(Np);
  const int Syt = (S + 2 * PB - 1) / (2 * PB) * (2 * PB);   // the rows of the realisation-major batch of right-hand sides
  const long ldyt = Syt + 32;                               // skewed off the power of two, as dWt is
  const int nchunk = prior ? (prior->nfeat + FEAT_CHUNK - 1) / FEAT_CHUNK : 0;
  long ldw = 0;
  int rc = gpak_block_reserve(ctx, cap, (size_t)cap * nd, kp.nterms, unfused, &ldw);
  if (rc) return rc;
  {
    const int rows_max = std::max(cap, Np);
    size_t part = unfused ? (size_t)cap * SAp : (size_t)nz * cap * SA;
    if (prior) part = std::max(part, (size_t)nchunk * rows_max * Sp);
    bool ok = ctx->dCondA.reserve((size_t)Np * SA) && ctx->dCondY.reserve((size_t)Np * S) && ctx->dCondYt.reserve((size_t)ldyt * Np) && ctx->dCondZ.reserve((size_t)cap * SA) &&
              ctx->dCondPart.reserve(part) && (!(Fsim || prior) || ctx->dCondF.reserve((size_t)cap * S)) &&
              (!unfused || ctx->dCondAt.reserve((size_t)SAp * Np));
    if (ok && prior) {
      const size_t wcols = (size_t)2 * nchunk * FEAT_CHUNK;   // every chunk may read a full padded one
      ok = ctx->dCondPhi.reserve((size_t)rows_max * 2 * FEAT_CHUNK) && ctx->dCondW.reserve(wcols * Sp) &&
           ctx->dCondOm.reserve(4 * (size_t)prior->nfeat) && ctx->dCondFt.reserve(prior->nfeat) && ctx->dCondB0.reserve(S);
    }
    if (!ok) {
      (void)hipGetLastError();
      ctx->err = "device allocation failed for the realisations' buffers (A, Ysim, Z, the slab partials)";
      return GPAK_ENOMEM;
    }
  }
  Timer t_all, t_solve, t_prior, t_prod;
  if (!t_all.ok() || !t_solve.ok() || !t_prior.ok() || !t_prod.ok()) { ctx->err = "hipEventCreate failed"; return GPAK_EHIP; }
  t_all.start(st);

  // pooled mean over the training set and all M * nd points, as gpak_predict_block
  const long Mn = M * nd;
  double s2[4] = {0, 0, 0, 0};
  for (int k = 0; k < d; k++)
    for (long i = 0; i < Mn; i++) s2[k] += Xd[i + (size_t)k * Mn];
  gpak_pooled_mean(ctx->xsum, N, s2, Mn, kp.mu);
  gpak_launch_transform(st, ctx->dX, Np, N, kp, ctx->Upred);
  kp.white = 0.0;   // Kern_White contributes nothing to a train x node block

  // Ysim on the device, N_p x S with zero padding rows
  if (prior) {
    const GpakPathPrior &pr = *prior;
    // W^T (S_p x 2 nfeat_pad, zero padded): W[2 f, s] = amp_f ab[2 f, s]; the chunks are FEAT_CHUNK features apart
    const size_t wcols = (size_t)2 * nchunk * FEAT_CHUNK;
    std::vector<double> hW(wcols * Sp, 0.0);
    std::vector<int> count(GPAK_MAX_TERMS, 0);
    for (int f = 0; f < pr.nfeat; f++) count[pr.feat_term[f]]++;
    for (int f = 0; f < pr.nfeat; f++) {
      const int tm = pr.feat_term[f];
      const double amp = std::sqrt(kp.term[tm].var2 / count[tm]);
      for (int s = 0; s < S; s++) {
        hW[s + (size_t)(2 * f) * Sp] = amp * pr.ab[2 * (size_t)f + (size_t)s * 2 * pr.nfeat];
        hW[s + (size_t)(2 * f + 1) * Sp] = amp * pr.ab[2 * (size_t)f + 1 + (size_t)s * 2 * pr.nfeat];
      }
    }
    std::vector<double> hb0(S, 0.0);
    const double sc = std::sqrt(kp.bias);
    for (int s = 0; pr.b0 && s < S; s++) hb0[s] = sc * pr.b0[s];
    t_prior.start(st);
    GPAK_HIP(hipMemcpyAsync(ctx->dCondW, hW.data(), sizeof(double) * hW.size(), hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(ctx->dCondOm, pr.omega, sizeof(double) * 4 * (size_t)pr.nfeat, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(ctx->dCondFt, pr.feat_term, sizeof(int) * (size_t)pr.nfeat, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipMemcpyAsync(ctx->dCondB0, hb0.data(), sizeof(double) * S, hipMemcpyHostToDevice, st));
    // E rides in A's buffer until the solves overwrite it column by column
    GPAK_HIP(hipMemsetAsync(ctx->dCondA, 0, sizeof(double) * (size_t)Np * S, st));
    GPAK_HIP(hipMemcpy2DAsync(ctx->dCondA, sizeof(double) * Np, pr.E, sizeof(double) * N, sizeof(double) * N, S, hipMemcpyHostToDevice, st));
    GPAK_HIP(hipStreamSynchronize(st));   // the host vectors above go out of scope
    // only the N sample rows of Ysim are written; the solves read no others (gpak_cond_yt_f64)
    prior_values(ctx, pr, ctx->Upred.base, ctx->Upred.cap, N, 1, Np, S, Sp, ctx->dCondA, Np, std::sqrt(ctx->sn2 + ctx->kp.white),
                 ctx->dCondY, Np, N);
    t_prior.stop(st);
    GPAK_HIP(hipStreamSynchronize(st));
    t_prior.collect();
  } else {
    GPAK_HIP(hipMemcpy2DAsync(ctx->dCondY, sizeof(double) * Np, Ysim, sizeof(double) * N, sizeof(double) * N, S, hipMemcpyHostToDevice, st));
  }

  // A = alpha 1^T - B^-1 (Ysim / sn2), B = I + (K + white I) / sn2 = L L^T.  Forwards: ALL columns at once, realisation-major,
  // by the blocked substitution of the prediction path (Yt := Yt L^-T, MFMA products); backwards: per column, the context's
  // back substitution (gpak_backsolve, as ensure_alpha runs it)
  t_solve.start(st);
  double *w1 = ctx->dWork + Np, *w2 = ctx->dWork + 2 * (size_t)Np;
  ctx->state.work_vectors_overwritten();
  if (unfused) GPAK_HIP(hipMemsetAsync(ctx->dCondAt, 0, sizeof(double) * (size_t)SAp * Np, st));
  hipLaunchKernelGGL(gpak_cond_yt_f64, dim3((Np + 255) / 256, Syt), dim3(256), 0, st, ctx->dCondY.p, N, Np, S, Syt, 1.0 / ctx->sn2,
                     ctx->dCondYt.p, ldyt);
  gpak_forward_subst_rows(ctx, ctx->dCondYt, ldyt, Syt);
  for (int s = 0; s < S; s++) {
    hipLaunchKernelGGL(gpak_cond_row_f64, dim3((Np + 255) / 256), dim3(256), 0, st, ctx->dCondYt + s, ldyt, Np, w1);
    gpak_backsolve(ctx, st, w1, w2, ctx->dWork + 3 * (size_t)Np);
    hipLaunchKernelGGL(gpak_cond_acol_f64, dim3((Np + 255) / 256), dim3(256), 0, st, ctx->dAlpha.p, w2, N, Np,
                       ctx->dCondA + (size_t)s * Np, unfused ? ctx->dCondAt + s : (double *)nullptr, (long)SAp);
  }
  hipLaunchKernelGGL(gpak_cond_acol_f64, dim3((Np + 255) / 256), dim3(256), 0, st, ctx->dAlpha.p, (const double *)nullptr, N, Np,
                     ctx->dCondA + (size_t)S * Np, unfused ? ctx->dCondAt + S : (double *)nullptr, (long)SAp);
  t_solve.stop(st);

  int batches = 0;
  for (long b0 = 0; b0 < M; b0 += cap, batches++) {
    const int mb = (int)std::min<long>(cap, M - b0);
    const int mbp = (mb + 2 * PB - 1) / (2 * PB) * (2 * PB);
    const long xs = (long)mb * nd;
    for (int k = 0; k < d; k++)
      GPAK_HIP(hipMemcpyAsync(ctx->dXblk + (size_t)k * xs, Xd + (size_t)k * Mn + (size_t)b0 * nd, sizeof(double) * xs,
                              hipMemcpyHostToDevice, st));
    gpak_launch_transform_blocks(st, ctx->dXblk, xs, mb, nd, cap, kp, ctx->dTblk);
    const double *F0 = nullptr;
    if (prior) {
      t_prior.start(st);
      prior_values(ctx, *prior, ctx->dTblk, cap, mb, nd, mbp, S, Sp, nullptr, 0, 1.0, ctx->dCondF, cap, mb);
      t_prior.stop(st);
      F0 = ctx->dCondF;
    } else if (Fsim) {
      GPAK_HIP(hipMemcpy2DAsync(ctx->dCondF, sizeof(double) * cap, Fsim + b0, sizeof(double) * M, sizeof(double) * mb, S,
                                hipMemcpyHostToDevice, st));
      F0 = ctx->dCondF;
    }
    t_prod.start(st);
    if (unfused) {
      gpak_launch_fill_blocks(st, ctx->dTblk, cap, mb, nd, ctx->Upred, mbp, Np, kp, ctx->dWt, ldw);
      // beta = 0 and alpha = 1: the tile is the accumulator chain itself, whichever of the GEMM's kernels the grid selects
      gpak_launch_gemm_nt(st, mbp / PB, SAp / PB, Np, 1.0, ctx->dWt, ldw, ctx->dCondAt, SAp, 0.0, ctx->dCondPart, cap, 0, 0, false, false);
      hipLaunchKernelGGL(gpak_cond_sum_f64, dim3((mb + 255) / 256, SA), dim3(256), 0, st, ctx->dCondPart.p, (size_t)0, (long)cap, 1, mb,
                         F0, (long)cap, S, 1.0, (const double *)nullptr, ctx->dCondZ.p, (long)cap);
    } else {
      gpak_launch_kmm(st, ctx->dTblk, cap, mb, nd, ctx->Upred, Np, kp, ctx->dCondA, Np, SA, F0, cap, S, ctx->dCondZ, cap, ctx->dCondPart);
    }
    t_prod.stop(st);
    GPAK_HIP(hipMemcpy2DAsync(Z + b0, sizeof(double) * M, ctx->dCondZ, sizeof(double) * cap, sizeof(double) * mb, S, hipMemcpyDeviceToHost, st));
    if (mean) GPAK_HIP(hipMemcpyAsync(mean + b0, ctx->dCondZ + (size_t)S * cap, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipStreamSynchronize(st));
    t_prod.collect();
    if (prior) t_prior.collect();
  }
  t_all.stop(st);
  GPAK_HIP(hipStreamSynchronize(st));
  t_all.collect();
  t_solve.collect();
  ctx->times.predict_ms = t_all.ms;
  if (summary) {
    summary->solve_ms = t_solve.ms;
    summary->product_ms = t_prod.ms;
    summary->prior_ms = t_prior.ms;
    summary->batches = batches;
    summary->fused = unfused ? 0 : 1;
  }
  return GPAK_OK;
}
