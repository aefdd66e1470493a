/* gpak_condition.h -- conditional simulation at any node count by conditioning an unconditional draw on the data with one
 * kriging step (Matheron's rule; "pathwise conditioning"), and the spectral prior sampler that supplies such draws on the
 * device.  Part of the context-level C-ABI, with the conventions of gpak.h (extern "C", status codes, host pointers,
 * column-major); gpak.h does NOT include it: include this header for the calls. */
#ifndef GPAK_CONDITION_H
#define GPAK_CONDITION_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags: the comparison path -- the averaged fill into the batch buffer and the GEMM against A -- instead of the fused kernel */
#define GPAK_COND_UNFUSED 1

/* device ms of the S solves with the training factor, of the prior (0 for gpak_condition) and of the product K-bar A (with
 * the fills of the comparison path); batches = node batches streamed; fused = 1 when the fused kernel ran, 0 for the
 * comparison path */
typedef struct { double solve_ms, prior_ms, product_ms; int batches, fused; } gpak_condition_summary;

/* Nodes: M blocks of nd discretisation points each, Xd (M * nd) x d in the layout of gpak_predict_block (nd = 1: points).
 * (Fsim[:, s], Ysim[:, s]) is an unconditional draw of the M node averages and of the N noisy observations; with
 *   Ky = K + white I + sn2 I,  alpha = Ky^-1 y,  A = alpha 1^T - Ky^-1 Ysim   (N x S),
 *   Z = Fsim + K-bar A,   K-bar[b, j] = (1/nd) sum_a k(x_{b,a}, x_j)  (the averaged cross-kernel of gpak_block_cross)
 * column s of Z is a draw from the posterior of the node averages whenever (Fsim, Ysim)[:, s] is a draw of the prior: the
 * map is exact and linear.  mean = K-bar alpha comes from the same pass as one more column of A.  Fsim NULL: zeros.
 *
 * No M x M matrix exists.  The nodes stream in batches of GPAK_OPT_PRED_BATCH under the block path's 1 GiB point budget;
 * Z and mean are the same bytes whatever the batch size, and two calls return the same bytes: the order of every sum
 * depends on the element alone.  Everything is fp64, also in a GPAK_F32 context; every composition is accepted; for
 * GPAK_DIST_EXPANSION the pooled mean is taken over the training set and all M * nd points, as gpak_predict_block takes it.
 * Runs gram / factor / alpha if they are stale, only reads them, and sets predict_ms.
 * GPAK_EINVAL: a NULL ctx, Xd, Ysim or Z; M, nd or S <= 0; d other than the training set's; flags with bits other than
 * GPAK_COND_UNFUSED.  GPAK_ESTATE without a training set or parameters, GPAK_ENOTIMPL for a multi-GPU context, GPAK_ENOMEM.
 * GPAK_ENOTPD from the training factor: Z and mean are quiet NaN. */
int gpak_condition(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, const double *Ysim /* N x S */,
                   const double *Fsim /* M x S, may be NULL */, int S, double *Z /* M x S */, double *mean /* M, may be NULL */,
                   int flags, gpak_condition_summary *summary /* may be NULL */);

/* The full sampler: a spectral (random Fourier feature) draw of the prior evaluated on the device at the training points
 * and at the nodes, then gpak_condition's sequence; the prior at the nodes never leaves the device.
 * Feature f < nfeat belongs to stationary term feat_term[f] of the composition in force; its frequency omega[4 f .. 4 f + 3]
 * is in that term's TRANSFORMED coordinates u_t(x) = (x - mu) A_t (mu: the pooled mean, the same for both evaluations);
 * omega[4 f + 3] multiplies the transformed 4th column and is ignored for 3-column inputs.  With F_t the number of
 * features of term t, theta_f(x) = omega_f . u_t(x) and c the constant the fill adds to every entry (Kern_Bias):
 *   f_s(x) = sum_f sqrt(var2_t / F_t) (ab[2 f, s] cos theta_f(x) + ab[2 f + 1, s] sin theta_f(x)) + sqrt(c) b0[s]
 *   Fsim[b, s] = (1/nd) sum_a f_s(x_{b,a}),   Ysim[j, s] = f_s(x_j) + sqrt(sn2 + white) E[j, s]
 * ab is (2 nfeat) x S, b0 has S entries (NULL where c == 0), E is N x S: unit normals for a draw.  The result is a
 * deterministic function of the inputs: the library draws no random numbers, and which frequencies make f_s a draw of the
 * prior is the caller's business (host/sim_spectral.hpp: the covariance of f_s is then the prior's to O(1/sqrt(F_t)), the
 * conditioning on the data exact).  A White child gives the nodes no nugget of their own here.
 * Statuses as gpak_condition, and GPAK_EINVAL for nfeat <= 0, a NULL feat_term, omega, ab or E, b0 NULL with c != 0, a
 * feat_term outside the composition's terms. */
int gpak_sample_path(gpak_ctx *ctx, const double *Xd, long M, int nd, int d, int nfeat, const int *feat_term,
                     const double *omega /* 4 x nfeat */, const double *ab /* (2 nfeat) x S */, const double *b0 /* S */,
                     const double *E /* N x S */, int S, double *Z /* M x S */, double *mean /* M, may be NULL */, int flags,
                     gpak_condition_summary *summary /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_CONDITION_H */
