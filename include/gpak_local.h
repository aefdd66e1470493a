/* gpak_local.h -- moving-neighbourhood kriging: every node is estimated from its own k <= 128 nearest samples, so the
 * samples to krige from may be any number (train on a subsample, estimate from all the assays).  Part of the context-level
 * C-ABI, with the conventions of gpak.h (extern "C", status codes, host pointers, column-major); gpak.h does NOT include it:
 * include this header for the calls. */
#ifndef GPAK_LOCAL_H
#define GPAK_LOCAL_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPAK_LOCAL_MAX    128   /* neighbours per node */
#define GPAK_LOCAL_LATENT 1     /* var without the noise term's sn2 / nd, as GPAK_BLOCK_LATENT */

/* upload_ms: the samples' upload and transform; krige_ms: the node batches (uploads, transform, kernel, copies back), both
 * device time; nodes = M; empty: nodes with no neighbour; notpd: nodes whose K_II had a pivot that is not positive;
 * batches: launches of the kernel; max_used: the longest list */
typedef struct { double upload_ms, krige_ms; long nodes, empty, notpd; int batches, max_used; } gpak_local_summary;

/* G (4 x 4, column-major) with |(x - x') G|^2 = D2 of stationary term `term` of the composition in force: the term's
 * metric factor A_t in the leading 3 x 3 and the factor of the fourth input column at G[3 + 4 * 3]; the rest zeros.  Its
 * leading d x d part is what gpak_local_neighbours takes.  For a one-term model the k nearest samples in this metric are
 * the k most correlated ones.  GPAK_EINVAL: a NULL ctx or G, term outside the composition; GPAK_ESTATE without
 * parameters; GPAK_ENOTIMPL for a multi-GPU context. */
int gpak_local_metric(const gpak_ctx *ctx, int term, double *G /* 4 x 4, column-major */);

/* The k nearest samples of every centre, exactly (the lists of a full sort).  Host code only; no context, no device.
 * Xs: Ns x d samples, Xc: M x d centres, both column-major, d = 3 or 4; G: d x d column-major, or NULL for the identity.
 *   t(x)_j = sum_r x_r G[r + d j]          r ascending, every product and sum rounded on its own (NULL G: t(x) = x)
 *   dist2  = sum_j (t(x)_j - t(c)_j)^2     j ascending
 * nbr[q + k * b], q < used[b]: the samples of centre b by ascending dist2, then ascending index (ties and duplicated
 * samples have one answer); radius > 0 keeps only dist2 <= radius * radius; the remaining slots hold -1.  used may be NULL.
 * Runs on `threads` std::threads, <= 0: min(hardware concurrency, 16), and never more than 256; the lists do not depend on
 * the thread count.
 * GPAK_EINVAL, nothing written: a NULL Xs, Xc or nbr; d other than 3 or 4; k outside 1..GPAK_LOCAL_MAX; Ns or M < 1; Ns
 * above INT_MAX; a NaN radius; a coordinate or an entry of G that is not finite. */
int gpak_local_neighbours(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G /* d x d or NULL */,
                          int k, double radius, int threads, int *nbr /* k x M */, int *used /* M, may be NULL */);

/* Simple kriging of M nodes, each from the samples its own list names.
 * Samples: Xs (Ns x d, the layout of gpak_set_train) and ys (Ns): arguments of the call, NOT the context's training set.
 * The context supplies the device, its stream and the kernel in force (gpak_set_kernel / gpak_set_params, sn2 included);
 * it needs no training set, and if it holds one the call leaves it, its factor and everything derived from them alone: the
 * context's later answers are the bytes they would have been without the call.  No N x N and no Ns-proportional matrix is
 * allocated: the transformed samples take 15 * Ns doubles (rounded up to 128 samples) on the device for the length of the
 * call, ys, the raw columns (freed after the transform) and the node batches beside them.
 * Nodes: M blocks of nd points each, Xd (M * nd) x d in the layout of gpak_predict_block (nd = 1: points).
 * Lists: nbr[q + k * b], q < k <= GPAK_LOCAL_MAX, the sample indices of node b; unused slots are -1 and come only after
 * the used ones (what gpak_local_neighbours writes).  With I the s used entries of node b and noise = sn2 + white:
 *   K_II[i, j] = k(x_i, x_j) + bias + noise * delta_ij
 *   kbar_i     = (1 / nd) sum_a k(p_a, x_i) + bias
 *   kbb        = (1 / nd^2) sum_{a, a'} (k(p_a, p_a') + bias) + white / nd      the prior variance of gpak_predict_block
 *   mean       = kbar^T K_II^-1 y_I
 *   var        = kbb - kbar^T K_II^-1 kbar + sn2 / nd          without the last term under GPAK_LOCAL_LATENT
 * which is gpak_predict_block's definition applied to a model that holds the samples I only: a White child is part of the
 * field, so its white / nd sits in kbb (and stays under GPAK_LOCAL_LATENT, as under GPAK_BLOCK_LATENT), and the noise term
 * is sn2 / nd; without a White child that is noise / nd.  The variance is not clamped.  A node with s = 0 gets mean 0 and
 * its prior variance kbb (+ sn2 / nd) and is counted in `empty`.
 * Distances are ALWAYS the direct form |(x - x') A_t|^2, whatever the context's dist_mode; the transform is centred on the
 * samples' column means, which changes no difference beyond rounding.  Everything is fp64, also in a GPAK_F32 context;
 * every composition is accepted (1-3 terms, bias, White, d = 3 or 4).  Nodes stream in batches of GPAK_OPT_PRED_BATCH
 * (default 16384); a node's mean and variance are the same bytes whatever the batch size, M, the padding of its list (k)
 * or the other nodes, and two calls return the same bytes.  Sets predict_ms.
 * A repeated index in a list is the caller's business (with noise > 0 the matrix stays positive definite).  A pivot that
 * is not positive makes that node's mean and var quiet NaN and counts it in `notpd` (the kernel counts them itself: a NaN
 * that comes from a NaN in ys or Xd, which nothing refuses, is not counted); the call still returns GPAK_OK.
 * GPAK_EINVAL before anything is written: a NULL ctx, Xs, ys, Xd, nbr or mean; Ns, M or nd < 1 (Ns above INT_MAX - 128);
 * k outside 1..GPAK_LOCAL_MAX; an index outside -1..Ns-1; a valid index after a -1; bits in flags other than
 * GPAK_LOCAL_LATENT.  GPAK_ENOTIMPL: d other than 3 or 4, or other than the training set's when the context holds one; a
 * multi-GPU context.  GPAK_ESTATE without parameters.  GPAK_ENOMEM when an allocation fails. */
int gpak_predict_local(gpak_ctx *ctx, const double *Xs, const double *ys, long Ns, int d,
                       const double *Xd, long M, int nd, const int *nbr, int k,
                       double *mean, double *var /* may be NULL */, int flags, gpak_local_summary *summary /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_LOCAL_H */
