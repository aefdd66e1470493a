/* gpak_local_ok.h -- ordinary kriging and the octant search for moving-neighbourhood kriging.  An addition to gpak_local.h
 * (whose types and constants it uses) with the same conventions; gpak.h does NOT include it: include this header for the
 * calls. */
#ifndef GPAK_LOCAL_OK_H
#define GPAK_LOCAL_OK_H

#include "gpak_local.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ordinary kriging of M nodes, each from the samples its own list names: the mean is not the model's constant but is
 * re-estimated from every node's own samples, and the weights sum to one.  Arguments, layouts, checks, batching, statuses,
 * timers (predict_ms) and summary are those of gpak_predict_local, and so is the promise that a context which holds a
 * training set is left with it, its factor and everything derived from them untouched.  K_II, kbar and kbb are exactly
 * those of gpak_predict_local (the bias, the noise on the diagonal, a White child's white / nd in kbb).  With K_II = L L^T,
 * w_y = L^-1 y_I, w_k = L^-1 kbar and w_1 = L^-1 1:
 *   a      = w_1 . w_1      (= 1^T K_II^-1 1)          b_y = w_1 . w_y          b_k = w_1 . w_k
 *   mu     = b_y / a                                   the local mean
 *   mean   = w_k . w_y + (1 - b_k) mu
 *   latent = kbb - w_k . w_k + (1 - b_k)^2 / a         not clamped
 *   var    = latent + sn2 / nd                         latent alone under GPAK_LOCAL_LATENT
 * (the order of the operations is stated in gpak_dev_local_ok.h).  A constant added to the bias changes nothing but
 * rounding; a constant added to ys is added to mean and mu.
 * mean: M doubles; var and mu: M doubles or NULL.  A node's mean, var and mu are the same bytes whatever the batch size, M,
 * the padding of its list (k), the other nodes, and whether var or mu is asked for; two calls return the same bytes.
 * A pivot that is not positive makes the node's mean, var and mu quiet NaN and counts it in `notpd`.  A node whose list is
 * empty has no ordinary-kriging estimate: mean, var and mu are quiet NaN, and it is counted in `empty`, not in `notpd`.
 * The call still returns GPAK_OK.  Statuses: those of gpak_predict_local, before anything is written. */
int gpak_predict_local_ok(gpak_ctx *ctx, const double *Xs, const double *ys, long Ns, int d,
                          const double *Xd, long M, int nd, const int *nbr, int k,
                          double *mean, double *var /* may be NULL */, double *mu /* may be NULL */, int flags,
                          gpak_local_summary *summary /* may be NULL */);

/* The octant search: at most per_octant samples from each of the eight octants around a centre, so that samples clustered
 * down one drill hole cannot fill a list from one direction.  Host code only; no context, no device.
 * Xs, Ns, d, Xc, M, G, k, threads, nbr, used: as gpak_local_neighbours takes them, with the same arithmetic and rounding:
 *   t(x)_j = sum_r x_r G[r + d j]          r ascending, every product and sum rounded on its own (NULL G: t(x) = x)
 *   e_j    = t(x)_j - t(c)_j
 *   dist2  = sum_j e_j^2                   j ascending
 * and the same cell grid.  The octant of a sample is the sign pattern of e_0, e_1, e_2: bit j is set when e_j < 0; a zero
 * difference counts as non-negative, so ties have one answer.  With d = 4 the fourth column counts in dist2 only.
 * Of the samples with dist2 <= radius * radius, each octant keeps its per_octant nearest by (dist2, index); of those at
 * most 8 * per_octant samples the k nearest by (dist2, index) are written to nbr[q + k * b] in that order, -1 after them;
 * used[b] is their number.  Exact: the lists are those of a full sort and do not depend on `threads`.  With per_octant = k
 * the lists are those of gpak_local_neighbours at the same radius, byte for byte.
 * GPAK_EINVAL, nothing written: what gpak_local_neighbours refuses; a radius that is not a positive finite number (it is
 * REQUIRED here: without it a centre on the hull would visit every cell for the samples of an empty octant); per_octant
 * outside 1..k. */
int gpak_local_neighbours_octant(const double *Xs, long Ns, int d, const double *Xc, long M,
                                 const double *G /* d x d or NULL */, int k, int per_octant, double radius, int threads,
                                 int *nbr /* k x M */, int *used /* M, may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_LOCAL_OK_H */
