/* gpak_design.h -- infill drilling design: rank candidate holes by the estimation variance they would remove from a set of
 * target blocks, exactly and without a refit.  Part of the context-level C-ABI, with the conventions of gpak.h (extern "C",
 * status codes, host pointers, column-major); gpak.h does NOT include it: include this header for the call. */
#ifndef GPAK_DESIGN_H
#define GPAK_DESIGN_H

#include "gpak_cv_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

/* var_before / var_after = sum_b wt_b P_bb before the first and after the last pick; ms = the call's device time
 * (predict_ms); holes = H, max_size = the points of the largest hole, picks = k */
typedef struct { double var_before, var_after, ms; int holes, max_size, picks; } gpak_design_summary;

/* Targets: T blocks of nd discretisation points each, uniform weights inside a block; Xt is (T * nd) x d in the layout of
 * gpak_predict_block (nd = 1: points); wt[b] >= 0 weighs block b (NULL: all ones).  Candidates: Mc points, Xc Mc x d,
 * hole[i] in [0, H) the hole of point i; every label is used, no hole has more than GPAK_CV_GROUP_MAX points, the points
 * of a hole need not be contiguous.
 *
 * Stack z = [block averages of the T targets; latent values at the Mc candidate points] and let P be its joint posterior
 * covariance given the training data -- gpak_predict_joint with GPAK_JOINT_LATENT on two segments of nd and of 1 point(s):
 *   P = prior - W W^T / sn2,  one row of W = L^-1 kbar per stacked entry,
 * the prior between a target block and a candidate point (1/nd) sum_a k(x_{b,a}, x_c); a White child puts white / nd on a
 * target's own diagonal entry and nothing anywhere else (not on a candidate's, not where a candidate coincides with a
 * target point).  The diagonal is not clamped.  For hole h with the index set I of its candidate rows:
 *   A_h = P_II + (sn2 + white) I = R R^T        the covariance of the noisy assays the hole would return
 *   reduction[b, h] = |R^-1 P_{I,b}|^2          the latent variance of block b now minus that with hole h in the training set
 *   gain[h] = sum_b wt_b reduction[b, h]        one chain over b ascending
 *   var[b] = P_bb
 * Greedy plan of k holes: take h* = argmax gain over the holes not yet taken (a tie goes to the smallest h), form
 * U = P_{:,I*} R^-T, update P <- P - U U^T over the whole stack, retire h* and score again: later gains are conditional on
 * the earlier picks.  picked[j], pick_gain[j] = the hole and its gain at the moment of pick j; var_after[b] = P_bb after
 * the last pick (= var for k = 0).  gain and reduction always report the first round, before any pick; k = 0 leaves
 * picked and pick_gain untouched.
 *
 * The stack is held at once: (T_p + Mc_p) rows of W by N_p and a (T_p + Mc_p)^2 matrix in the buffers of the joint calls
 * (T_p, Mc_p: T and Mc rounded up to 256), which is the size limit; candidates are not streamed.  Everything is fp64, also in
 * a GPAK_F32 context; every composition is accepted; for GPAK_DIST_EXPANSION the pooled mean is taken over the training
 * set, all T * nd target points and all Mc candidate points.  Runs gram / factor / alpha if they are stale, only reads
 * them, and sets predict_ms; two calls return the same bytes.
 * GPAK_EINVAL before anything is factored: T, nd or Mc <= 0; d other than the training set's; a NULL Xt, Xc, hole or gain;
 * H outside [1, Mc], a label outside [0, H), an unused label, a hole above GPAK_CV_GROUP_MAX points (the text names the
 * first offending point or label); a negative or non-finite weight; k outside [0, H]; picked or pick_gain NULL with k > 0;
 * points beyond the block path's 1 GiB budget.  GPAK_ESTATE without a training set or parameters, GPAK_ENOTIMPL for a
 * multi-GPU context, GPAK_ENOMEM when the stack does not fit.  GPAK_ENOTPD from the training factor: every output is quiet
 * NaN and the text says "training factor"; from a hole's A_h: the text names the hole and that hole's gain and
 * reduction are NaN. */
int gpak_design(gpak_ctx *ctx, const double *Xt, long T, int nd, const double *Xc, long Mc, int d, const int *hole, int H,
                const double *wt, int k, double *gain /* H */, double *reduction /* T x H column-major, may be NULL */,
                double *var /* T, may be NULL */, int *picked /* k */, double *pick_gain /* k */,
                double *var_after /* T, may be NULL */, gpak_design_summary *summary /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DESIGN_H */
