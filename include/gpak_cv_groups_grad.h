/* gpak_cv_groups_grad.h -- training on the leave-group-out criterion.  Part of the context-level C-ABI, with the
 * conventions of gpak.h (extern "C", status codes, host pointers, column-major); gpak.h does NOT include it: include this
 * header for the call. */
#ifndef GPAK_CV_GROUPS_GRAD_H
#define GPAK_CV_GROUPS_GRAD_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient of the leave-group-out objective F = -log_pl of gpak_cv_groups, for fitting a model to the honest
 * cross-validation of grouped data (drill holes) instead of the marginal likelihood or the leave-one-out criterion.  With
 * Kinv = (K + sn2 I)^-1, alpha = Kinv y and, per group I, S = sn2 [Kinv]_II, e_I = y_I - mean_I = sn2 S^-1 alpha_I:
 *   F = sum_g [ 1/2 alpha_I . e_I - 1/2 log |S / sn2| ] + N/2 log 2 pi,   dF / d theta = 1/2 sum_ij W_ij dK_ij / d theta,
 *   W = Kinv C Kinv - v alpha^T - alpha v^T,   C = blockdiag(sn2 S^-1 + e_I e_I^T),   v = Kinv e.
 * Groups of one sample give gpak_loo_grad.  Same parameters, same compositions and the same pair pass as gpak_grad_exact;
 * the matrix work is that of gpak_loo_grad (N^3/3 + N^3/3 + N^3 flops in the gradient's two N x N workspaces) plus the two
 * passes of gpak_cv_groups and one N x N column mix.  fp64 also in a GPAK_F32 context.  Runs gram / factor / alpha if they
 * are stale, sets grad_ms and leaves factor, alpha and nlZ valid; two calls return the same bytes.
 * The labels are those of gpak_cv_groups: group[i] in [0, n_groups) for each training sample, every label used, no group
 * larger than GPAK_CV_GROUP_MAX.  The summary's mse, mssr, msmd, log_pl, groups and max_size are the bytes gpak_cv_groups
 * returns on the same context; its ms is grad_ms.
 * Before anything is factored: GPAK_ESTATE without a training set or parameters; GPAK_EINVAL for a NULL g or group, a
 * wrong ng and every label error gpak_cv_groups refuses; GPAK_ENOTIMPL for a composition with a White child and for a
 * multi-GPU context.  On GPAK_ENOTPD from the training factor g and the summary's values are quiet NaN.  Should some S
 * lose positive definiteness to rounding, the status is GPAK_ENOTPD, all of g is NaN and the error text names the group. */
/* g = dF/dtheta, F = -log_pl of gpak_cv_groups with the same labels; layout and ng exactly as gpak_grad_exact;
 * summary (may be NULL) = the bytes gpak_cv_groups returns on this context, except ms = grad_ms */
int gpak_cv_groups_grad(gpak_ctx *ctx, const int *group, int n_groups, double *g, int ng, gpak_cv_groups_summary *summary);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_CV_GROUPS_GRAD_H */
