/* gpak_cv_folds_grad.h -- training on the k-fold criterion: gpak_cv_groups_grad without the limit on a group's size.
 * Part of the context-level C-ABI, with the conventions of gpak.h (extern "C", status codes, host pointers, column-major);
 * gpak.h does NOT include it: include this header for the call. */
#ifndef GPAK_CV_FOLDS_GRAD_H
#define GPAK_CV_FOLDS_GRAD_H

#include "gpak_cv_folds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient of F = -log_pl of gpak_cv_folds with the same labels and flags: gpak_cv_groups_grad.h has the formulas,
 *   dF / d theta = 1/2 sum_ij W_ij dK_ij / d theta,   W = H H^T - v alpha^T - alpha v^T,   H[:, I] = Kinv[:, I] Q_I,
 *   Q_I = sqrt(sn2) T + (beta / sqrt(sn2)) e_I w^T,   beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)),
 * with T = R^-T, w and e_I of gpak_cv_folds.h; the closed form holds for a group of any size.
 * The groups of at most GPAK_CV_GROUP_MAX samples go exactly as in gpak_cv_groups_grad, all of them in one launch per pass:
 * a labelling with no larger group and flags == 0 returns the bytes gpak_cv_groups_grad returns.  Every other group runs
 * the sequence of gpak_cv_folds alone, in ascending group number, and leaves its Q_I (m_p x m_p, m_p = its size rounded up
 * to 128) in a store; once Kinv stands as one N x N matrix, its columns I are multiplied by Q_I out of place (2 N m^2
 * flop) and written back: up to 256 columns by the fp64 MFMA column mix of gpak_dev_cv_mix.h, wider sets by a column
 * gather, the library's bulk fp64 product and a column scatter, which is the faster of the two there.
 * Workspaces beside the gradient's two N x N matrices and those of gpak_cv_folds: the store of the Q_I, sum of m_p^2
 * doubles over the groups above GPAK_CV_GROUP_MAX samples, and the N_p x m_p result of the mix for the largest of them
 * (twice that when it is wider than 256: the gathered operand beside the result), which shares the buffer of P (that
 * buffer holds the larger of the two).  GPAK_ENOMEM names the one that did not fit.
 * Everything is fp64, also in a GPAK_F32 context.  Runs gram / factor / alpha if they are stale, sets grad_ms and leaves
 * factor, alpha and nlZ valid; two calls return the same bytes.
 * Before anything is factored, with this call's name in the error text: GPAK_ESTATE without a training set or parameters;
 * GPAK_EINVAL for a NULL g or group, a wrong ng, an unknown bit in flags and every label error gpak_cv_folds refuses;
 * GPAK_ENOTIMPL for a composition with a White child and for a multi-GPU context.  On GPAK_ENOTPD from the training factor
 * g and the summary's values are quiet NaN.  Should some S lose positive definiteness to rounding, the status is
 * GPAK_ENOTPD, all of g is NaN and the error text names the group. */
/* g = dF/dtheta; layout and ng exactly as gpak_grad_exact; flags: GPAK_CV_FOLDS_NO_BATCH;
 * summary (may be NULL) = the bytes gpak_cv_folds returns on this context with these flags, except ms = grad_ms */
int gpak_cv_folds_grad(gpak_ctx *ctx, const int *group, int n_groups, double *g, int ng, gpak_cv_groups_summary *summary,
                       int flags);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_CV_FOLDS_GRAD_H */
