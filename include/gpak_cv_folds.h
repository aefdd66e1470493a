/* gpak_cv_folds.h -- k-fold cross-validation from the factor: gpak_cv_groups without the limit on a group's size.
 * Context-level C-ABI, same conventions as gpak.h (extern "C", status codes, host pointers, column-major).  gpak.h does
 * not include this header: include it where the call is used. */
#ifndef GPAK_CV_FOLDS_H
#define GPAK_CV_FOLDS_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Leave out a whole group of training samples and predict it jointly from all the others, for every group and without a
 * refit: the numbers of gpak_cv_groups (gpak_cv_groups.h has the formulas), for groups of ANY size -- the k folds of
 * N / k samples of k-fold cross-validation, a drill hole of 150 samples.
 * Groups of at most GPAK_CV_GROUP_MAX samples take the batched kernels of gpak_cv_groups, all of them in one launch each:
 * a labelling with no larger group returns the bytes gpak_cv_groups returns.  Every other group is processed alone, one
 * after another in ascending group number: its rows of G = L^-T are packed into a dense matrix P, S = P P^T is formed by
 * the fp64 MFMA product, factored S = R R^T, inverted T = R^-T, and
 *   w = T^T alpha_I,  e_I = sn2 T w,  mean_I = y_I - e_I,  var_i = sn2 sum_{j >= i} T_ij^2,
 *   logp_g = -1/2 alpha_I . e_I - 1/2 (m log sn2 - 2 sum_j log R_jj) - m/2 log 2 pi.
 * A group's numbers depend on its member set and the training factor alone: not on the other groups, the numbering of the
 * labels or the buffer that holds G.  GPAK_CV_FOLDS_NO_BATCH sends every group, whatever its size, down the second path.
 * Workspaces beside L^-T as one N x N matrix (as gpak_cv_groups): P, m_p x (N_p - k0) doubles with m_p the largest such
 * group rounded up to 128, and S, m_p x m_p; kept by the context.  GPAK_ENOMEM names the one that did not fit.
 * Everything is fp64, also in a GPAK_F32 context; every composition works, White children included.  Runs gram / factor /
 * alpha if they are stale and leaves factor, alpha and nlZ valid; changes no field of gpak_timing; two calls return the
 * same bytes.
 * Before anything is factored: GPAK_ESTATE without a training set or parameters; GPAK_EINVAL for a NULL group, n_groups
 * outside [1, N], a label outside [0, n_groups), an unused label (the error text names the first offending sample or
 * label) or an unknown bit in flags; GPAK_ENOTIMPL for a multi-GPU context.
 * On GPAK_ENOTPD from the training factor every output that was passed is quiet NaN.  Should some S lose positive
 * definiteness to rounding, that group's outputs and the summary's values are NaN, the status is GPAK_ENOTPD and the
 * error text names the group. */
#define GPAK_CV_FOLDS_NO_BATCH 1   /* every group, whatever its size, takes the one-group-at-a-time path */
/* group[i] in [0, n_groups) for each of the N training samples, in training order; every label used at least once.
 * mean (N), var (N), group_logp (n_groups), summary: each may be NULL. */
int gpak_cv_folds(gpak_ctx *ctx, const int *group, int n_groups, double *mean, double *var, double *group_logp,
                  gpak_cv_groups_summary *summary, int flags);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_CV_FOLDS_H */
