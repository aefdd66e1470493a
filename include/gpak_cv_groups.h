/* gpak_cv_groups.h -- leave-group-out cross-validation from the factor.  Part of the context-level C-ABI: gpak.h includes
 * it, so a user of gpak.h has the call; same conventions (extern "C", status codes, host pointers, column-major). */
#ifndef GPAK_CV_GROUPS_H
#define GPAK_CV_GROUPS_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Leave out a whole group of training samples (a drill hole, a fold) and predict it jointly from all the others, for
 * every group at once and without a refit (Rasmussen & Williams 5.4.2 in block form).  With Ky = K + sn2 I = sn2 B,
 * B = L L^T, G = L^-T and alpha = Ky^-1 y, for a group with index set I of size s:
 *   S = [B^-1]_II = G_I G_I^T = R R^T,   e_I = sn2 S^-1 alpha_I,   mean_I = y_I - e_I,
 *   Sigma_I = sn2 S^-1 (the covariance of y_I given every sample outside the group, noise included),
 *   var_i = [Sigma_I]_ii,   logp_g = log N(y_I; mean_I, Sigma_I).
 * Groups of one sample give gpak_loo.  The cost is that of gpak_loo with L^-T held as ONE N x N matrix (the gradient's
 * workspace when it exists, otherwise a buffer of the call's own: GPAK_ENOMEM when it does not fit; GPAK_OPT_LOO_ROWS
 * does not apply) plus two small passes.  Everything is fp64, also in a GPAK_F32 context; no kernel parameters are
 * needed, so every composition works, White children included.  Runs gram / factor / alpha if they are stale and leaves
 * factor, alpha and nlZ valid; changes no field of gpak_timing; two calls return the same bytes.
 * Before anything is factored: GPAK_ESTATE without a training set or parameters; GPAK_EINVAL for a NULL group, n_groups
 * outside [1, N], a label outside [0, n_groups), an unused label or a group of more than GPAK_CV_GROUP_MAX samples (the
 * error text names the first offending sample or label); GPAK_ENOTIMPL for a multi-GPU context.
 * On GPAK_ENOTPD from the training factor every output that was passed is quiet NaN.  Should some S lose positive
 * definiteness to rounding, that group's outputs and the summary's values are NaN, the status is GPAK_ENOTPD and the
 * error text names the group. */
#define GPAK_CV_GROUP_MAX 128
typedef struct {
  double mse;      /* mean_i (y_i - mean_i)^2                                              */
  double mssr;     /* mean_i (y_i - mean_i)^2 / var_i (marginal variances)                 */
  double msmd;     /* (1/N) sum_g e_I' Sigma_I^-1 e_I: 1 for a calibrated model            */
  double log_pl;   /* sum_g logp_g: joint log predictive density of the left-out groups    */
  double ms;       /* device time of this call                                             */
  int    groups;   /* n_groups                                                             */
  int    max_size; /* largest group                                                        */
} gpak_cv_groups_summary;
/* group[i] in [0, n_groups) for each of the N training samples, in training order; every label used at least once;
 * no group larger than GPAK_CV_GROUP_MAX.  mean (N), var (N), group_logp (n_groups), summary: each may be NULL. */
int gpak_cv_groups(gpak_ctx *ctx, const int *group, int n_groups, double *mean, double *var, double *group_logp,
                   gpak_cv_groups_summary *summary);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_CV_GROUPS_H */
