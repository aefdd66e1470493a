/* gpak_loo_grad.h -- training on the leave-one-out criterion.  Part of the context-level C-ABI: gpak.h includes it, so
 * a user of gpak.h has the call; same conventions (extern "C", status codes, host pointers, column-major). */
#ifndef GPAK_LOO_GRAD_H
#define GPAK_LOO_GRAD_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient of the leave-one-out objective F = -log_pl of gpak_loo (Rasmussen & Williams eq. 5.10-5.13), for fitting
 * a model to its cross-validation instead of the marginal likelihood.  With Kinv = (K + sn2 I)^-1, alpha = Kinv y and
 * kappa_i = Kinv_ii:  dF / d theta = 1/2 sum_ij W_ij dK_ij / d theta,  W = 2 Kinv diag(c) Kinv - v alpha^T - alpha v^T,
 * c_i = (1 / kappa_i + alpha_i^2 / kappa_i^2) / 2,  v = Kinv b,  b_i = alpha_i / kappa_i.  Same parameters, same
 * compositions and the same pair pass as gpak_grad_exact; the matrix work is N^3/3 + N^3/3 + N^3 flops in the gradient's
 * two N x N workspaces.  fp64 also in a GPAK_F32 context.  Runs gram / factor / alpha if they are stale, sets grad_ms and
 * leaves factor, alpha and nlZ valid.  The summary's mse, mssr, log_pl and passes are those of gpak_loo on the same
 * context, its ms is grad_ms.  GPAK_EINVAL for a NULL g or a wrong ng, GPAK_ESTATE without a training set or
 * parameters, GPAK_ENOTIMPL for a composition with a White child and for a multi-GPU context -- all three before anything
 * is factored; on GPAK_ENOTPD g and the summary's three values are quiet NaN. */
/* g = dF/dtheta, F = -log_pl of gpak_loo; layout and ng exactly as gpak_grad_exact; summary may be NULL */
int gpak_loo_grad(gpak_ctx *ctx, double *g, int ng, gpak_loo_summary *summary);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_LOO_GRAD_H */
