/* gpak_dev_local_ok.h -- the kernel of gpak_predict_local_ok alone, on caller-owned device buffers: ordinary kriging in a
 * moving neighbourhood.  The conventions of gpak_dev_local.h (the stream first, every pointer but `kern` a device pointer,
 * status codes of gpak.h); gpak_dev.h does NOT include it. */
#ifndef GPAK_DEV_LOCAL_OK_H
#define GPAK_DEV_LOCAL_OK_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ordinary kriging of nB nodes, each from its own list of at most 128 samples.  Every argument up to `flags` is that of
 * gpak_dev_local_krige (gpak_dev_local.h) and means the same; K_II, kbar and kbb are the same values, evaluated by the same
 * code.  The LDS image has one row more, the ones vector under y_I^T and kbar^T, so the factorisation K_II = L L^T leaves
 *   w_y = L^-1 y_I,  w_k = L^-1 kbar,  w_1 = L^-1 1
 * and five dot products are summed, each element j by lane j mod 64 in ascending j, then one xor-butterfly of the 64 lanes:
 *   m0 = w_k . w_y,  q = w_k . w_k,  a = w_1 . w_1,  b_y = w_1 . w_y,  b_k = w_1 . w_k
 * One lane then computes, in this order, every operation rounded once (fma: one rounding):
 *   mu   = b_y / a                          the local mean: the GLS estimate from the node's own samples
 *   r    = 1 - b_k
 *   t    = r / a
 *   mean = fma(r, mu, m0)
 *   var  = fma(r, t, kbb - q) + add         add = (noise - white) / nd, or 0 under GPAK_LOCAL_LATENT; not clamped
 * which is the system [K_II 1; 1^T 0][lambda; nu] = [kbar; 1] solved by block elimination: the weights sum to one and no
 * indefinite matrix is factored.  a > 0 whenever the factor exists.
 * mean, var (may be NULL), mu (may be NULL): nB doubles.  *info: the smallest node + 1 with a pivot that is not positive
 * (its mean, var and mu are quiet NaN), or 0; the call writes it, whatever it held.  A node whose list is EMPTY has no
 * ordinary-kriging estimate: its mean, var and mu are quiet NaN and it does not touch *info.
 * A node's bytes are the same in every tier: whatever k pads its list to, whatever nB and whatever the other nodes.
 * Everything but mean, var, mu and info is only read.
 * EINVAL, nothing written: as gpak_dev_local_krige -- a NULL P, u, ys, kern, nbr, mean or info; nB, nd or n < 1; cap < nB;
 * ucap < n; k outside 1..128; flags with bits other than GPAK_LOCAL_LATENT; an unusable composition. */
int gpak_dev_local_krige_ok(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n,
                            const double *ys, const double *kern, double bias, int dist_mode, double white, double noise,
                            const int *nbr, int k, int flags, double *mean, double *var, double *mu, int *info);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_LOCAL_OK_H */
