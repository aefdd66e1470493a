/* gpak_dev_local.h -- the kernel of gpak_predict_local alone, on caller-owned device buffers: the conventions of gpak_dev.h
 * and gpak_dev_condition.h (the stream first, every pointer but `kern` a device pointer, status codes of gpak.h). */
#ifndef GPAK_DEV_LOCAL_H
#define GPAK_DEV_LOCAL_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Simple kriging of nB nodes, each from its own list of at most 128 samples (the formulas of gpak_predict_local in
 * gpak_local.h): per node the s listed samples are gathered, K_II is filled from the covariance function, factored and
 * solved in LDS; no matrix goes to global memory.
 * P: the nodes' transformed points POINT-MAJOR, as gpak_dev_kmm takes them -- point a of node b at index a * cap + b of
 * each array, the arrays nd * cap apart, five per term as gpak_dev_transform_k writes them.  u / ucap / n: the transformed
 * samples of the same call (same composition, same centre), ys their n values.  kern, bias, dist_mode: as gpak_dev_kmm
 * takes them (GPAK_DIST_HYB / GPAK_DIST_D4 of gpak_dev.h); the distance is the direct form whatever the low bits say.
 * white: the White child's variance -- white / nd in the prior variance kbb; the value a serialized composition carries in
 * kern[4] is not read.  noise: what is added to the diagonal of K_II (sn2 + white at the context level); the variance's
 * last term is (noise - white) / nd.  nbr: k x nB, nbr[q + k * b] the sample indices of node b, -1 from the first unused
 * slot on.  flags: 0 or GPAK_LOCAL_LATENT (gpak_local.h).
 * mean, var (may be NULL): nB doubles.  *info: the smallest node + 1 with a pivot that is not positive (its mean and var
 * are quiet NaN), or 0; the call writes it, whatever it held.
 * The tier -- the LDS image and whether a node takes one wave (k <= 32, four nodes per workgroup) or a workgroup -- is
 * chosen from k; the arithmetic of a node is the same in every tier: the same bytes whatever k pads its list to, whatever
 * nB and whatever the other nodes.  Everything but mean, var and info is only read.
 * EINVAL, nothing written: a NULL P, u, ys, kern, nbr, mean or info; nB, nd or n < 1; cap < nB; ucap < n; k outside 1..128;
 * flags with other bits; an unusable composition.  The indices are not checked on the host: a node's list ends at its first
 * entry outside 0..n-1, whatever that entry is (gpak_predict_local refuses such lists before it launches). */
int gpak_dev_local_krige(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n,
                         const double *ys, const double *kern, double bias, int dist_mode, double white, double noise,
                         const int *nbr, int k, int flags, double *mean, double *var, int *info);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_LOCAL_H */
