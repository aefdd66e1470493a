/* gpak_dev_condition.h -- the fused product of gpak_condition alone, on caller-owned device buffers: the conventions of
 * gpak_dev.h (the stream first, every pointer a device pointer, column-major, status codes of gpak.h). */
#ifndef GPAK_DEV_CONDITION_H
#define GPAK_DEV_CONDITION_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Z[b, s] = F0[b, s] + sum_j K-bar[b, j] A[j, s],  K-bar[b, j] = (1/nd) sum_a k(p_{b,a}, u_j) + bias,  b < nB, j < n, s < S:
 * the averaged cross-kernel is evaluated in the A-fragment layout of v_mfma_f64_16x16x4 and never stored.
 * P: the nB blocks' transformed points POINT-MAJOR -- point a of block b at index a * cap + b of each array, the arrays
 * nd * cap apart, five per term as gpak_dev_transform_k writes them (nd = 1: exactly its output for cap points); read up
 * to block nB - 1 only.  u / ucap / n: the transformed training points of the same call.  kern, bias, dist_mode: as
 * gpak_dev_fill_b takes them (GPAK_DIST_HYB / GPAK_DIST_D4 of gpak_dev.h).  A: n x S, leading dimension lda; F0: nB x S,
 * leading dimension ldf, or NULL for zeros; Z: nB x S, leading dimension ldz.
 * The samples are cut into gpak_dev_kmm_slabs(n) slabs whose boundaries depend on n rounded up to 128 alone; inside a slab
 * every element is one MFMA chain over j ascending, the slab sums are added in ascending order and F0 last.  scratch must
 * hold gpak_dev_kmm_slabs(n) * nB * S doubles.  Everything except Z and scratch is only read; of Z only the nB x S
 * elements are written.  Two calls return the same bytes, and an element does not depend on nB, S or the other blocks.
 * EINVAL, nothing written: a NULL P, u, kern, A, Z or scratch; nB, nd, n or S < 1; cap < nB; ucap < n; lda < n; ldf or
 * ldz < nB; an unusable composition. */
int gpak_dev_kmm(void *stream, const double *P, int cap, int nB, int nd, const double *u, int ucap, int n, const double *kern,
                 double bias, int dist_mode, const double *A, long lda, int S, const double *F0, long ldf, double *Z, long ldz,
                 double *scratch);
/* the number of sample slabs of gpak_dev_kmm for n training points, and the samples per slab */
int gpak_dev_kmm_slabs(int n);
int gpak_dev_kmm_slab_len(int n);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_CONDITION_H */
