/* gpak_dev_cv_kernels.h -- every kernel of the cross-validation calls (gpak_loo, gpak_cv_groups, gpak_cv_folds and their
 * _grad forms) alone, on caller-owned device buffers: the conventions of gpak_dev.h (the stream first, every pointer a
 * device pointer, column-major, status codes of gpak.h, GPAK_EINVAL before any launch).  Each entry runs the launch code
 * of the library's own calls -- grids, LDS sizes and the one-time opt-in included -- on the arguments given here.  What an
 * entry does not list as written comes back bit for bit.  The index lists live on the device; their CONTENTS cannot be
 * checked before the launch and are the caller's contract. */
#ifndef GPAK_DEV_CV_KERNELS_H
#define GPAK_DEV_CV_KERNELS_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the batched groups of at most 128 samples (gpak_cv_groups; the small folds of gpak_cv_folds) ----------------------
 * perm: the members of all groups, group after group, each group's members ASCENDING, in [0, Np); offs[g] .. offs[g + 1]:
 * where group g sits in perm (n_groups + 1 ints, every size s in [1, 128]); soff[g]: where the S of group g starts in S
 * (doubles), sp * sp doubles each with sp = s rounded up to 16. */

/* S_g = G_I G_I^T of every group, I its members, from the rows I of the upper triangular Np x Np matrix G (leading
 * dimension ld): S_ij = sum_{k >= k0} G[I_i, k] G[I_j, k], k0 = the 128-tile of the group's smallest row -- columns left
 * of k0 are not read -- one accumulator chain over k ascending (the bytes do not depend on ld, on the other groups or on
 * their order).  Written, column-major with leading dimension sp at S + soff[g]: the 16 x 16 tiles on and below the
 * diagonal tiles, whole, rows and columns s .. sp - 1 of them +0.  The tiles strictly above the diagonal tiles are not
 * written.  Read: the rows I of G, perm, offs, soff.  GPAK_EINVAL: a NULL pointer, n_groups < 1, Np < 128 or not a
 * multiple of 128, ld < Np. */
int gpak_dev_cvg_gram(void *stream, const double *G, long ld, int Np, const int *perm, const int *offs, int n_groups,
                      const long long *soff, double *S);

/* Every group from its S (the lower triangle of the s x s block is read; layout as above): S = R R^T, X = R^-1,
 *   e = sn2 S^-1 alpha_I,  mean[I] = y[I] - e,  var[I_i] = sn2 sum_j X_ji^2,
 *   logp[g] = -1/2 alpha_I . e - 1/2 (s log sn2 - 2 sum_j log R_jj) - s/2 log 2 pi,
 *   gsum[3 g ..] = sum e_i^2, sum e_i^2 / var_i, alpha_I . e.
 * mean, var: written at the members only.  max_size: the largest s (it sizes the LDS of the launch).  A group whose S has a
 * pivot that is not positive: NaN in its mean, var, logp and gsum, and *info = min(*info, g + 1); the caller presets *info
 * (INT_MAX).  E, Qb, qoff all NULL: the plain variant.  All three given: the weights variant, the same arithmetic and
 * bytes, and for every group that did not fail E[I] = e (at the members only) and
 *   Q = sqrt(sn2) X^T + (beta / sqrt(sn2)) e w^T,  w = X alpha_I,  beta = sn2 / (1 + sqrt(1 + sn2 |w|^2)),
 * so that Q Q^T = sn2 S^-1 + e e^T, written ROW-major with pitch 128 at Qb + qoff[g]: the s x s entries only.
 * GPAK_EINVAL: a NULL pointer among the first, n_groups < 1, max_size outside [1, 128], sn2 not positive, one or two of
 * E, Qb, qoff given. */
int gpak_dev_cvg_solve(void *stream, const double *S, const long long *soff, const int *perm, const int *offs, int n_groups,
                       int max_size, const double *y, const double *alpha, double sn2, double *mean, double *var,
                       double *logp, double *gsum, int *info, double *E, double *Qb, const long long *qoff);

/* H[:, cols] <- H[:, cols] Qbin in place for every bin b < n_bins: cols = perm[bstart[b] .. bstart[b + 1]) (distinct, at
 * most 128, the bins disjoint), Qbin the 128 x 128 ROW-major matrix at Qb + b * 128 * 128 of which the first width rows
 * are read and the leading width x width block decides the result.  All Np rows of H (leading dimension ld).  Every element is one accumulator chain over the bin's
 * columns in list order.  Written: the listed columns of H.  GPAK_EINVAL: a NULL pointer, n_bins < 1, Np < 128 or not a
 * multiple of 128, ld < Np. */
int gpak_dev_cvg_mix(void *stream, double *H, long ld, int Np, const int *perm, const int *bstart, int n_bins,
                     const double *Qb);

/* ---- the stages of a group above 128 samples, one group at a time (gpak_cv_folds) --------------------------------------
 * m: the group's size, m_p = m rounded up to 128.  rows: its m members (device ints).  T = R^-T is upper triangular m_p x
 * m_p with leading dimension ldt; what lies below its diagonal is never read.  info: one device int, INT_MAX unless the
 * group's factorisation failed. */

/* Rows and columns m .. m_p - 1 of the LOWER triangle of S (leading dimension lds) become the identity.  Nothing else is
 * written; m = m_p launches nothing.  GPAK_EINVAL: S NULL, m < 1, lds < m_p. */
int gpak_dev_cvf_pad(void *stream, double *S, long lds, int m);

/* wv[j] = sum_{i <= j} T[i, j] alpha[rows[i]] for j < m.  GPAK_EINVAL: a NULL pointer, m < 1, ldt < m. */
int gpak_dev_cvf_w(void *stream, const double *T, long ldt, int m, const int *rows, const double *alpha, double *wv);

/* ev[i] = sn2 sum_{j >= i} T[i, j] wv[j], vv[i] = sn2 sum_{j >= i} T[i, j]^2 (i, j < m); mean[rows[i]] = y[rows[i]] -
 * ev[i], var[rows[i]] = vv[i].  *info != INT_MAX: NaN in all four.  GPAK_EINVAL: a NULL pointer, m < 1, ldt < m. */
int gpak_dev_cvf_ev(void *stream, const double *T, long ldt, int m, const double *wv, const int *rows, const double *y,
                    double sn2, const int *info, double *ev, double *vv, double *mean, double *var);

/* gsum[0..2] = sum ev_i^2, sum ev_i^2 / vv_i, sum alpha[rows[i]] ev_i and
 * logp[0] = -1/2 gsum[2] - 1/2 (m log sn2 - 2 sum_i log R[i, i]) - m/2 log 2 pi: of R (leading dimension ldr) the first m
 * diagonal entries are read.  *info != INT_MAX: NaN in all four.  GPAK_EINVAL: a NULL pointer, m < 1, ldr < m. */
int gpak_dev_cvf_sums(void *stream, const double *R, long ldr, int m, const double *ev, const double *vv, const int *rows,
                      const double *alpha, double sn2, const int *info, double *logp, double *gsum);

/* sc[0] = sqrt(sn2), sc[1] = beta / sqrt(sn2) with beta = sn2 / (1 + sqrt(1 + sn2 |wv|^2)).  GPAK_EINVAL: a NULL pointer,
 * m < 1. */
int gpak_dev_cvf_beta(void *stream, const double *wv, int m, double sn2, double *sc);

/* Q[i, j] = sc[0] T[i, j] + sc[1] ev[i] wv[j] for i, j < m (T[i, j] = 0 for j < i) and +0 on the rest of m_p x m_p, with
 * leading dimension ldq; transposed != 0: Q^T so stored.  E[rows[i]] = ev[i]: E is written at the members only.
 * GPAK_EINVAL: a NULL pointer, m < 1, ldt < m, ldq < m_p. */
int gpak_dev_cvf_q(void *stream, int transposed, const double *T, long ldt, int m, const double *wv, const double *ev,
                   const double *sc, const int *rows, double *Q, long ldq, double *E);

/* A[:, c] = H[:, cols[c]] for c < m and +0 for m <= c < m_p, all Np rows (A: leading dimension lda).
 * GPAK_EINVAL: a NULL pointer, m < 1, m > Np, ld < Np, lda < Np. */
int gpak_dev_cvf_gather(void *stream, const double *H, long ld, int Np, const int *cols, int m, double *A, long lda);

/* H[:, cols[c]] = Z[:, c] for c < m, all Np rows (cols distinct).  GPAK_EINVAL: a NULL pointer, m < 1, m > Np, ld < Np,
 * ldz < Np. */
int gpak_dev_cvf_unmix(void *stream, double *H, long ld, int Np, const int *cols, int m, const double *Z, long ldz);

/* ---- leave-one-out (gpak_loo, gpak_loo_grad) and what gpak_cv_groups_grad shares with it --------------------------------
 * Np: a multiple of 128.  A slab holds pass a of P of the upper triangular G: local row r is global row
 * ((r / 128) * P + a) * 128 + r % 128, all Np columns, leading dimension lds; rows = 128 * (the number of 128-row blocks
 * g < Np / 128 with g = a mod P). */

/* d[i] = sum_{k >= 128 (i / 128)} G[i, k]^2 for the global rows i of the pass: the same bytes whatever P, a or lds.  The
 * 512-column chunks strictly left of a row block's diagonal block are neither read nor written.  part: workspace of
 * ceil(Np / 512) * rows doubles (the chunk sums; the chunks left of the diagonal's stay as they were).  Of d only the
 * pass's rows are written.  GPAK_EINVAL: a NULL pointer, Np < 128 or not a multiple of 128, P < 1, a outside [0, P), a
 * pass without rows, lds < rows, lds odd or slab not 16-byte aligned (the loads are 16 bytes wide). */
int gpak_dev_loo_rowsumsq(void *stream, const double *slab, long lds, int Np, int P, int a, double *part, double *d);

/* var[i] = sn2 / d[i], mean[i] = y[i] - alpha[i] var[i] for i < N (nothing beyond N is read or written) and
 * sums[0..2] = sum (y - mean)^2, sum (y - mean)^2 / var, sum log var, added in a fixed order.  part: workspace of
 * ceil(N / 256) * 16 doubles, of which the first three of every 16 are written.  GPAK_EINVAL: a NULL pointer, N < 1, sn2
 * not positive. */
int gpak_dev_loo_finish(void *stream, int N, const double *d, const double *y, const double *alpha, double sn2, double *mean,
                        double *var, double *part, double *sums);

/* For i < N, with ik = sn2 / d[i] and b = alpha[i] ik: s[i] = sqrt((ik + b^2) / 2) / sn2, r[i] = b / sn2; +0 for
 * N <= i < Np.  GPAK_EINVAL: a NULL pointer, N < 1, N > Np, sn2 not positive. */
int gpak_dev_loo_vectors(void *stream, int N, int Np, const double *d, const double *alpha, double sn2, double *s, double *r);

/* H[i, k] = s[k] * Binv[max(i, k), min(i, k)] for i, k < N and +0 on the rest of Np x Np: the full matrix from the 64 x 64
 * tiles of Binv on and below the diagonal tiles, which are read whole; nothing above them is read.  s: Np entries.
 * GPAK_EINVAL: a NULL pointer, N < 1, N > Np, Np < 128 or not a multiple of 128, ldb or ldh < Np or odd, Binv or H not
 * 16-byte aligned. */
int gpak_dev_loo_mirror_scale(void *stream, int N, int Np, const double *Binv, long ldb, const double *s, double *H, long ldh);

/* W[i, j] -= v[i] alpha[j] + alpha[i] v[j] on the 64 x 64 tiles on and below the diagonal tiles (whole), in place; the
 * tiles above them are neither read nor written.  v, alpha: Np entries.  GPAK_EINVAL: a NULL pointer, Np < 128 or not a
 * multiple of 128, ld < Np or odd, W, v or alpha not 16-byte aligned. */
int gpak_dev_loo_rank2(void *stream, int Np, double *W, long ld, const double *v, const double *alpha);

/* s[i] = c for i < N and +0 for N <= i < Np.  GPAK_EINVAL: s NULL, N < 0, N > Np, Np < 1. */
int gpak_dev_lgo_colscale(void *stream, int N, int Np, double c, double *s);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_CV_KERNELS_H */
