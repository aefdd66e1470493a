/* gpak_dev_design.h -- the score pass of gpak_design alone, on caller-owned device buffers: the conventions of gpak_dev.h
 * (the stream first, every pointer a device pointer, column-major, status codes of gpak.h). */
#ifndef GPAK_DEV_DESIGN_H
#define GPAK_DEV_DESIGN_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* P: the LOWER storage of a symmetric matrix of at least rows x rows, leading dimension ld; its first T columns are the
 * targets.  rows[offs[h] .. offs[h + 1]) = the rows of hole h, ascending, every one in [T, ld), at most 128 of them.  For
 * each of the n_live holes h = live[j] (live NULL: h = j), with I its rows:
 *   A = P_II + noise I = R R^T,  X = R^-1,  Z = X P_{I, 0..T-1}   (fp64 MFMA, each element one chain over the rows ascending)
 *   reduction[b + h * ldr] = sum_i Z_ib^2  (reduction may be NULL),  gain[h] = sum_b wt[b] * reduction[b, h], b ascending
 * (wt NULL: all ones).  A pivot that is not positive: that hole's outputs are quiet NaN and *info takes the minimum of its
 * value and h + 1 (set it to INT_MAX before the call).  P, rows, offs, live and wt are only read; nothing but gain[h],
 * column h of reduction (T entries) and *info is written.  Two calls return the same bytes.
 * EINVAL: a NULL P, rows, offs, gain or info; T < 1, n_live < 1, ld <= T, ldr < T with reduction set. */
int gpak_dev_design_score(void *stream, const double *P, long ld, int T, const int *rows, const int *offs, const int *live,
                          int n_live, double noise, const double *wt, double *gain, double *reduction, long ldr, int *info);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_DESIGN_H */
