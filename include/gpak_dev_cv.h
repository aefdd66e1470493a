/* gpak_dev_cv.h -- device-pointer level pieces of the cross-validation calls, on caller-owned device buffers: the
 * conventions of gpak_dev.h (the stream first, every pointer a device pointer, column-major, status codes of gpak.h). */
#ifndef GPAK_DEV_CV_H
#define GPAK_DEV_CV_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gather of gpak_cv_folds: m scattered rows of the Np x Np matrix G (leading dimension ld), from column k0 on, as a
 * dense operand.  P is m_p x (Np - k0) with m_p = m rounded up to 128 and leading dimension ldp >= m_p:
 *   P[r, c] = G[rows[r], k0 + c]  for r < m,      P[r, c] = 0  for m <= r < m_p
 * (the zero rows are written on every call).  rows: m device ints in [0, Np).  Nothing outside those m_p rows of the
 * Np - k0 columns of P is written and G is only read.  GPAK_EINVAL: m < 1, m > Np, k0 outside [0, Np), ld < Np or
 * ldp < m_p. */
int gpak_dev_pack_rows(void *stream, const double *G, long ld, int Np, const int *rows, int m, int k0, double *P, long ldp);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_CV_H */
