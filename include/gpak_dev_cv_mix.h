/* gpak_dev_cv_mix.h -- the column mix of gpak_cv_folds_grad alone, on caller-owned device buffers: the conventions of
 * gpak_dev.h (the stream first, every pointer a device pointer, column-major, status codes of gpak.h). */
#ifndef GPAK_DEV_CV_MIX_H
#define GPAK_DEV_CV_MIX_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Z[:, c] = sum_{k<m} H[:, cols[k]] * Q[k, c]  (c < m, all Np rows), then H[:, cols[c]] = Z[:, c].  cols: m distinct
 * ascending device ints in [0, Np); Q m x m, ldq >= m; Z workspace Np x m_p, ldz >= Np.  Every other column of H, all of Q
 * and cols come back bit-identical; nothing of Z beyond Np x m is promised.  EINVAL: m < 1, m > Np, ld < Np, ldq < m, ldz < Np
 * The product is one fp64 MFMA kernel (each element of Z one accumulator chain over k ascending: two calls give the same
 * bytes); the write-back is a second launch, stream-ordered behind it. */
int gpak_dev_mix_cols(void *stream, double *H, long ld, int Np, const int *cols, int m, const double *Q, long ldq,
                      double *Z, long ldz);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_CV_MIX_H */
