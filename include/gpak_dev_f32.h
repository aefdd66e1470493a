/* gpak_dev_f32.h -- the fp32 prediction kernels of a GPAK_F32 context, each ALONE on caller-owned device buffers.
 * Part of the device-pointer level C-ABI: same conventions as gpak_dev.h (extern "C", status codes, every pointer a
 * device pointer, column-major, calls only enqueue on `stream`).  Every entry point is a thin wrapper over the launcher
 * the prediction itself uses (csrc/gemm_f32.hip, the ladder of csrc/predict.hip), so what a caller runs here is the
 * product's code under the process-wide kernel tuning (GPAK_F32_ACC, GPAK_F32_RSD, GPAK_F32_TILE, gpak_reload_tuning).
 * A refusal returns GPAK_EINVAL and writes nothing. */
#ifndef GPAK_DEV_F32_H
#define GPAK_DEV_F32_H

#include "gpak.h"     /* the status codes */
#include "gpak_dev.h" /* GPAK_DIST_HYB, GPAK_DIST_D4, gpak_dev_transform_k */

#ifdef __cplusplus
extern "C" {
#endif

/* C (128 mt x 128 nt, ldc) = beta C + alpha A B^T, A: 128 mt x K (lda), B: 128 nt x K (ldb).  beta == 0 never reads C.
 * K > 128 takes the wide-accumulation kernel (fp32 chunks of 128 summed in fp64) unless GPAK_F32_ACC=plain.
 * GPAK_EINVAL: K < 128 or no multiple of 128 (the only K the ladder produces), a leading dimension below the rows or no
 * multiple of 4, a pointer that is not 16-byte aligned, A == C with nt != 1 or K != 128 (the ladder's one in-place
 * product: W_j := W_j inv(D_j)^T).  mt <= 0 or nt <= 0: nothing to do, GPAK_OK. */
int gpak_dev_gemm_nt_f32(void *stream, int mt, int nt, int K, float alpha, const float *A, long lda, const float *B,
                         long ldb, float beta, float *C, long ldc);

/* C[i, j] = (float) k(p_i, q_j) for i < nP, j < nQ and 0.0f elsewhere in rows_p x cols_p (ld): the cross-kernel of the
 * fp32 prediction, WITHOUT Sigma_White.  uP / uQ: points transformed by gpak_dev_transform_k under the same kern /
 * dist_mode (GPAK_DIST_HYB and GPAK_DIST_D4 as there; the distance is always formed directly, from differences).
 * GPAK_EINVAL: rows_p <= 0 or no multiple of 128, cols_p <= 0 or no multiple of 64, capP < rows_p or odd (rows are read
 * in pairs up to rows_p), nP outside [0, rows_p], nQ outside [0, min(cols_p, capQ)], uP not 16-byte aligned, ld < rows_p
 * or odd, C not 8-byte aligned, a composition gpak_build_kp refuses. */
int gpak_dev_fill_f32(void *stream, const double *uP, int capP, int nP, const double *uQ, int capQ, int nQ, int rows_p,
                      int cols_p, const double *kern, double bias, int dist_mode, float *C, long ld);

/* out[r + c ldo] = (float) L[r + c ld] for r >= c, 0.0f above the diagonal, r, c < Np.  GPAK_EINVAL: Np <= 0, ld or ldo
 * below Np. */
int gpak_dev_lower_to_f32(void *stream, const double *L, long ld, int Np, float *out, long ldo);
/* out[i] = (float) in[i], i < n.  n == 0: nothing to do. */
int gpak_dev_vec_to_f32(void *stream, const double *in, long n, float *out);

/* part[s part_ld + t] = sum of V[t, c]^2 (in fp64) over the columns of split s, t < rows: split s holds columns
 * [s cps, min(cols, (s + 1) cps)), cps = ceil(cols / splits).  GPAK_EINVAL: rows or cols <= 0, splits outside
 * [1, cols], ldv or part_ld below rows. */
int gpak_dev_rowsumsq_f32(void *stream, const float *V, long ldv, int rows, int cols, int splits, double *part,
                          int part_ld);

/* Wt (mrows x Np, ldw) := Wt Lf^-T: the ladder of the fp32 forward substitution.  Lf: the fp32 image of the factor
 * (gpak_dev_lower_to_f32, ldLf); invf: the fp32 image (gpak_dev_vec_to_f32) of the Np / 128 pairs of inverse diagonal
 * blocks as gpak_dev_factor_panel leaves them.  levels (HOST array): ascending block widths, each a multiple of the one
 * before, the first 128; nlevels == 0: 128 / 512.  GPAK_EINVAL: any other levels, more than 8 of them, mrows or Np <= 0
 * or no multiple of 128, ldw below mrows or ldLf below Np or either no multiple of 4, a pointer that is not 16-byte
 * aligned. */
int gpak_dev_fwd_subst_f32(void *stream, float *Wt, long ldw, int mrows, int Np, const float *Lf, long ldLf,
                           const float *invf, const int *levels, int nlevels);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_F32_H */
