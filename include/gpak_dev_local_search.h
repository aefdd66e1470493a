/* gpak_dev_local_search.h -- the kernel of gpak_local_neighbours_dev alone, on caller-owned device buffers: the conventions
 * of gpak_dev_local.h (the stream first, every pointer a device pointer, status codes of gpak.h). */
#ifndef GPAK_DEV_LOCAL_SEARCH_H
#define GPAK_DEV_LOCAL_SEARCH_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The k nearest samples of nB centres, exactly, from samples binned into a uniform cell grid over their first three
 * transformed coordinates.  One wave per centre walks the cells ring by ring around the centre's cell and keeps its best k
 * in registers; no wave waits for another.
 * The grid: a sample with transformed coordinates t lies in cell a_j = min(max(floor((t_j - lo_j) / h), 0), n_j - 1), j < 3;
 * start is the running count over the cells and scale >= max |lo_j|, max |hi_j| of the samples.  Nothing else is assumed of
 * it: the lists are exact for every grid with these properties.  A centre outside the grid is taken to the layer of cells
 * just outside it.  Before ring r every unseen sample is at least (r - 1) h - slack away, slack = 1e-10 (scale + max_j |tc_j|
 * + h); the rings end when the list is full and its worst dist2 is strictly below that bound squared, when the bound passes
 * the radius, or with the grid.
 *   dist2 = sum_j (t_j - tc_j)^2, j ascending, every difference, product and sum rounded on its own (no fused multiply-add).
 * The transforms are NOT done here: pts and tc hold transformed coordinates.
 * nbr[q + k * b], q < used[b]: the samples of centre b by ascending (dist2, index); radius > 0 keeps only dist2 <= radius *
 * radius; the remaining slots are -1 -- the lists of gpak_local_neighbours (gpak_local.h).  A centre with a coordinate that
 * is not finite gets an empty list.  Everything but nbr, used, dist2 and visited is only read.
 * EINVAL, nothing written: a NULL pts, ids, start, tc or nbr; n or nB < 1; d other than 3 or 4; k outside 1..128; an n_j < 1;
 * h not positive and finite; a NaN radius. */
int gpak_dev_local_search(void *stream,
                          const double *pts,   /* n x d, sample-major, in cell order */
                          const int *ids,      /* n: their sample indices, ascending inside a cell */
                          const int *start,    /* n0 * n1 * n2 + 1: first slot of every cell, cell index (a0 * n1 + a1) * n2 + a2 */
                          int n, int d, double lo0, double lo1, double lo2, double h, int n0, int n1, int n2, double scale,
                          const double *tc,    /* nB x d, centre-major: the TRANSFORMED centres */
                          int nB, int k, double radius,
                          int *nbr,            /* k x nB */
                          int *used,           /* nB, may be NULL */
                          double *dist2,       /* k x nB, may be NULL: dist2 of every listed sample, 0.0 in the unused slots */
                          unsigned long long *visited /* may be NULL: += samples whose distance was formed */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_DEV_LOCAL_SEARCH_H */
