/* gpak_local_search.h -- the neighbour search of moving-neighbourhood kriging on the device.  Part of the context-level
 * C-ABI, with the conventions of gpak.h (extern "C", status codes, host pointers, column-major); neither gpak.h nor
 * gpak_local.h includes it: include this header for the call. */
#ifndef GPAK_LOCAL_SEARCH_H
#define GPAK_LOCAL_SEARCH_H

#include "gpak.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grid_ms: binning the samples on the host, wall time; upload_ms: the grid's upload; search_ms: the centre batches (uploads,
 * kernel, copies back), both device time; centres = M; cells: cells of the grid; visited: samples whose distance was
 * formed, over all centres; batches: launches of the kernel; max_used: the longest list */
typedef struct { double grid_ms, upload_ms, search_ms; long centres, cells; unsigned long long visited; int batches, max_used; } gpak_local_search_summary;

/* gpak_local_neighbours (gpak_local.h) with the search on the device: the same arguments without `threads`, the same
 * checks, and nbr and used are the same bytes.  dist2 (k x M, may be NULL): dist2 of every listed sample in the arithmetic
 * gpak_local.h states, 0.0 in the unused slots.
 * The context supplies the device and its stream and nothing else: it needs neither parameters nor a training set, and if
 * it holds one the call leaves it, its factor and everything derived from them alone.  The samples are binned and both
 * point sets transformed on the host, by the code of the host search; the grid is uploaded once and the centres stream in
 * batches of GPAK_OPT_PRED_BATCH (default 16384), one launch of gpak_dev_local_search (gpak_dev_local_search.h) and one
 * host synchronisation each.  A centre's list does not depend on the batch size, on M or on the other centres.  The device
 * buffers (d doubles and an int per sample, an int per cell, a batch of centres and lists) are the call's own and are freed
 * before it returns.
 * GPAK_EINVAL before anything is written: a NULL ctx; what gpak_local_neighbours refuses; Ns above INT_MAX - 128.
 * GPAK_ENOTIMPL for a multi-GPU context.  GPAK_ENOMEM when an allocation fails. */
int gpak_local_neighbours_dev(gpak_ctx *ctx, const double *Xs, long Ns, int d, const double *Xc, long M, const double *G /* d x d or NULL */,
                              int k, double radius, int *nbr /* k x M */, int *used /* M, may be NULL */, double *dist2 /* k x M, may be NULL */,
                              gpak_local_search_summary *summary /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GPAK_LOCAL_SEARCH_H */
