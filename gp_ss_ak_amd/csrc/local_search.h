// local_search.h -- the exact k-nearest-sample search of moving-neighbourhood kriging (gpak_local_neighbours,
// include/gpak_local.h).  Host code only: plain C++, no HIP, compiles alone (as potrf_plan.h does).
#pragma once

#define GPAK_LOCAL_SEARCH_MAX 128   // GPAK_LOCAL_MAX of include/gpak_local.h

// Xs: Ns x d column-major samples, Xc: M x d column-major centres, G: d x d column-major or null (identity).
//   t(x)_j = sum_r x_r G[r + d j]   (r ascending, every product and sum rounded on its own; null G: t(x) = x)
//   dist2  = sum_j (t(x)_j - t(c)_j)^2   (j ascending)
// nbr[q + k b], q < used[b]: the samples of centre b by ascending (dist2, index), with dist2 <= radius^2 when radius > 0;
// the remaining slots are -1.  Exact: the lists are those of a full sort of all Ns samples.  The search is a uniform cell
// grid over the first three transformed coordinates, visited ring by ring around the centre's cell until the k-th best
// distance lies inside the rings already seen; the centres are cut into `threads` contiguous slices, one std::thread each
// (threads <= 0: min(hardware concurrency, 16); never more than 256), and a centre's list does not depend on the slicing.
// Returns 0, or 2 (GPAK_EINVAL) for a null Xs, Xc or nbr, d other than 3 or 4, k outside 1..128, Ns or M < 1, Ns above
// INT_MAX, or a coordinate (raw or transformed) that is not finite.
extern "C" int gpak_local_neighbours(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k,
                                     double radius, int threads, int *nbr, int *used);
