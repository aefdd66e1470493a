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

// The octant search (gpak_local_neighbours_octant, include/gpak_local_ok.h): the same transform, distances, grid and rings.
// The octant of a sample is the sign pattern of its first three transformed differences e_j = t(x)_j - t(c)_j: bit j is set
// when e_j < 0, a zero counting as non-negative; a fourth column counts in dist2 only.  Of the samples with dist2 <=
// radius^2 each octant keeps its per_octant nearest by (dist2, index) -- eight heaps filled in the one pass over the rings,
// which ends when every octant's heap is settled or the rings have left the radius -- and of those the k nearest are written
// in ascending (dist2, index), -1 after them.  Exact, and independent of `threads`; per_octant = k gives the lists of
// gpak_local_neighbours.  Returns 2 also for a radius that is not positive and finite (it is required: it is what ends the
// rings of a centre with an empty octant) and for per_octant outside 1..k.
extern "C" int gpak_local_neighbours_octant(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k,
                                            int per_octant, double radius, int threads, int *nbr, int *used);
