// local_search.cpp -- gpak_local_neighbours and gpak_local_neighbours_octant: see local_search.h.  No HIP in this file.
#include "local_search.h"
#include "local_grid.h"   // transform_point, Grid, build_grid: shared with the device search

#include <algorithm>
#include <climits>
#include <cmath>
#include <thread>
#include <utility>
#include <vector>

namespace {

using gpak_local_grid::Grid;
using gpak_local_grid::build_grid;
using gpak_local_grid::transform_point;

// Every sample inside `radius` (all of them when radius <= 0) is handed to take(dist2, index, octant), ring by ring of
// cells around the centre's cell, until stop(lb) says that no sample at least lb >= 0 away is wanted any more.  The octant
// is the sign pattern of the first three differences: bit j set when t(x)_j - t(c)_j < 0.
// false: a transformed coordinate of the centre is not finite
template <class Stop, class Take>
bool visit_rings(const Grid &g, const double *tc, double radius, Stop stop, Take take) {
  const int d = g.d;
  const double r2max = radius * radius;
  int ic[3], r0 = 0, r_end = 0;
  double cmax = 0.0;
  for (int j = 0; j < d; j++) {
    if (!std::isfinite(tc[j])) return false;
    cmax = std::max(cmax, std::fabs(tc[j]));
  }
  for (int j = 0; j < 3; j++) {
    // a centre outside the grid is taken to the layer of cells just outside it: every sample is then at least as far from
    // the centre as from that cell, so the ring bound below stays a lower bound, and the ring arithmetic stays small
    const double f = std::floor((tc[j] - g.lo[j]) / g.h);
    ic[j] = f < -1.0 ? -1 : (f > (double)g.n[j] ? g.n[j] : (int)f);
    r0 = std::max(r0, std::max(-ic[j], ic[j] - (g.n[j] - 1)));
    r_end = std::max(r_end, std::max(ic[j], g.n[j] - 1 - ic[j]));
  }
  // rounding in the cell assignment and in the differences: far below a cell, far above an ulp of any coordinate
  const double slack = 1e-10 * (g.scale + cmax + g.h);
  for (int r = r0; r <= r_end; r++) {
    if (r > 0) {   // every sample not yet seen is at least (r - 1) h away
      const double lb = (double)(r - 1) * g.h - slack;
      if (lb > 0.0 && (stop(lb) || (radius > 0.0 && lb > radius))) break;
    }
    const int a0lo = std::max(0, ic[0] - r), a0hi = std::min(g.n[0] - 1, ic[0] + r);
    const int a1lo = std::max(0, ic[1] - r), a1hi = std::min(g.n[1] - 1, ic[1] + r);
    for (int a0 = a0lo; a0 <= a0hi; a0++)
      for (int a1 = a1lo; a1 <= a1hi; a1++) {
        const bool shell = std::abs(a0 - ic[0]) == r || std::abs(a1 - ic[1]) == r;
        int a2lo = std::max(0, ic[2] - r), a2hi = std::min(g.n[2] - 1, ic[2] + r), step = 1;
        if (!shell) {   // only the two faces ic2 - r and ic2 + r
          a2lo = ic[2] - r; a2hi = ic[2] + r; step = r > 0 ? 2 * r : 1;
        }
        for (long a2 = a2lo; a2 <= a2hi; a2 += step) {
          if (a2 < 0 || a2 >= g.n[2]) continue;
          const size_t c = g.cell_index(a0, a1, (int)a2);
          for (long p = g.start[c]; p < g.start[c + 1]; p++) {
            const double *t = &g.pts[(size_t)p * d];
            double e = t[0] - tc[0];
            int oct = e < 0.0 ? 1 : 0;
            double s = e * e;
            for (int j = 1; j < d; j++) {
              e = t[j] - tc[j];
              if (j < 3 && e < 0.0) oct |= 1 << j;
              s = s + e * e;
            }
            if (radius > 0.0 && !(s <= r2max)) continue;
            take(s, g.ids[p], oct);
          }
        }
      }
  }
  return true;
}

typedef std::pair<double, int> Cand;   // (dist2, index): the order of the lists

// the `cap` smallest candidates seen so far, as a max-heap
struct Best {
  Cand *heap;
  int cap, n = 0;
  void take(const Cand &cand) {
    if (n < cap) {
      heap[n++] = cand;
      std::push_heap(heap, heap + n);
    } else if (cand < heap[0]) {
      std::pop_heap(heap, heap + n);
      heap[n - 1] = cand;
      std::push_heap(heap, heap + n);
    }
  }
  bool settled(double lb) const { return n == cap && heap[0].first < lb * lb; }   // nothing lb or more away can enter
};

// the list of one centre; false: a transformed coordinate of the centre is not finite
bool search_one(const Grid &g, const double *tc, int k, double radius, int *out, int *count) {
  Cand heap[GPAK_LOCAL_SEARCH_MAX];
  Best best{heap, k};
  if (!visit_rings(g, tc, radius, [&](double lb) { return best.settled(lb); },
                   [&](double s, int id, int) { best.take(Cand(s, id)); }))
    return false;
  std::sort_heap(heap, heap + best.n);
  for (int q = 0; q < k; q++) out[q] = q < best.n ? heap[q].second : -1;
  *count = best.n;
  return true;
}

// the octant list of one centre: the per_octant nearest of each octant inside the radius, of those the k nearest
bool search_one_octant(const Grid &g, const double *tc, int k, int per_octant, double radius, Cand *work, int *out, int *count) {
  Best oct[8];
  for (int o = 0; o < 8; o++) oct[o] = Best{work + (size_t)o * per_octant, per_octant};
  auto all_settled = [&](double lb) {
    for (int o = 0; o < 8; o++)
      if (!oct[o].settled(lb)) return false;
    return true;
  };
  if (!visit_rings(g, tc, radius, all_settled, [&](double s, int id, int o) { oct[o].take(Cand(s, id)); })) return false;
  int n = 0;   // the octants' candidates side by side, then one sort
  for (int o = 0; o < 8; o++)
    for (int q = 0; q < oct[o].n; q++) work[n++] = oct[o].heap[q];
  std::sort(work, work + n);
  const int keep = std::min(n, k);
  for (int q = 0; q < k; q++) out[q] = q < keep ? work[q].second : -1;
  *count = keep;
  return true;
}

// the checks both searches share; true: refuse
bool bad_arguments(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k, double radius,
                   const int *nbr) {
  if (!Xs || !Xc || !nbr || (d != 3 && d != 4) || k < 1 || k > GPAK_LOCAL_SEARCH_MAX || Ns < 1 || M < 1 || Ns > INT_MAX ||
      std::isnan(radius))
    return true;
  for (size_t i = 0; i < (size_t)Ns * d; i++)
    if (!std::isfinite(Xs[i])) return true;
  for (size_t i = 0; i < (size_t)M * d; i++)
    if (!std::isfinite(Xc[i])) return true;
  for (int i = 0; G && i < d * d; i++)
    if (!std::isfinite(G[i])) return true;
  return false;
}

// both searches: per_octant = 0 is the plain one.  Results go to buffers of the call's own, so that a refusal writes nothing
int search_all(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k, int per_octant, double radius,
               int threads, int *nbr, int *used) {
  Grid g;
  if (!build_grid(Xs, Ns, d, G, g)) return 2;
  int nt = threads;
  if (nt <= 0) nt = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  nt = (int)std::min<long>(std::min(nt, 256), M);   // a caller's number has a ceiling too
  std::vector<int> bad((size_t)nt, 0);
  std::vector<int> lists((size_t)k * M), counts((size_t)M);
  auto slice = [&](int w) {
    const long b0 = M * w / nt, b1 = M * (w + 1) / nt;
    double tc[4];
    std::vector<Cand> work((size_t)8 * per_octant);
    for (long b = b0; b < b1; b++) {
      transform_point(Xc, M, b, d, G, tc);
      const bool fine = per_octant ? search_one_octant(g, tc, k, per_octant, radius, work.data(), &lists[(size_t)k * b], &counts[b])
                                   : search_one(g, tc, k, radius, &lists[(size_t)k * b], &counts[b]);
      if (!fine) { bad[w] = 1; return; }
    }
  };
  if (nt == 1) {
    slice(0);
  } else {
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; w++) pool.emplace_back(slice, w);
    for (auto &th : pool) th.join();
  }
  for (int w = 0; w < nt; w++)
    if (bad[w]) return 2;
  std::copy(lists.begin(), lists.end(), nbr);
  if (used) std::copy(counts.begin(), counts.end(), used);
  return 0;
}

}  // namespace

extern "C" int gpak_local_neighbours(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k,
                                     double radius, int threads, int *nbr, int *used) {
  if (bad_arguments(Xs, Ns, d, Xc, M, G, k, radius, nbr)) return 2;
  return search_all(Xs, Ns, d, Xc, M, G, k, 0, radius, threads, nbr, used);
}

extern "C" int gpak_local_neighbours_octant(const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k,
                                            int per_octant, double radius, int threads, int *nbr, int *used) {
  if (bad_arguments(Xs, Ns, d, Xc, M, G, k, radius, nbr) || !(radius > 0.0) || !std::isfinite(radius) || per_octant < 1 ||
      per_octant > k)
    return 2;
  return search_all(Xs, Ns, d, Xc, M, G, k, per_octant, radius, threads, nbr, used);
}
