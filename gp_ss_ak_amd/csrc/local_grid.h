// local_grid.h -- the uniform cell grid of the neighbour searches: the one place that transforms a point and bins the
// samples.  The host search (local_search.cpp) and the device search (local_search_dev.hip) both include it, so both see
// the same cells filled by the same arithmetic.  Plain C++: no HIP header, nothing else of the library; every function is
// inline.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace gpak_local_grid {

// no fused multiply-add in these functions, so that the bytes are the same in every object: under clang (hipcc contracts
// by default) the pragma sees to it whatever the including file's flags; another compiler is given -ffp-contract=off
#if defined(__clang__)
#define GPAK_GRID_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPAK_GRID_NO_FMA
#endif

// t = x G, the arithmetic local_search.h states (a test restates it in NumPy and expects the same bytes)
inline void transform_point(const double *X, long n, long i, int d, const double *G, double *t) {
  GPAK_GRID_NO_FMA
  if (!G) {
    for (int j = 0; j < d; j++) t[j] = X[i + (size_t)j * n];
    return;
  }
  for (int j = 0; j < d; j++) {
    double s = X[i] * G[(size_t)d * j];
    for (int r = 1; r < d; r++) s = s + X[i + (size_t)r * n] * G[r + (size_t)d * j];
    t[j] = s;
  }
}

// A sample with transformed coordinates t lies in cell a_j = min(max(floor((t_j - lo_j) / h), 0), n_j - 1), j < 3; the cells
// along the third axis are contiguous: cell (a0, a1, a2) has index (a0 n1 + a1) n2 + a2.  scale >= max |lo_j|, |hi_j|.
struct Grid {
  int d = 3;
  double lo[3] = {0, 0, 0}, h = 1.0, scale = 0.0;
  int n[3] = {1, 1, 1};
  std::vector<long> start;     // n0 n1 n2 + 1: the running count over the cells
  std::vector<double> pts;     // the transformed samples in cell order, d per sample
  std::vector<int> ids;        // their indices: ascending inside a cell
  int cell_of(const double *t, int i) const {
    GPAK_GRID_NO_FMA
    const double f = std::floor((t[i] - lo[i]) / h);
    return f <= 0.0 ? 0 : (f >= (double)(n[i] - 1) ? n[i] - 1 : (int)f);
  }
  size_t cell_index(int a0, int a1, int a2) const { return ((size_t)a0 * n[1] + a1) * n[2] + a2; }
};

// false: a transformed coordinate of a sample is not finite
inline bool build_grid(const double *Xs, long Ns, int d, const double *G, Grid &g) {
  GPAK_GRID_NO_FMA
  g.d = d;
  std::vector<double> T((size_t)Ns * d);
  double hi[3] = {0, 0, 0};
  for (long i = 0; i < Ns; i++) {
    double *t = &T[(size_t)i * d];
    transform_point(Xs, Ns, i, d, G, t);
    for (int j = 0; j < d; j++)
      if (!std::isfinite(t[j])) return false;
    for (int j = 0; j < 3; j++) {
      if (i == 0 || t[j] < g.lo[j]) g.lo[j] = t[j];
      if (i == 0 || t[j] > hi[j]) hi[j] = t[j];
    }
  }
  double ext[3], vol = 1.0;
  int m = 0;
  for (int j = 0; j < 3; j++) {
    ext[j] = hi[j] - g.lo[j];
    if (!std::isfinite(ext[j])) return false;
    if (ext[j] > 0.0) { vol *= ext[j]; m++; }
    g.scale = std::max(g.scale, std::max(std::fabs(g.lo[j]), std::fabs(hi[j])));
  }
  // about four samples per cell over the dimensions that have an extent
  const double cells = std::max(1.0, (double)Ns / 4.0);
  g.h = m ? std::pow(vol / cells, 1.0 / m) : 1.0;
  if (!(g.h > 0.0) || !std::isfinite(g.h)) g.h = 1.0;
  // the cells grow until no dimension has more than 4096 of them and the grid no more than about 8 per sample.  No count is
  // ever capped: a sample's cell is floor((t - lo) / h) in every dimension, which the ring bound of the searches relies on
  for (;;) {
    double total = 1.0, most = 1.0;
    for (int j = 0; j < 3; j++) {
      const double c = ext[j] > 0.0 ? std::floor(ext[j] / g.h) + 1.0 : 1.0;
      most = std::max(most, c);
      total *= c;
      g.n[j] = c <= 4096.0 ? (int)c : 4096;
    }
    if (most <= 4096.0 && total <= 8.0 * (double)Ns + 64.0) break;
    g.h *= 1.26;
  }
  const size_t nc = (size_t)g.n[0] * g.n[1] * g.n[2];
  g.start.assign(nc + 1, 0);
  std::vector<size_t> cell((size_t)Ns);
  for (long i = 0; i < Ns; i++) {
    const double *t = &T[(size_t)i * d];
    const size_t c = g.cell_index(g.cell_of(t, 0), g.cell_of(t, 1), g.cell_of(t, 2));
    cell[i] = c;
    g.start[c + 1]++;
  }
  for (size_t c = 0; c < nc; c++) g.start[c + 1] += g.start[c];
  std::vector<long> at(g.start.begin(), g.start.end() - 1);
  g.pts.resize((size_t)Ns * d);
  g.ids.resize((size_t)Ns);
  for (long i = 0; i < Ns; i++) {   // ascending i: a cell's samples stay in index order
    const long p = at[cell[i]]++;
    g.ids[p] = (int)i;
    for (int j = 0; j < d; j++) g.pts[(size_t)p * d + j] = T[(size_t)i * d + j];
  }
  return true;
}

}  // namespace gpak_local_grid
