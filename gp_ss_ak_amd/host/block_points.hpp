// block_points.hpp -- cell-centred discretisation of rectangular blocks for block-support prediction
// (gpak_predict_block).  Plain host code: no device, no context, nothing but the standard library.
#pragma once
#include <cstddef>
#include <vector>

// centres: M x d column-major (d = 3 or 4; columns x, y, z and an optional fourth that is copied to every point).
// size = the block's edge lengths (dx, dy, dz), disc = points per axis (nx, ny, nz), each >= 1.
// Xd becomes (M * nd) x d column-major, nd = nx * ny * nz: row b * nd + a is point a = (i * ny + j) * nz + k of block b
// (x slowest, z fastest) at centre + (((i + 0.5) / nx - 0.5) dx, ((j + 0.5) / ny - 0.5) dy, ((k + 0.5) / nz - 0.5) dz).
// Returns nd, or 0 for arguments it cannot use.
inline int gpak_block_points(const double *centres, size_t M, size_t d, const double size[3], const int disc[3],
                             std::vector<double> &Xd) {
  if (!centres || d < 3 || disc[0] < 1 || disc[1] < 1 || disc[2] < 1) return 0;
  std::vector<double> off[3];
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < disc[k]; i++) off[k].push_back(((i + 0.5) / disc[k] - 0.5) * size[k]);
  const size_t nd = (size_t)disc[0] * disc[1] * disc[2], rows = M * nd;
  Xd.assign(rows * d, 0.0);
  for (size_t b = 0; b < M; b++) {
    size_t r = b * nd;
    for (int i = 0; i < disc[0]; i++)
      for (int j = 0; j < disc[1]; j++)
        for (int k = 0; k < disc[2]; k++, r++) {
          Xd[r] = centres[b] + off[0][i];
          Xd[r + rows] = centres[b + M] + off[1][j];
          Xd[r + 2 * rows] = centres[b + 2 * M] + off[2][k];
          for (size_t c = 3; c < d; c++) Xd[r + c * rows] = centres[b + c * M];
        }
  }
  return (int)nd;
}
