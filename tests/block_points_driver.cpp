// Prints gpak_block_points (gp_ss_ak_amd/host/block_points.hpp) for centres read from stdin, at full precision.  Built by
// tests/test_block.py with plain g++ and only that header's directory on the include path: the discretisation needs
// neither the device library nor a context.
//   block_points_driver M d dx dy dz nx ny nz  < M*d centre values, row by row
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "block_points.hpp"

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  const size_t M = (size_t)atol(argv[1]), d = (size_t)atol(argv[2]);
  const double size[3] = {atof(argv[3]), atof(argv[4]), atof(argv[5])};
  const int disc[3] = {atoi(argv[6]), atoi(argv[7]), atoi(argv[8])};
  std::vector<double> c(M * d), Xd;
  for (size_t b = 0; b < M; b++)
    for (size_t k = 0; k < d; k++)
      if (scanf("%lf", &c[b + k * M]) != 1) return 3;
  const int nd = gpak_block_points(c.data(), M, d, size, disc, Xd);
  if (nd <= 0) return 4;
  const size_t rows = M * (size_t)nd;
  printf("%d\n", nd);
  for (size_t r = 0; r < rows; r++) {
    for (size_t k = 0; k < d; k++) printf("%.17g%c", Xd[r + k * rows], k + 1 < d ? ' ' : '\n');
  }
  return 0;
}
