// Prints gpak_sim_normals (gp_ss_ak_amd/host/sim_normals.hpp) at full precision, one value per line.  Built by
// tests/test_joint.py with plain g++ and only that header's directory on the include path: the generator of the `sim`
// verb needs neither the device library nor a context.
//   sim_normals_driver seed n
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim_normals.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<double> z;
  gpak_sim_normals((std::uint64_t)strtoull(argv[1], nullptr, 10), (std::size_t)atol(argv[2]), z);
  for (double v : z) printf("%.17g\n", v);
  return 0;
}
