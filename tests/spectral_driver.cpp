// TEST INFRASTRUCTURE: gp_ss_ak_amd/host/sim_spectral.hpp compiled alone (plain host code, no device).
//   spectral_driver freq SEED F DIM PROFILE IW   -> F lines "term w0 w1 w2 w3" of one term of that profile
//   spectral_driver stream SEED N                -> N values of GpakNormalStream, then N of gpak_sim_normals
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sim_normals.hpp"
#include "sim_spectral.hpp"

int main(int argc, char **argv) {
  if (argc == 7 && !strcmp(argv[1], "freq")) {
    GpakNormalStream z(strtoull(argv[2], nullptr, 10));
    const int F = atoi(argv[3]), dim = atoi(argv[4]);
    std::vector<GpakSpectralTerm> terms(1, GpakSpectralTerm{atoi(argv[5]), atof(argv[6])});
    std::vector<int> ft;
    std::vector<double> om;
    gpak_spectral_frequencies(z, terms, F, dim, ft, om);
    for (size_t f = 0; f < ft.size(); f++)
      printf("%d %.17g %.17g %.17g %.17g\n", ft[f], om[4 * f], om[4 * f + 1], om[4 * f + 2], om[4 * f + 3]);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "stream")) {
    const size_t n = strtoull(argv[3], nullptr, 10);
    GpakNormalStream z(strtoull(argv[2], nullptr, 10));
    for (size_t i = 0; i < n; i++) printf("%.17g\n", z.next());
    std::vector<double> v;
    gpak_sim_normals(strtoull(argv[2], nullptr, 10), n, v);
    for (size_t i = 0; i < n; i++) printf("%.17g\n", v[i]);
    return 0;
  }
  return 2;
}
