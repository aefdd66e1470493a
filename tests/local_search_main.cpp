// Stand-alone driver of gpak_local_neighbours (gp_ss_ak_amd/csrc/local_search.cpp) for sanitizer builds: tests/test_local.py
// compiles the two files with g++ under -fsanitize=address,undefined and under -fsanitize=thread and runs the program as it
// is.  It holds the search to a full sort on a regular lattice (ties everywhere) and on duplicated samples, with one and
// with four threads; exit status 0 = every list equal.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "../gp_ss_ak_amd/csrc/local_search.h"

static int check(const char *name, const std::vector<double> &Xs, long Ns, int d, const std::vector<double> &Xc, long M, int k,
                 double radius) {
  std::vector<int> want((size_t)k * M, -1), count(M, 0);
  for (long b = 0; b < M; b++) {
    std::vector<std::pair<double, int>> all;
    for (long i = 0; i < Ns; i++) {
      double e = Xs[i] - Xc[b];
      double s = e * e;
      for (int j = 1; j < d; j++) { e = Xs[i + j * Ns] - Xc[b + j * M]; s = s + e * e; }
      if (radius > 0.0 && !(s <= radius * radius)) continue;
      all.emplace_back(s, (int)i);
    }
    std::sort(all.begin(), all.end());
    count[b] = (int)std::min<size_t>(k, all.size());
    for (int q = 0; q < count[b]; q++) want[q + (size_t)k * b] = all[q].second;
  }
  int bad = 0;
  for (int threads : {1, 4}) {
    std::vector<int> nbr((size_t)k * M, -7), used(M, -7);
    if (gpak_local_neighbours(Xs.data(), Ns, d, Xc.data(), M, nullptr, k, radius, threads, nbr.data(), used.data()) != 0) {
      printf("%s threads=%d: refused\n", name, threads);
      return 1;
    }
    if (nbr != want || used != count) {
      printf("%s threads=%d: lists differ from the full sort\n", name, threads);
      bad = 1;
    }
  }
  return bad;
}

int main() {
  int bad = 0;
  {   // lattice 6 x 6 x 6, centres on the lattice points and between them
    const int n = 6;
    const long Ns = n * n * n;
    std::vector<double> Xs(3 * Ns);
    for (long i = 0; i < Ns; i++) { Xs[i] = (double)(i / (n * n)); Xs[i + Ns] = (double)((i / n) % n); Xs[i + 2 * Ns] = (double)(i % n); }
    const long M = 2 * Ns;
    std::vector<double> Xc(3 * M);
    for (long b = 0; b < M; b++)
      for (int j = 0; j < 3; j++) Xc[b + j * M] = Xs[b % Ns + j * Ns] + (b < Ns ? 0.0 : 0.5);
    Xc[M - 1] = 1e300; Xc[M - 2] = -1e300; Xc[2 * M - 3] = 3e9;   // centres far outside the samples' box
    bad |= check("lattice k=17", Xs, Ns, 3, Xc, M, 17, 0.0);
    bad |= check("lattice k=128 radius", Xs, Ns, 3, Xc, M, 128, 1.5);
  }
  {   // every sample three times, four columns, more neighbours asked for than there are samples
    const long base = 30, Ns = 3 * base;
    std::vector<double> Xs(4 * Ns);
    for (long i = 0; i < Ns; i++) {
      const long r = i % base;
      Xs[i] = 0.37 * (double)(r % 5); Xs[i + Ns] = 0.11 * (double)(r / 5); Xs[i + 2 * Ns] = 0.05 * (double)r; Xs[i + 3 * Ns] = (double)(r % 2);
    }
    const long M = 40;
    std::vector<double> Xc(4 * M);
    for (long b = 0; b < M; b++)
      for (int j = 0; j < 4; j++) Xc[b + j * M] = b < base ? Xs[b + j * Ns] : 0.01 * (double)(b * (j + 1));
    bad |= check("duplicates k=128", Xs, Ns, 4, Xc, M, 128, 0.0);
    bad |= check("duplicates k=1", Xs, Ns, 4, Xc, M, 1, 0.0);
  }
  if (!bad) printf("ok\n");
  return bad;
}
