// Stand-alone driver of gpak_local_neighbours_octant (gp_ss_ak_amd/csrc/local_search.cpp) for sanitizer builds:
// tests/test_local_ok.py compiles the two files with g++ under -fsanitize=address,undefined and under -fsanitize=thread and
// runs the program as it is.  It holds the octant search to a full sort on a regular lattice (zero differences and equal
// distances everywhere) and on duplicated samples with four columns, with one and with four threads, checks that
// per_octant = k gives the plain search's lists and that refusals write nothing; exit status 0 = everything as expected.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "../gp_ss_ak_amd/csrc/local_search.h"

static int check(const char *name, const std::vector<double> &Xs, long Ns, int d, const std::vector<double> &Xc, long M, int k,
                 int per, double radius) {
  std::vector<int> want((size_t)k * M, -1), count(M, 0);
  for (long b = 0; b < M; b++) {
    std::vector<std::pair<double, int>> oct[8], all;
    for (long i = 0; i < Ns; i++) {
      double e = Xs[i] - Xc[b];
      int o = e < 0.0 ? 1 : 0;
      double s = e * e;
      for (int j = 1; j < d; j++) {
        e = Xs[i + j * Ns] - Xc[b + j * M];
        if (j < 3 && e < 0.0) o |= 1 << j;
        s = s + e * e;
      }
      if (!(s <= radius * radius)) continue;
      oct[o].emplace_back(s, (int)i);
    }
    for (auto &v : oct) {
      std::sort(v.begin(), v.end());
      for (size_t q = 0; q < v.size() && q < (size_t)per; q++) all.push_back(v[q]);
    }
    std::sort(all.begin(), all.end());
    count[b] = (int)std::min<size_t>(k, all.size());
    for (int q = 0; q < count[b]; q++) want[q + (size_t)k * b] = all[q].second;
  }
  int bad = 0;
  for (int threads : {1, 4}) {
    std::vector<int> nbr((size_t)k * M, -7), used(M, -7);
    if (gpak_local_neighbours_octant(Xs.data(), Ns, d, Xc.data(), M, nullptr, k, per, radius, threads, nbr.data(), used.data()) != 0) {
      printf("%s threads=%d: refused\n", name, threads);
      return 1;
    }
    if (nbr != want || used != count) {
      printf("%s threads=%d: lists differ from the full sort\n", name, threads);
      bad = 1;
    }
    if (per == k) {
      std::vector<int> plain((size_t)k * M, -7), pused(M, -7);
      if (gpak_local_neighbours(Xs.data(), Ns, d, Xc.data(), M, nullptr, k, radius, threads, plain.data(), pused.data()) != 0 ||
          plain != nbr || pused != used) {
        printf("%s threads=%d: per_octant = k differs from the plain search\n", name, threads);
        bad = 1;
      }
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
    Xc[M - 1] = 1e300; Xc[M - 2] = -1e300; Xc[2 * M - 3] = 3e9;   // centres far outside the samples' box: empty lists
    bad |= check("lattice k=17 per=3", Xs, Ns, 3, Xc, M, 17, 3, 2.5);
    bad |= check("lattice k=128 per=16", Xs, Ns, 3, Xc, M, 128, 16, 3.5);
    bad |= check("lattice k=8 per=1", Xs, Ns, 3, Xc, M, 8, 1, 1.5);
    bad |= check("lattice k=24 per=24", Xs, Ns, 3, Xc, M, 24, 24, 2.0);
    // refusals write nothing
    std::vector<int> nbr(8 * M, -7), used(M, -7);
    const int rcs[] = {
        gpak_local_neighbours_octant(Xs.data(), Ns, 3, Xc.data(), M, nullptr, 8, 2, 0.0, 1, nbr.data(), used.data()),
        gpak_local_neighbours_octant(Xs.data(), Ns, 3, Xc.data(), M, nullptr, 8, 2, -1.0, 1, nbr.data(), used.data()),
        gpak_local_neighbours_octant(Xs.data(), Ns, 3, Xc.data(), M, nullptr, 8, 0, 1.0, 1, nbr.data(), used.data()),
        gpak_local_neighbours_octant(Xs.data(), Ns, 3, Xc.data(), M, nullptr, 8, 9, 1.0, 1, nbr.data(), used.data()),
        gpak_local_neighbours_octant(nullptr, Ns, 3, Xc.data(), M, nullptr, 8, 2, 1.0, 1, nbr.data(), used.data())};
    for (int rc : rcs)
      if (rc != 2) { printf("a refusal returned %d\n", rc); bad = 1; }
    for (int v : nbr) if (v != -7) { printf("a refusal wrote a list\n"); bad = 1; break; }
    for (int v : used) if (v != -7) { printf("a refusal wrote a count\n"); bad = 1; break; }
  }
  {   // every sample three times, four columns
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
    bad |= check("duplicates k=128 per=128", Xs, Ns, 4, Xc, M, 128, 128, 5.0);
    bad |= check("duplicates k=12 per=2", Xs, Ns, 4, Xc, M, 12, 2, 1.2);
  }
  if (!bad) printf("ok\n");
  return bad;
}
