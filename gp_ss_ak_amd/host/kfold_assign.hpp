// kfold_assign.hpp -- the fold of each sample for `cv --kfold K [--seed n]`.
// Plain host code: no device, no context.  std::mt19937_64 is specified bit for bit by the standard; the shuffle is a
// Fisher-Yates loop written out here and NOT std::shuffle, whose use of the generator is the library's choice: one seed
// gives one assignment whatever the standard library (as sim_normals.hpp writes out its normals).
#pragma once
#include <cstddef>
#include <cstdint>
#include <random>
#include <utility>
#include <vector>

// fold[i] = (the position of sample i in a permutation of 0 .. n - 1) mod K, so the K folds differ in size by at most one.
// The permutation: the identity shuffled from the back, for i = n - 1 .. 1 swap entries i and gen() mod (i + 1).
inline void gpak_kfold_assign(std::uint64_t seed, std::size_t n, int K, std::vector<int> &fold) {
  std::mt19937_64 gen(seed);
  std::vector<std::size_t> perm(n);
  for (std::size_t i = 0; i < n; i++) perm[i] = i;
  for (std::size_t i = n; i-- > 1;) std::swap(perm[i], perm[(std::size_t)(gen() % (std::uint64_t)(i + 1))]);
  fold.resize(n);
  for (std::size_t pos = 0; pos < n; pos++) fold[perm[pos]] = (int)(pos % (std::size_t)K);
}
