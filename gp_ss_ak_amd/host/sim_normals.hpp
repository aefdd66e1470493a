// sim_normals.hpp -- the standard normals of the `sim` verb (gpak_sample_joint takes them from its caller).
// Plain host code: no device, no context.  std::mt19937_64 is specified bit for bit by the standard; the transform is
// Box-Muller written out here and NOT std::normal_distribution, whose algorithm is the library's choice: one seed gives
// one file whatever the standard library.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <random>
#include <vector>

// out[0 .. n): pairs (r cos t, r sin t), r = sqrt(-2 ln u1), t = 2 pi u2, with u = (the top 53 bits of a draw + 0.5) / 2^53
// in (0, 1): the logarithm never sees 0.  An odd n drops the sine of the last pair.
inline void gpak_sim_normals(std::uint64_t seed, std::size_t n, std::vector<double> &out) {
  std::mt19937_64 gen(seed);
  out.resize(n);
  const double scale = 1.0 / 9007199254740992.0, two_pi = 6.283185307179586476925286766559;
  for (std::size_t i = 0; i < n; i += 2) {
    const double u1 = ((double)(gen() >> 11) + 0.5) * scale, u2 = ((double)(gen() >> 11) + 0.5) * scale;
    const double r = std::sqrt(-2.0 * std::log(u1)), t = two_pi * u2;
    out[i] = r * std::cos(t);
    if (i + 1 < n) out[i + 1] = r * std::sin(t);
  }
}
