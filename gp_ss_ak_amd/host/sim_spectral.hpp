// sim_spectral.hpp -- the frequencies of the spectral prior sampler (gpak_sample_path takes them from its caller) and the
// one stream of normals `sim --method path` draws everything from.  Plain host code: no device, no context.
//
// A stationary term of the composition is k(h) = var2 * profile(|h A|^2); in the term's transformed coordinates u = x A it
// is isotropic, and by Bochner's theorem k(h) / var2 = E cos(omega . u(h)) for omega drawn from its spectral measure:
//   profile exp(-sqrt(D2))       (ExpAns, Exp): the multivariate Cauchy -- omega = g / |e|, g in R^dim and e in R standard
//                                normals -- whose characteristic function is exp(-|h|);
//   profile exp(-0.5 iw D2)      (RBF): omega = sqrt(iw) g.
// dim = the input columns (3 or 4).  With F frequencies per term the covariance of the draw is the prior's to
// O(1 / sqrt(F)): |K^(h) - k(h)| <= 5 var2 / sqrt(F) at 200 lags with probability 1 - 4e-4 (Hoeffding).
//
// One seed gives one stream, consumed in this order: the frequencies term by term (per feature g[0 .. dim), then e for the
// Cauchy), ab (column by column), b0, E (column by column), the node noise (column by column).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <random>
#include <vector>

// The sequence of gpak_sim_normals (sim_normals.hpp) for the same seed, one value at a time: the cosine of a Box-Muller
// pair, then its sine.
class GpakNormalStream {
 public:
  explicit GpakNormalStream(std::uint64_t seed) : gen_(seed) {}
  double next() {
    if (have_) { have_ = false; return held_; }
    const double scale = 1.0 / 9007199254740992.0, two_pi = 6.283185307179586476925286766559;
    const double u1 = ((double)(gen_() >> 11) + 0.5) * scale, u2 = ((double)(gen_() >> 11) + 0.5) * scale;
    const double r = std::sqrt(-2.0 * std::log(u1)), t = two_pi * u2;
    held_ = r * std::sin(t);
    have_ = true;
    return r * std::cos(t);
  }
  void fill(double *out, std::size_t n, double scale = 1.0) { for (std::size_t i = 0; i < n; i++) out[i] = scale * next(); }

 private:
  std::mt19937_64 gen_;
  double held_ = 0.0;
  bool have_ = false;
};

#define GPAK_SPECTRAL_EXPSQRT 0   // exp(-sqrt(D2)): ExpAns, Exp
#define GPAK_SPECTRAL_RBF 1       // exp(-0.5 iw D2)
struct GpakSpectralTerm {
  int profile;
  double iw;   // RBF only
};

// F frequencies for each term, term by term: feat_term[f] = the term of feature f, omega[4 f .. 4 f + 3] its frequency
// (omega[4 f + 3] = 0 for dim = 3)
inline void gpak_spectral_frequencies(GpakNormalStream &z, const std::vector<GpakSpectralTerm> &terms, int F, int dim,
                                      std::vector<int> &feat_term, std::vector<double> &omega) {
  feat_term.clear();
  omega.clear();
  for (std::size_t t = 0; t < terms.size(); t++)
    for (int f = 0; f < F; f++) {
      double g[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < dim; k++) g[k] = z.next();
      const double s = terms[t].profile == GPAK_SPECTRAL_RBF ? std::sqrt(terms[t].iw) : 1.0 / std::fabs(z.next());
      feat_term.push_back((int)t);
      for (int k = 0; k < 4; k++) omega.push_back(s * g[k]);
    }
}
