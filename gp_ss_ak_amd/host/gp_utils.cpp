// gp_utils.cpp -- see gp_utils.hpp.
#include "gp_utils.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../include/gpak.h"
#include "sim_spectral.hpp"

int GP_utils::default_precision = GPAK_F64;
int GP_utils::default_gpus = 1;
bool GP_utils::exact_gradient = false;
bool GP_utils::loo_objective = false;
std::vector<int> GP_utils::group_labels;
bool GP_utils::fold_objective = false;
int GP_utils::group_count = 0;

void GP_utils::create_ctx() {
  int rc;
  if (default_gpus > 1) rc = gpak_create_multi(&ctx, default_gpus, nullptr, default_precision);
  else rc = gpak_create(&ctx, getenv("GPAK_DEVICE") ? atoi(getenv("GPAK_DEVICE")) : 0, default_precision);
  if (rc != GPAK_OK) gpak_host_fatal(default_gpus > 1 ? "gpak_create_multi" : "gpak_create", nullptr);
}

std::string GP_utils::timingJson() const {
  gpak_phase_times t;
  if (gpak_timing(ctx, &t) != GPAK_OK) return "{}";
  char buf[1024];
  snprintf(buf, sizeof buf,
           "{\"n\": %d, \"n_padded\": %d, \"evaluations\": %d, \"last\": {\"gram_ms\": %.6g, \"factor_ms\": %.6g, "
           "\"solve_ms\": %.6g, \"nlz_ms\": %.6g, \"kmatvec_ms\": %.6g, \"predict_ms\": %.6g, \"grad_ms\": %.6g}, "
           "\"accumulated\": {\"gram_ms\": %.6g, \"factor_ms\": %.6g, \"solve_ms\": %.6g, \"nlz_ms\": %.6g}, "
           "\"precision\": \"%s\", \"gpus\": %d}",
           t.n, t.n_padded, t.evaluations, t.gram_ms, t.factor_ms, t.solve_ms, t.nlz_ms, t.kmatvec_ms, t.predict_ms,
           t.grad_ms, t.accumulated_ms[0], t.accumulated_ms[1], t.accumulated_ms[2], t.accumulated_ms[3],
           default_precision == GPAK_F32 ? "f32" : "f64", default_gpus);
  return buf;
}

GP_utils::GP_utils() { create_ctx(); }

GP_utils::GP_utils(Kernels *kernel, mat Xin, mat Yin, int, int likeLtype, int, unsigned int numhyper,
                   unsigned int numlik_par, unsigned int numMF_par, int verbos)
    : Xinp(Xin), yTarg(Yin), KerenlW(kernel) {
  create_ctx();
  setNumMFpar(numMF_par);
  setNumlikfpar(numlik_par);
  setNumCovpar(numhyper);
  setLikelihoodType(likeLtype);
  setVerbose(verbos);
  setOutDim((unsigned)yTarg.n_cols);
  setInpDim((unsigned)Xin.n_cols);
  setNumData((unsigned)yTarg.n_rows);
  if (numlik_par > 0) {
    hyperlf.resize(numlik_par, 1);
    for (unsigned i = 0; i < numlik_par; i++) hyperlf(i) = 0.016;  // GP_Utils.cpp:43
  }
  initialize_vars();
}

GP_utils::~GP_utils() {
  if (ctx) gpak_destroy(ctx);
  if (owns_kernel) delete KerenlW;
}

void GP_utils::initialize_vars() {
  if (Xinp.n_rows == 0) return;
  if (gpak_set_train(ctx, Xinp.memptr(), yTarg.memptr(), (int)Xinp.n_rows, (int)Xinp.n_cols) != GPAK_OK)
    gpak_host_fatal("gpak_set_train", ctx);
  dirty = true;
}

unsigned int GP_utils::getNumPars() const { return KerenlW->getNPars() + getNumMFpar() + getNumlikfpar(); }

void GP_utils::get_GP_Pars(mat &param) const {  // GP_Utils.cpp:101-128
  unsigned c = 0;
  for (unsigned i = 0; i < KerenlW->getNPars(); i++) param(c++) = KerenlW->getParam(i);
  for (unsigned i = 0; i < getNumlikfpar(); i++) param(c++) = hyperlf(i);
}

void GP_utils::set_GP_Pars(mat &param) const {  // GP_Utils.cpp:130-157: always invalidates
  dirty = true;
  unsigned c = 0;
  for (unsigned i = 0; i < KerenlW->getNPars(); i++) KerenlW->setParam(param(c++), i);
  for (unsigned i = 0; i < getNumlikfpar(); i++) hyperlf(i) = param(c++);
}

void GP_utils::sync_params() const {
  if (!dirty) return;
  double e[8], bias, white;
  if (gpak_extract_expans_bias(KerenlW, e, &bias)) {
    if (gpak_set_params(ctx, e, bias, hyperlf(0), gpak_host_dist_mode()) != GPAK_OK) gpak_host_fatal("gpak_set_params", ctx);
  } else {
    std::vector<int> kinds;
    std::vector<double> pars;
    if (!gpak_extract_composition(KerenlW, kinds, pars, &bias, &white) || kinds.empty()) {
      std::cerr << "GP_utils: this kernel composition is not on the HIP path." << std::endl;
      exit(1);
    }
    if (gpak_set_kernel(ctx, (int)kinds.size(), kinds.data(), pars.data(), bias, white, hyperlf(0), gpak_host_dist_mode()) != GPAK_OK)
      gpak_host_fatal("gpak_set_kernel", ctx);
  }
  dirty = false;
}

void GP_utils::updateKernel() const { sync_params(); }

double GP_utils::logLikelihood() const {
  sync_params();
  double nlz = std::numeric_limits<double>::quiet_NaN();
  int rc = gpak_nlz(ctx, &nlz);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_nlz", ctx);
  return nlz;
}

double GP_utils::LooObjective() const {
  sync_params();
  gpak_loo_summary s;
  int rc = gpak_loo(ctx, nullptr, nullptr, &s);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_loo", ctx);
  return -s.log_pl;   // NaN on Chol_fail
}

double GP_utils::GroupObjective() const {
  sync_params();
  if (group_labels.size() != Xinp.n_rows) { std::cerr << "GroupObjective: one label per training sample is needed." << std::endl; exit(1); }
  gpak_cv_groups_summary s;
  int rc = fold_objective ? gpak_cv_folds(ctx, group_labels.data(), group_count, nullptr, nullptr, nullptr, &s, 0)
                          : gpak_cv_groups(ctx, group_labels.data(), group_count, nullptr, nullptr, nullptr, &s);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal(fold_objective ? "gpak_cv_folds" : "gpak_cv_groups", ctx);
  return -s.log_pl;   // NaN on Chol_fail
}

double GP_utils::GradLL(mat &g) const {  // GP_Utils.cpp:1171-1262
  double nlz = std::numeric_limits<double>::quiet_NaN();
  const bool group_objective = !group_labels.empty();
  if (!loo_objective && !group_objective) {
    nlz = logLikelihood();
    if (Chol_fail) return std::numeric_limits<double>::quiet_NaN();
  }
  // one device call evaluates GradLL + every child's getGradients; the result comes back as the
  // stationary children's blocks in order, then the Bias entry, then the likelihood entry
  std::vector<const Kernels *> leaves;
  if (const HybKerns *h = dynamic_cast<const HybKerns *>(KerenlW)) {
    for (unsigned i = 0; i < h->getNumKerns(); i++) leaves.push_back(h->getKern(i));
  } else {
    leaves.push_back(KerenlW);
  }
  int ng = 2;
  for (const Kernels *c : leaves) {
    if (dynamic_cast<const Kern_Bias *>(c)) continue;
    if (dynamic_cast<const Kern_White *>(c)) {
      // upstream, Kern_White inherits a getGradients that calls itself (Kernel.h:56-60, 257-283)
      std::cerr << "GradLL: a White child has no gradient (the reference recurses without end here)." << std::endl;
      exit(1);
    }
    ng += (int)c->getNPars();
  }
  std::vector<double> gd(ng);
  if (group_objective) {
    sync_params();
    if (group_labels.size() != Xinp.n_rows) { std::cerr << "GradLL: one label per training sample is needed." << std::endl; exit(1); }
    gpak_cv_groups_summary s;
    int rc = fold_objective ? gpak_cv_folds_grad(ctx, group_labels.data(), group_count, gd.data(), ng, &s, 0)
                            : gpak_cv_groups_grad(ctx, group_labels.data(), group_count, gd.data(), ng, &s);
    Chol_fail = (rc == GPAK_ENOTPD);
    if (Chol_fail) return std::numeric_limits<double>::quiet_NaN();
    if (rc != GPAK_OK) gpak_host_fatal(fold_objective ? "gpak_cv_folds_grad" : "gpak_cv_groups_grad", ctx);
    nlz = -s.log_pl;
  } else if (loo_objective) {
    sync_params();
    gpak_loo_summary s;
    int rc = gpak_loo_grad(ctx, gd.data(), ng, &s);
    Chol_fail = (rc == GPAK_ENOTPD);
    if (Chol_fail) return std::numeric_limits<double>::quiet_NaN();
    if (rc != GPAK_OK) gpak_host_fatal("gpak_loo_grad", ctx);
    nlz = -s.log_pl;
  } else if (exact_gradient) {
    if (gpak_grad_exact(ctx, gd.data(), ng) != GPAK_OK) gpak_host_fatal("gpak_grad_exact", ctx);
  } else if (gpak_grad_hyb(ctx, gd.data(), ng) != GPAK_OK) gpak_host_fatal("gpak_grad_hyb", ctx);
  unsigned out = 0;
  int in = 0;
  for (const Kernels *c : leaves) {
    if (dynamic_cast<const Kern_Bias *>(c)) { g(out++) = gd[ng - 2]; continue; }
    for (unsigned i = 0; i < c->getNPars(); i++) g(out++) = gd[in++];
  }
  g(out) = gd[ng - 1];
  return nlz;
}

void GP_utils::posteriorMeanVar(mat &mu, mat &varSigma, const mat &Xin) const {
  logLikelihood();
  if (Chol_fail) { mu.fill(std::numeric_limits<double>::quiet_NaN()); varSigma.fill(std::numeric_limits<double>::quiet_NaN()); return; }
  if (mu.n_elem != Xin.n_rows) mu.resize(Xin.n_rows, 1);
  if (varSigma.n_elem != Xin.n_rows) varSigma.resize(Xin.n_rows, 1);
  if (gpak_predict(ctx, Xin.memptr(), (long)Xin.n_rows, (int)Xin.n_cols, mu.memptr(), varSigma.memptr(), compat) != GPAK_OK)
    gpak_host_fatal("gpak_predict", ctx);
}

void GP_utils::LooCV(mat &mean, mat &var, gpak_loo_summary &s) const {
  sync_params();
  if (mean.n_elem != Xinp.n_rows) mean.resize(Xinp.n_rows, 1);
  if (var.n_elem != Xinp.n_rows) var.resize(Xinp.n_rows, 1);
  int rc = gpak_loo(ctx, mean.memptr(), var.memptr(), &s);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_loo", ctx);
}

void GP_utils::GroupCV(const std::vector<int> &group, int n_groups, mat &mean, mat &var, mat &logp,
                       gpak_cv_groups_summary &s) const {
  sync_params();
  if (group.size() != Xinp.n_rows) { std::cerr << "GroupCV: one label per training sample is needed." << std::endl; exit(1); }
  if (mean.n_elem != Xinp.n_rows) mean.resize(Xinp.n_rows, 1);
  if (var.n_elem != Xinp.n_rows) var.resize(Xinp.n_rows, 1);
  if (n_groups > 0 && logp.n_elem != (size_t)n_groups) logp.resize(n_groups, 1);
  int rc = gpak_cv_groups(ctx, group.data(), n_groups, mean.memptr(), var.memptr(), logp.memptr(), &s);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_cv_groups", ctx);
}

void GP_utils::FoldCV(const std::vector<int> &group, int n_groups, mat &mean, mat &var, mat &logp,
                      gpak_cv_groups_summary &s) const {
  sync_params();
  if (group.size() != Xinp.n_rows) { std::cerr << "FoldCV: one label per training sample is needed." << std::endl; exit(1); }
  if (mean.n_elem != Xinp.n_rows) mean.resize(Xinp.n_rows, 1);
  if (var.n_elem != Xinp.n_rows) var.resize(Xinp.n_rows, 1);
  if (n_groups > 0 && logp.n_elem != (size_t)n_groups) logp.resize(n_groups, 1);
  int rc = gpak_cv_folds(ctx, group.data(), n_groups, mean.memptr(), var.memptr(), logp.memptr(), &s, 0);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_cv_folds", ctx);
}

void GP_utils::BlockMeanVar(mat &mean, mat &var, const mat &Xd, int nd, bool latent) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (var.n_elem != M) var.resize(M, 1);
  int rc = gpak_predict_block(ctx, Xd.memptr(), (long)M, nd, (int)Xd.n_cols, mean.memptr(), var.memptr(),
                              latent ? GPAK_BLOCK_LATENT : 0);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_predict_block", ctx);
}

void GP_utils::LocalMetric(double G[16]) const {
  sync_params();
  if (gpak_local_metric(ctx, 0, G) != GPAK_OK) gpak_host_fatal("gpak_local_metric", ctx);
}

void GP_utils::LocalNeighbours(const mat &Xs, const mat &Xc, const double G[16], int k, double radius, std::vector<int> &nbr,
                               std::vector<int> &used) {
  const int d = (int)Xs.n_cols;
  std::vector<double> Gd((size_t)d * d);   // the leading d x d part
  for (int c = 0; c < d; c++)
    for (int r = 0; r < d; r++) Gd[r + (size_t)d * c] = G[r + 4 * c];
  nbr.assign((size_t)k * Xc.n_rows, -1);
  used.assign(Xc.n_rows, 0);
  if (gpak_local_neighbours(Xs.memptr(), (long)Xs.n_rows, d, Xc.memptr(), (long)Xc.n_rows, Gd.data(), k, radius, 0, nbr.data(),
                            used.data()) != GPAK_OK) {
    std::cerr << "gpak_local_neighbours refused the samples or the nodes (a coordinate that is not finite?)" << std::endl;
    exit(1);
  }
}

void GP_utils::LocalNeighboursDev(const mat &Xs, const mat &Xc, const double G[16], int k, double radius, std::vector<int> &nbr,
                                  std::vector<int> &used, gpak_local_search_summary &summary) const {
  const int d = (int)Xs.n_cols;
  std::vector<double> Gd((size_t)d * d);   // the leading d x d part
  for (int c = 0; c < d; c++)
    for (int r = 0; r < d; r++) Gd[r + (size_t)d * c] = G[r + 4 * c];
  nbr.assign((size_t)k * Xc.n_rows, -1);
  used.assign(Xc.n_rows, 0);
  if (gpak_local_neighbours_dev(ctx, Xs.memptr(), (long)Xs.n_rows, d, Xc.memptr(), (long)Xc.n_rows, Gd.data(), k, radius, nbr.data(),
                                used.data(), nullptr, &summary) != GPAK_OK)
    gpak_host_fatal("gpak_local_neighbours_dev", ctx);
}

void GP_utils::LocalMeanVar(mat &mean, mat &var, const mat &Xs, const mat &ys, const mat &Xd, int nd, const std::vector<int> &nbr,
                            int k, bool latent, gpak_local_summary &summary) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (var.n_elem != M) var.resize(M, 1);
  int rc = gpak_predict_local(ctx, Xs.memptr(), ys.memptr(), (long)Xs.n_rows, (int)Xs.n_cols, Xd.memptr(), (long)M, nd, nbr.data(),
                              k, mean.memptr(), var.memptr(), latent ? GPAK_LOCAL_LATENT : 0, &summary);
  if (rc != GPAK_OK) gpak_host_fatal("gpak_predict_local", ctx);
}

void GP_utils::LocalNeighboursOctant(const mat &Xs, const mat &Xc, const double G[16], int k, int per_octant, double radius,
                                     std::vector<int> &nbr, std::vector<int> &used) {
  const int d = (int)Xs.n_cols;
  std::vector<double> Gd((size_t)d * d);   // the leading d x d part
  for (int c = 0; c < d; c++)
    for (int r = 0; r < d; r++) Gd[r + (size_t)d * c] = G[r + 4 * c];
  nbr.assign((size_t)k * Xc.n_rows, -1);
  used.assign(Xc.n_rows, 0);
  if (gpak_local_neighbours_octant(Xs.memptr(), (long)Xs.n_rows, d, Xc.memptr(), (long)Xc.n_rows, Gd.data(), k, per_octant, radius, 0,
                                   nbr.data(), used.data()) != GPAK_OK) {
    std::cerr << "gpak_local_neighbours_octant refused the samples or the nodes (a coordinate that is not finite?)" << std::endl;
    exit(1);
  }
}

void GP_utils::LocalMeanVarOk(mat &mean, mat &var, mat &mu, const mat &Xs, const mat &ys, const mat &Xd, int nd,
                              const std::vector<int> &nbr, int k, bool latent, gpak_local_summary &summary) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (var.n_elem != M) var.resize(M, 1);
  if (mu.n_elem != M) mu.resize(M, 1);
  int rc = gpak_predict_local_ok(ctx, Xs.memptr(), ys.memptr(), (long)Xs.n_rows, (int)Xs.n_cols, Xd.memptr(), (long)M, nd,
                                 nbr.data(), k, mean.memptr(), var.memptr(), mu.memptr(), latent ? GPAK_LOCAL_LATENT : 0, &summary);
  if (rc != GPAK_OK) gpak_host_fatal("gpak_predict_local_ok", ctx);
}

void GP_utils::JointMeanCov(mat &mean, mat &cov, const mat &Xd, int nd, bool latent) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (cov.n_rows != M || cov.n_cols != M) cov.resize(M, M);
  int rc = gpak_predict_joint(ctx, Xd.memptr(), (long)M, nd, (int)Xd.n_cols, mean.memptr(), cov.memptr(),
                              latent ? GPAK_JOINT_LATENT : 0);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_predict_joint", ctx);
}

bool GP_utils::JointSample(mat &Z, mat &mean, const mat &Xd, int nd, const mat &Xi, double nugget, bool latent) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0, S = Xi.n_cols;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (Z.n_rows != M || Z.n_cols != S) Z.resize(M, S);
  int rc = gpak_sample_joint(ctx, Xd.memptr(), (long)M, nd, (int)Xd.n_cols, Xi.memptr(), (int)S, nugget, Z.memptr(),
                             mean.memptr(), latent ? GPAK_JOINT_LATENT : 0);
  Chol_fail = (rc == GPAK_ENOTPD && std::isnan(mean[0]));   // the training factor; otherwise the blocks' covariance
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_sample_joint", ctx);
  return rc == GPAK_OK;
}

bool GP_utils::PathSample(mat &Z, mat &mean, const mat &Xd, int nd, unsigned long long seed, int features, bool latent,
                          gpak_condition_summary &summary) const {
  sync_params();
  const size_t M = nd > 0 ? Xd.n_rows / nd : 0, N = Xinp.n_rows;
  const int S = (int)Z.n_cols, dim = (int)Xd.n_cols;
  if (mean.n_elem != M) mean.resize(M, 1);
  if (Z.n_rows != M) Z.resize(M, S);
  // the stationary terms of the composition in force, as sync_params hands them to the library
  std::vector<int> kinds;
  std::vector<double> pars;
  double e[8], bias = 0.0, white = 0.0;
  if (gpak_extract_expans_bias(KerenlW, e, &bias)) {
    kinds.assign(1, GPAK_KERN_EXPANS);
  } else if (!gpak_extract_composition(KerenlW, kinds, pars, &bias, &white) || kinds.empty()) {
    std::cerr << "GP_utils: this kernel composition is not on the HIP path." << std::endl;
    exit(1);
  }
  std::vector<GpakSpectralTerm> terms;
  size_t off = 0;
  for (int kind : kinds) {
    GpakSpectralTerm t = {kind == GPAK_KERN_RBF ? GPAK_SPECTRAL_RBF : GPAK_SPECTRAL_EXPSQRT, 0.0};
    if (kind == GPAK_KERN_RBF) t.iw = pars[off + 1];
    off += kind == GPAK_KERN_EXPANS ? 8 : kind == GPAK_KERN_EXP ? 2 : 3;
    terms.push_back(t);
  }
  GpakNormalStream z(seed);
  std::vector<int> feat_term;
  std::vector<double> omega;
  gpak_spectral_frequencies(z, terms, features, dim, feat_term, omega);
  const size_t nfeat = feat_term.size();
  std::vector<double> ab(2 * nfeat * (size_t)S), b0((size_t)S), E(N * (size_t)S);
  z.fill(ab.data(), ab.size());
  z.fill(b0.data(), b0.size());
  z.fill(E.data(), E.size());
  int rc = gpak_sample_path(ctx, Xd.memptr(), (long)M, nd, dim, (int)nfeat, feat_term.data(), omega.data(), ab.data(), b0.data(),
                            E.data(), S, Z.memptr(), mean.memptr(), 0, &summary);
  Chol_fail = (rc == GPAK_ENOTPD);
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_sample_path", ctx);
  if (rc == GPAK_OK && !latent) {
    const double sd = std::sqrt((hyperlf(0) + white) / nd);
    for (size_t i = 0; i < M * (size_t)S; i++) Z[i] += sd * z.next();
  }
  return rc == GPAK_OK;
}

bool GP_utils::DesignHoles(const mat &Xd, int nd, const mat &Xc, const std::vector<int> &hole, int H, const double *wt, int k,
                           std::vector<double> &gain, std::vector<int> &picked, std::vector<double> &pick_gain,
                           gpak_design_summary &summary) const {
  sync_params();
  const size_t T = nd > 0 ? Xd.n_rows / nd : 0;
  gain.assign((size_t)H, 0.0);
  picked.assign((size_t)k, -1);
  pick_gain.assign((size_t)k, 0.0);
  int rc = gpak_design(ctx, Xd.memptr(), (long)T, nd, Xc.memptr(), (long)Xc.n_rows, (int)Xd.n_cols, hole.data(), H, wt, k,
                       gain.data(), nullptr, nullptr, picked.data(), pick_gain.data(), nullptr, &summary);
  Chol_fail = (rc == GPAK_ENOTPD && std::isnan(summary.var_before));   // the training factor; otherwise a hole's A_h
  if (rc != GPAK_OK && rc != GPAK_ENOTPD) gpak_host_fatal("gpak_design", ctx);
  return rc == GPAK_OK;
}

void GP_utils::Calc_Out(mat &yPred, mat &yVar, const mat &Xin) const { posteriorMeanVar(yPred, yVar, Xin); }

void GP_utils::OptimisePars(unsigned int iters) {  // GP_Utils.cpp:1288-1301
  if (getVerbose() > 2) { std::cout << "Initial model:" << std::endl; ShowKernelPars(std::cout); }
  // the reference only honours `iters` at verbosity > 2 (the `if` swallowed the call, :1295-1296)
  if (getVerbose() > 2 && getNumPars() < 40) setMaxIters(iters);
  if (getenv("GPAK_MAX_ITERS")) setMaxIters((unsigned)atoi(getenv("GPAK_MAX_ITERS")));
  Optimise();
  if (getVerbose() > 0) ShowKernelPars(std::cout);
}

std::ostream &GP_utils::ShowKernelPars(std::ostream &os) const {  // GP_Utils.cpp:1303-1322
  std::cout << "Standard GP Model: " << std::endl;
  std::cout << "Optimiser: " << getDefaultOptimiserStr() << std::endl;
  std::cout << "Inference: " << getInf() << std::endl;
  std::cout << "Data Set Size: " << getNumData() << std::endl;
  std::cout << "Kernel Type: " << std::endl;
  KerenlW->ShowKernelPars(os);
  for (unsigned i = 0; i < getNumlikfpar(); i++) std::cout << "likelihood hyperparmeters : " << hyperlf(i) << std::endl;
  if (getVerbose()) std::cout << "Log likelihood: " << logLikelihood() << std::endl;
  return os;
}

void GP_utils::ToFile_GP_Params(std::ostream &out) const {  // GP_Utils.cpp:1360-1390
  out << "Inference=" << getInf() << std::endl;
  out << "likelihood=" << getLikelihoodType() << std::endl;
  out << "MeanFunction=" << getMean() << std::endl;
  out << "numData=" << getNumData() << std::endl;
  out << "outputDim=" << getOutDim() << std::endl;
  out << "inputDim=" << getInpDim() << std::endl;
  out << "NumHyperKernel=" << KerenlW->getNPars() << std::endl;
  out << "NumHyperLik=" << getNumlikfpar() << std::endl;
  out << "NumHyperMean=" << getNumMFpar() << std::endl;
  KerenlW->StrmOut(out);
  for (unsigned i = 0; i < getNumlikfpar(); i++) out << "Hyperparams_likelihood=" << hyperlf(i) << std::endl;
}

void GP_utils::FromFile_GP_Params(std::istream &in) {  // GP_Utils.cpp:1324-1358
  setInf(ReadStrStrm(in, "Inference"));
  setLikelihoodType(ReadIntStrm(in, "likelihood"));
  setMean(ReadStrStrm(in, "MeanFunction"));
  setNumData(ReadIntStrm(in, "numData"));
  setOutDim(ReadIntStrm(in, "outputDim"));
  setInpDim(ReadIntStrm(in, "inputDim"));
  setNumCovpar(ReadIntStrm(in, "NumHyperKernel"));
  setNumlikfpar(ReadIntStrm(in, "NumHyperLik"));
  setNumMFpar(ReadIntStrm(in, "NumHyperMean"));
  KerenlW = ReadKerFromFile(in);
  owns_kernel = true;
  if (getNumlikfpar() > 0) {
    hyperlf.resize(getNumlikfpar(), 1);
    for (unsigned i = 0; i < getNumlikfpar(); i++) hyperlf(i) = ReadDoubleStrm(in, "Hyperparams_likelihood");
  }
  dirty = true;
}

void writeGPFile(const GP_utils &model, const std::string &modelFileName, const std::string &comment) {
  model.WFile(modelFileName, comment);
}

GP_utils *readGpFromFile(const std::string &modelFileName, int verbosity) {
  if (verbosity > 0) std::cout << "Loading model file." << std::endl;
  std::ifstream in(modelFileName.c_str());
  if (!in.is_open()) { std::cout << "Error in reading file name. \n"; exit(1); }
  GP_utils *m = new GP_utils();
  // skip the comment line, then the key=value body
  m->StrmIn(in);
  if (verbosity > 0) std::cout << "Model Info has been read.\n";
  m->setVerbose(verbosity);
  return m;
}

// ---------------------------------------------------------------------------------------------
// A plain projected L-BFGS with backtracking (NOT the reference's algorithm; opt_algs.cpp holds
// the restatement of Opt_pars.cpp).  Kept as an alternative driver: GPAK_OPT=simple.
// ---------------------------------------------------------------------------------------------
void Opt_Algs::SimpleLBFGSOptimise() {
  const unsigned n = getNumPars();
  const double lb = 1e-4, ub = 6.0;  // Opt_pars.cpp:184-188
  const unsigned mem = 6;
  mat x(1, n), g(1, n), xn(1, n), gn(1, n);
  get_GP_Pars(x);
  for (unsigned i = 0; i < n; i++) x(i) = std::min(ub, std::max(lb, x(i)));
  set_GP_Pars(x);
  double fx = Grad_Values(g);
  numFuncEval++;
  std::vector<std::vector<double>> S, Y;
  std::vector<double> rho;
  for (unsigned iter = 1; iter <= getMaxIters(); iter++) {
    // two-loop recursion on the free variables
    std::vector<double> d(n), q(n), al(S.size());
    for (unsigned i = 0; i < n; i++) q[i] = g(i);
    for (int k = (int)S.size() - 1; k >= 0; k--) {
      double a = 0; for (unsigned i = 0; i < n; i++) a += S[k][i] * q[i];
      al[k] = a * rho[k];
      for (unsigned i = 0; i < n; i++) q[i] -= al[k] * Y[k][i];
    }
    double gam = 1.0;
    if (!S.empty()) {
      double sy = 0, yy = 0;
      for (unsigned i = 0; i < n; i++) { sy += S.back()[i] * Y.back()[i]; yy += Y.back()[i] * Y.back()[i]; }
      if (yy > 0) gam = sy / yy;
    } else {
      double gn2 = 0; for (unsigned i = 0; i < n; i++) gn2 += g(i) * g(i);
      gam = gn2 > 0 ? 0.1 / std::sqrt(gn2) : 1.0;
    }
    for (unsigned i = 0; i < n; i++) q[i] *= gam;
    for (size_t k = 0; k < S.size(); k++) {
      double b = 0; for (unsigned i = 0; i < n; i++) b += Y[k][i] * q[i];
      b *= rho[k];
      for (unsigned i = 0; i < n; i++) q[i] += S[k][i] * (al[k] - b);
    }
    for (unsigned i = 0; i < n; i++) {
      d[i] = -q[i];
      if ((x(i) <= lb && d[i] < 0) || (x(i) >= ub && d[i] > 0)) d[i] = 0;  // active bounds
    }
    // backtracking on the objective; a step is kept only if it decreases nlZ (Opt_pars.cpp:268)
    double step = 1.0, fnew = fx;
    bool ok = false;
    for (int ls = 0; ls < 12; ls++) {
      for (unsigned i = 0; i < n; i++) xn(i) = std::min(ub, std::max(lb, x(i) + step * d[i]));
      set_GP_Pars(xn);
      fnew = Grad_Values(gn);
      numFuncEval++;
      if (fnew == fnew && fnew < fx) { ok = true; break; }
      step *= 0.5;
    }
    if (!ok) {
      set_GP_Pars(x);
      if (S.empty()) break;      // steepest-descent step failed too: stop
      S.clear(); Y.clear(); rho.clear();  // drop the curvature pairs and retry along -g
      if (getVerbose() > 0) std::cout << "Iteration: " << iter << " -logL: " << fx << std::endl;
      continue;
    }
    std::vector<double> s(n), yv(n);
    double sy = 0;
    for (unsigned i = 0; i < n; i++) { s[i] = xn(i) - x(i); yv[i] = gn(i) - g(i); sy += s[i] * yv[i]; }
    if (sy > 1e-12) {
      if (S.size() == mem) { S.erase(S.begin()); Y.erase(Y.begin()); rho.erase(rho.begin()); }
      S.push_back(s); Y.push_back(yv); rho.push_back(1.0 / sy);
    }
    double dx = 0; for (unsigned i = 0; i < n; i++) dx = std::max(dx, std::fabs(s[i]));
    x = xn; g = gn;
    double df = fx - fnew;
    fx = fnew;
    if (getVerbose() > 0) std::cout << "Iteration: " << iter << " -logL: " << fx << std::endl;
    if (dx < 1e-7 || df < 1e-9 * std::fabs(fx)) break;
  }
  set_GP_Pars(x);
}
