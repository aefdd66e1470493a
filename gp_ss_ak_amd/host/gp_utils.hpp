// gp_utils.hpp -- host-side mirror of the reference's model classes on the hot path:
// ModelInfo / Modeling (ModelInf.h:22-179), Opt_Algs (Opt_pars.h:21-315, callbacks only) and
// GP_utils (GP_Utils.h:23-389).  Same member names and call sequence; every O(N^2)/O(N^3)
// member forwards to the C-ABI (include/gpak.h) instead of Armadillo.
#pragma once
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../include/gpak.h"
#include "../../include/gpak_cv_folds.h"
#include "../../include/gpak_cv_groups_grad.h"
#include "../../include/gpak_cv_folds_grad.h"
#include "../../include/gpak_condition.h"
#include "../../include/gpak_design.h"
#include "../../include/gpak_local.h"
#include "../../include/gpak_local_ok.h"
#include "../../include/gpak_local_search.h"
#include "kernels.hpp"

class ModelInfo {
 public:
  virtual ~ModelInfo() {}
  virtual unsigned int getNumData() const { return numData; }
  virtual void setNumData(unsigned int v) { numData = v; }

 private:
  unsigned int numData = 0;
};

class Modeling : public ModelInfo {
 public:
  void setInpDim(unsigned int d) { inputDim = d; }
  unsigned int getInpDim() const { return inputDim; }
  void setOutDim(unsigned int d) { outputDim = d; }
  unsigned int getOutDim() const { return outputDim; }
  void setNumMFpar(unsigned int v) { NumMF = v; }
  unsigned int getNumMFpar() const { return NumMF; }
  void setNumlikfpar(unsigned int v) { Numlikf = v; }
  unsigned int getNumlikfpar() const { return Numlikf; }
  void setNumCovpar(unsigned int v) { NumCov = v; }
  unsigned int getNumCovpar() const { return NumCov; }
  virtual void Calc_Out(mat &yPred, mat &yVar, const mat &X) const = 0;
  virtual unsigned int getNumPars() const = 0;

 private:
  unsigned int outputDim = 1, inputDim = 0, NumMF = 0, Numlikf = 0, NumCov = 0;
};

// the optimiser's view of a model (Opt_pars.h:51-55) and the driver loop.
class Opt_Algs {
 public:
  enum { SCG, BFGS, LBFGS };
  virtual ~Opt_Algs() {}
  virtual unsigned int getNumPars() const = 0;
  virtual void get_GP_Pars(mat &param) const = 0;
  virtual void set_GP_Pars(mat &param) const = 0;
  virtual double Grad_Values(mat &g) const = 0;
  virtual double ObjVal() const = 0;
  // name of parameter i (ProjectedLBFGSOptimise keeps those that begin with "Angle" linear) and whether Grad_Values
  // returns the exact gradient of ObjVal (then Optimise runs ProjectedLBFGSOptimise)
  virtual std::string getParName(unsigned int) const { return ""; }
  virtual bool exactGradient() const { return false; }
  void setVerbose(int v) const { verbose = v; }
  int getVerbose() const { return verbose; }
  void setOptimiser(int v) { defaultOptimiser = v; }
  int getOptimiser() const { return defaultOptimiser; }
  std::string getDefaultOptimiserStr() const { return defaultOptimiser == SCG ? "SCG" : defaultOptimiser == BFGS ? "BFGS" : "LBFGS"; }
  void setMaxIters(unsigned int v) { maxIters = v; }
  unsigned int getMaxIters() const { return maxIters; }
  // Opt_pars.cpp:179-332 with cauchy_point (:11-105), Primal_Conjugate_grad (:108-174) and
  // Efficient_line_search (:543-974), restated as written in opt_algs.cpp: box [1e-4, 6] on every
  // parameter, memory 6, progress lines "Iteration: k -logL: v".
  void LBFGSOptimise();
  // plain projected L-BFGS with backtracking (not the reference's trajectory); GPAK_OPT=simple
  void SimpleLBFGSOptimise();
  // projected L-BFGS in log-parameters with Armijo backtracking, for an exact gradient (opt_algs.cpp)
  void ProjectedLBFGSOptimise();
  void Optimise() {
    const char *e = getenv("GPAK_OPT");
    if (exactGradient()) ProjectedLBFGSOptimise();
    else if (e && std::string(e) == "simple") SimpleLBFGSOptimise();
    else LBFGSOptimise();
  }
  unsigned int numFuncEval = 0;

 private:
  mutable int verbose = 0;
  int defaultOptimiser = LBFGS;
  unsigned int maxIters = 100;
};

class GP_utils : public Modeling, public Opt_Algs, public StreamIntfce {
 public:
  enum likelihoodTypeE { likeL_Gaussian, likeL_WarpGauss };
  enum InferenceTypeE { inf_laplace, inf_EP };
  enum MeanTypeE { mean_zero, mean_sum };

  GP_utils();
  GP_utils(Kernels *kernel, mat Xin, mat Yin, int Inf_type = inf_laplace, int likeLtype = likeL_Gaussian,
           int mean_type = mean_zero, unsigned int numhyper = 1, unsigned int numlik_par = 1,
           unsigned int numMF_par = 0, int verbos = 2);
  ~GP_utils();

  // uploads Xinp / yTarg to the device (the reference allocates its N x N members here,
  // GP_Utils.cpp:60-86; none of them exists on the host any more)
  void initialize_vars();

  // Modeling
  void Calc_Out(mat &yPred, mat &yVar, const mat &Xin) const override;
  void posteriorMeanVar(mat &mu, mat &varSigma, const mat &Xin) const;

  // Opt_Algs callbacks (Opt_pars.h:236-253)
  unsigned int getNumPars() const override;
  void get_GP_Pars(mat &param) const override;
  void set_GP_Pars(mat &param) const override;
  double Grad_Values(mat &g) const override { return GradLL(g); }
  double ObjVal() const override { return !group_labels.empty() ? GroupObjective() : loo_objective ? LooObjective() : logLikelihood(); }
  std::string getParName(unsigned int i) const override { return i < KerenlW->getNPars() ? KerenlW->getParamName(i) : "likelihood"; }
  bool exactGradient() const override { return exact_gradient || loo_objective || !group_labels.empty(); }

  double logLikelihood() const;   // NaN on Chol_fail (GP_Utils.cpp:1145-1158)
  // g is 1 x getNumPars(); the exact gradient (gpak_grad_exact) when exact_gradient is set; with loo_objective the
  // gradient of LooObjective() (gpak_loo_grad), with the group objective that of GroupObjective() (gpak_cv_groups_grad /
  // gpak_cv_folds_grad);
  // either is then the value returned
  double GradLL(mat &g) const;
  double LooObjective() const;    // -log_pl of gpak_loo at the current parameters; NaN on Chol_fail
  double GroupObjective() const;  // -log_pl of gpak_cv_groups with setGroupObjective's labels (of gpak_cv_folds with setFoldObjective's); NaN on Chol_fail
  // leave-one-out cross-validation of the training set from the current factor (gpak_loo): mean and variance (noise
  // included) of every yTarg(i) given all the other samples, N x 1 each; NaN on Chol_fail
  void LooCV(mat &mean, mat &var, gpak_loo_summary &s) const;
  // leave-group-out cross-validation (gpak_cv_groups): group[i] in [0, n_groups) for every training sample; mean and
  // marginal variance (noise included) of every yTarg(i) given all the samples outside its group, N x 1 each, and the
  // joint log predictive density of each group (n_groups x 1); NaN on Chol_fail
  void GroupCV(const std::vector<int> &group, int n_groups, mat &mean, mat &var, mat &logp, gpak_cv_groups_summary &s) const;
  // k-fold cross-validation (gpak_cv_folds): GroupCV for groups of any size
  void FoldCV(const std::vector<int> &group, int n_groups, mat &mean, mat &var, mat &logp, gpak_cv_groups_summary &s) const;
  // block-support prediction (gpak_predict_block): mean and variance of the average of the field over each block, block
  // b = rows b * nd .. b * nd + nd of Xd; the variance includes sn2 / nd unless latent; M x 1 each, NaN on Chol_fail
  void BlockMeanVar(mat &mean, mat &var, const mat &Xd, int nd, bool latent) const;
  // joint posterior of the blocks (gpak_predict_joint): mean M x 1 and the full M x M covariance (exactly symmetric;
  // the diagonal includes sn2 / nd unless latent and is not clamped); NaN on Chol_fail
  void JointMeanCov(mat &mean, mat &cov, const mat &Xd, int nd, bool latent) const;
  // conditional simulation (gpak_sample_joint): Z (M x S) = mean 1' + Lc Xi for the caller's normals Xi (M x S), Lc the
  // factor of the covariance + nugget I.  Returns false when that matrix is not positive definite (Z NaN, mean valid);
  // everything NaN on Chol_fail
  bool JointSample(mat &Z, mat &mean, const mat &Xd, int nd, const mat &Xi, double nugget, bool latent) const;
  // conditional simulation at any node count (gpak_sample_path): a spectral draw of the prior from `features` frequencies
  // per stationary term (sim_spectral.hpp), conditioned on the data by kriging; every normal comes from the one stream of
  // `seed` in sim_spectral.hpp's order.  Unless latent, sqrt((sn2 + white) / nd) times a normal is added per node and
  // realisation on the host.  Everything NaN on Chol_fail (then false)
  bool PathSample(mat &Z, mat &mean, const mat &Xd, int nd, unsigned long long seed, int features, bool latent,
                  gpak_condition_summary &summary) const;
  // moving-neighbourhood kriging (gpak_predict_local) of the blocks of Xd (as BlockMeanVar) from the samples (Xs, ys) that
  // nbr (k per node, -1 padded: LocalNeighbours) names; the context needs the kernel only, no training set.  LocalMetric:
  // G (4 x 4) of stationary term 0 (gpak_local_metric); LocalNeighbours: the k nearest samples of every centre in it
  void LocalMetric(double G[16]) const;
  static void LocalNeighbours(const mat &Xs, const mat &Xc, const double G[16], int k, double radius, std::vector<int> &nbr,
                              std::vector<int> &used);
  // LocalNeighboursDev: the same lists from the context's device (gpak_local_neighbours_dev)
  void LocalNeighboursDev(const mat &Xs, const mat &Xc, const double G[16], int k, double radius, std::vector<int> &nbr,
                          std::vector<int> &used, gpak_local_search_summary &summary) const;
  void LocalMeanVar(mat &mean, mat &var, const mat &Xs, const mat &ys, const mat &Xd, int nd, const std::vector<int> &nbr, int k,
                    bool latent, gpak_local_summary &summary) const;
  // the same with ordinary kriging (gpak_predict_local_ok), mu the local means; LocalNeighboursOctant: at most per_octant
  // samples from each octant around a centre inside the radius, of those the k nearest (gpak_local_neighbours_octant)
  static void LocalNeighboursOctant(const mat &Xs, const mat &Xc, const double G[16], int k, int per_octant, double radius,
                                    std::vector<int> &nbr, std::vector<int> &used);
  void LocalMeanVarOk(mat &mean, mat &var, mat &mu, const mat &Xs, const mat &ys, const mat &Xd, int nd, const std::vector<int> &nbr,
                      int k, bool latent, gpak_local_summary &summary) const;
  // infill drilling design (gpak_design): the gain of each of the H candidate holes (hole[i] in [0, H) for candidate point i
  // of Xc) on the target blocks Xd (nd points each; wt: one weight per block, or null) and a greedy plan of k of them;
  // false when the A_h of some hole is not positive definite; everything NaN on Chol_fail
  bool DesignHoles(const mat &Xd, int nd, const mat &Xc, const std::vector<int> &hole, int H, const double *wt, int k,
                   std::vector<double> &gain, std::vector<int> &picked, std::vector<double> &pick_gain,
                   gpak_design_summary &summary) const;
  void OptimisePars(unsigned int iters);
  void updateKernel() const;
  std::ostream &ShowKernelPars(std::ostream &os) const;

  double getHyperlfVal(unsigned int i) const { return hyperlf(i); }
  void setHyperlfVal(double v, unsigned int i) const { hyperlf(i) = v; dirty = true; }
  void setInf(const std::string &s) { InfS = s; }
  std::string getInf() const { return InfS; }
  void setMean(const std::string &s) { MeanS = s; }
  std::string getMean() const { return MeanS; }
  void setLikelihoodType(int v) { likelihoodType = v; }
  int getLikelihoodType() const { return likelihoodType; }
  void setCompatFlags(int f) { compat = f; }
  // device-side options of every GP_utils constructed afterwards (the CLI's --precision / --gpus)
  static void setDeviceOptions(int precision, int gpus) { default_precision = precision; default_gpus = gpus; }
  // the CLI's --gradient: false (default) = GradLL + getGradients as the reference writes them (gpak_grad_hyb),
  // true = the derivative of logLikelihood() (gpak_grad_exact) and, through Optimise(), the driver that suits it
  static void setExactGradient(bool v) { exact_gradient = v; }
  // the CLI's --objective: false (default) = Optimise() minimises logLikelihood(); true = it minimises LooObjective()
  // with its exact gradient, through the exact gradient's driver
  static void setLooObjective(bool v) { loo_objective = v; }
  // the CLI's --objective lgo: Optimise() minimises GroupObjective(), -log_pl of the leave-group-out predictions of
  // gpak_cv_groups, with its exact gradient gpak_cv_groups_grad through the exact gradient's driver.  labels[i] in
  // [0, n_groups) for every training sample, in training order, no group above GPAK_CV_GROUP_MAX; no labels: off
  static void setGroupObjective(const std::vector<int> &labels, int n_groups) { group_labels = labels; group_count = n_groups; fold_objective = false; }
  // the same for groups of any size (train --folds / --kfold): GroupObjective() is -log_pl of gpak_cv_folds and its
  // gradient gpak_cv_folds_grad
  static void setFoldObjective(const std::vector<int> &labels, int n_groups) { group_labels = labels; group_count = n_groups; fold_objective = true; }
  // gpak_phase_times of this model's context as one JSON object (the CLI's --timing)
  std::string timingJson() const;
  bool Chol_failed() const { return Chol_fail; }

  void ToFile_GP_Params(std::ostream &out) const override;
  void FromFile_GP_Params(std::istream &in) override;

  mat Xinp;
  mat yTarg;
  Kernels *KerenlW = nullptr;
  mutable mat hyperlf;

 private:
  void sync_params() const;
  gpak_ctx *ctx = nullptr;
  static int default_precision, default_gpus;
  static bool exact_gradient, loo_objective;
  static std::vector<int> group_labels;   // setGroupObjective: empty = no group objective
  static int group_count;
  static bool fold_objective;             // setFoldObjective: the labels are folds of any size
  void create_ctx();
  bool owns_kernel = false;
  mutable bool dirty = true;     // KUpdateStat / AlphaUpStatus (GP_Utils.h:257-279)
  mutable bool Chol_fail = false;
  int likelihoodType = likeL_Gaussian;
  int compat = 3;                // reproduce Q3/Q4 of SURVEY.md 8(c) like the reference
  std::string InfS = "Lapalce", MeanS = "Zero";
};

void writeGPFile(const GP_utils &model, const std::string &modelFileName, const std::string &comment = "");
GP_utils *readGpFromFile(const std::string &modelFileName, int verbosity = 2);
