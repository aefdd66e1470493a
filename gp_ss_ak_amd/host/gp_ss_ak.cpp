// gp_ss_ak.cpp -- the reference's command line (gp_ss_ak.cpp:14-557) over the HIP hot path:
//   gp_ss_ak [-v n] [-pm m] [-np] [device options] train [-k ExpAns] [-kn 1] [-o LBFGS] [-# iters]
//            [--groups labels.txt | --folds labels.txt | --kfold K [--seed n]] train.txt [model]
//   gp_ss_ak [-v n] [-pm m]       [device options] test  test.txt model train.txt [out_file]
//   gp_ss_ak [-v n]               [device options] cv [-np] [--groups labels.txt | --folds labels.txt | --kfold K [--seed n]]
//            train.txt model [out_file]
//   gp_ss_ak [-v n] --block-size dx,dy,dz --block-disc nx,ny,nz [--latent] block blocks.txt model train.txt [out_file]
//   gp_ss_ak [-v n] [--block-size dx,dy,dz --block-disc nx,ny,nz] [--latent] [--nugget v] --realisations S (--seed n | --xi file)
//            sim [--method joint|path [--features F]] nodes.txt model train.txt [out_file]
//   gp_ss_ak [-v n] --neighbours k [--radius r] [--octant n] [--kriging simple|ordinary] [--search host|device]
//            [--block-size dx,dy,dz --block-disc nx,ny,nz] [--latent] local nodes.txt model train.txt [out_file]
// device options (not reference flags): --gpus n (multi-GPU context), --precision f64|f32
// (fp32 prediction work), --timing file|- (JSON of the context's phase times after the verb), --gradient reference|exact
// (exact: GradLL returns the derivative of nlZ and -o LBFGS runs Opt_Algs::ProjectedLBFGSOptimise; one GPU only),
// --objective nlz|loo (loo: `train` minimises -log_pl of the leave-one-out predictions, what `cv` reports, with its exact
// gradient gpak_loo_grad and the exact gradient's driver; the objective column of the trace holds -log_pl; one GPU only;
// lgo: the same for the leave-group-out predictions of `cv --groups`, with gpak_cv_groups_grad: `--objective lgo train
// --groups FILE`, FILE as `cv --groups` reads it and held to the same checks before a context exists; `--objective lgo train
// --folds FILE` and `--objective lgo train --kfold K [--seed n]` the same for groups of any size, with gpak_cv_folds_grad,
// the labels read, made and checked as `cv --folds` / `cv --kfold` do it, so that `cv --kfold K --seed n` on the trained
// model reports the criterion that was trained.  `train` reads the
// samples with readDataFile, which fills row p from the p-th data line, and prepareData, which shifts and scales columns
// in place; GP_utils hands Xinp and yTarg to gpak_set_train as they are.  No step reorders, drops or adds a row, so label
// i of FILE belongs to training sample i of the context, exactly as in `cv`).
// cv (not a reference verb): leave-one-out cross-validation of a trained model on its training set, from one
// factorisation (gpak_loo; one GPU only), written to <model>_loo.txt.  With --groups FILE (one integer label per training
// sample, in input order; `#` lines are skipped) it leaves out whole groups instead -- a drill hole, a fold -- of at most
// 128 samples each (gpak_cv_groups) and writes <model>_lgo.txt.  With --folds FILE (labels as for --groups) the groups may
// have any size -- k folds of N / k samples, a hole of 150 (gpak_cv_folds) -- and it writes <model>_folds.txt; --kfold K
// [--seed n, default 1] makes the labels itself: the fold of a sample is its position in a seeded permutation mod K
// (kfold_assign.hpp), recorded in the Fold column.  The three options exclude each other.
// block (not a reference verb): mean and standard deviation of the AVERAGE grade of rectangular blocks (gpak_predict_block;
// one GPU only).  blocks.txt has the test file's format: block centres, and a last column that is read as y and carried
// through.  Each block is discretised in the file's units into nx * ny * nz cell-centred points, which then pass through
// the same input transform as `test`; written to <model>_block.txt in input order.
// sim (not a reference verb): S realisations of the grade at the nodes given the training data (conditional simulation,
// gpak_sample_joint; one GPU only).  nodes.txt is read as block reads its centres; without --block-size / --block-disc the
// nodes are points.  The normals come from --xi (an M x S text matrix) or from --seed (std::mt19937_64 + Box-Muller,
// sim_normals.hpp).  Written to <model>_sim.txt in input order: the conditional mean and the S realisations.
// sim --method path [--features F, default 4096] (with --seed; no --xi, no --nugget): the same file for ANY number of nodes
// (gpak_sample_path): a spectral draw of the prior from F random frequencies per stationary term (sim_spectral.hpp; its
// covariance is the prior's to O(1/sqrt(F))) conditioned on the data by kriging, which is exact; no M x M matrix exists.
// design (not a reference verb): ranks candidate drill holes by the estimation variance they would remove from the targets
// (gpak_design; one GPU only):  gp_ss_ak [--block-size dx,dy,dz --block-disc nx,ny,nz] [--pick k] [--weights w.txt]
// design --candidates cand.txt --holes holes.txt targets.txt model train.txt.  targets.txt and cand.txt are read as block
// reads its centres (the last column is carried for the targets and ignored for the candidates; without --block-size /
// --block-disc the targets are points); holes.txt holds one integer label per candidate point, read and checked as `cv
// --groups` reads its labels and mapped to 0 .. H - 1 in ascending order; --weights one non-negative number per target.
// Everything is checked before a context exists.  Written to <model>_design.txt, one line per hole in ascending label:
// Hole, Samples, Gain, Share = gain / var_before, Pick = 1 .. k in pick order or 0, and for a picked hole its conditional
// gain.  Variances are in the units of the model's standardised grade.
// Same verbs, flags and files (<model>, <model>_Statistics.txt, <model>_predict.txt,
// <model>_gnu.plt); -np/--no-prompt skips the two interactive stdin questions of `train`
// (gp_ss_ak.cpp:235-285) and the gnuplot call of `test` (:503-505).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <numeric>
#include <chrono>
#include <sstream>
#include <string>

#include "block_points.hpp"
#include "control.hpp"
#include "gp_utils.hpp"
#include "kfold_assign.hpp"
#include "sim_normals.hpp"

class GP_Cntrl : public Control {
 public:
  GP_Cntrl(int argc, char **argv) : Control(argc, argv) {
    GP_utils::setDeviceOptions(precision, gpus);
    GP_utils::setExactGradient(exact_gradient);
    GP_utils::setLooObjective(loo_objective);
  }
  // FILE of --groups for leave-group-out: the labels as read, their sorted unique values and each sample's rank among them;
  // everything that can be refused is refused here, before a context exists
  void groupLabelsOf(const std::string &file, int n, std::vector<long long> &labels, std::vector<long long> &values,
                     std::vector<int> &group) const;
  void writeTiming(const GP_utils &m) const {
    if (timing_file.empty()) return;
    const std::string j = m.timingJson();
    if (timing_file == "-") { std::cout << "TIMING " << j << std::endl; return; }
    std::ofstream out(timing_file.c_str());
    out << j << "\n";
  }
  void train();
  void test();
  void cv();
  void readGroupLabels(const std::string &file, std::vector<long long> &labels, const std::string &option) const;
  // --folds FILE | --kfold K [--seed n] of `cv` and `train`: the options as given, and the labels they stand for
  struct FoldOptions {
    std::string file;
    bool kfold_set = false, seed_set = false;
    bool seed_here = false;               // --seed among the verb's own options (not only before the verb, where sim reads it)
    long kfold = 0;
    unsigned long long seed = 1;
    bool given() const { return !file.empty() || kfold_set; }
  };
  bool foldOption(FoldOptions &o);   // the current argument is one of the three: taken (with its value); else false
  // the labels of n training samples (read or made), their sorted unique values and each sample's rank among them;
  // everything that can be refused is refused here, before a context exists
  void foldLabelsOf(const FoldOptions &o, int n, std::vector<long long> &labels, std::vector<long long> &values,
                    std::vector<int> &group) const;
  void block();
  void sim();
  void design();
  void local();
  void localOptionsOnlyWithLocal() const {
    if (local_kriging_set || local_octant_set) ErrorTermination("--kriging and --octant are options of the local verb");
    if (local_search_set) ErrorTermination("--search is an option of the local verb");
  }
  void Help() const;
};

void GP_Cntrl::Help() const {
  std::cout << "\nGP_SS_AK hot path on MI355X\nCommand:\n \t ./gp_ss_ak [options] Command [Comnd-options] TrainDataFile.txt modelName\n"
            << "Commands:\ntrain :\n \t To find hyperparameter by maxmizing likelihood (--objective loo: the leave-one-out pseudo-likelihood; --objective lgo with train --groups file: the leave-group-out one; with train --folds file / --kfold K [--seed n]: the same for groups of any size, k folds).\n"
            << "test :\n \t To estimate test data set and plot the results.\n"
            << "cv :\n \t To cross-validate a trained model on its training data, leaving one sample out at a time (--groups file: one group of samples at a time; --folds file / --kfold K [--seed n]: groups of any size, k folds).\n"
            << "design :\n \t To rank candidate drill holes by the estimation variance they would remove from targets ([--block-size dx,dy,dz --block-disc nx,ny,nz] [--pick k] [--weights file] design --candidates file --holes file targets model train).\n"
            << "local :\n \t To estimate nodes or blocks from the k nearest of any number of samples (--neighbours k [--radius r] [--octant n: at most n samples per octant, needs --radius] [--kriging simple|ordinary: ordinary re-estimates the mean from every node's own samples] [--search host|device: device searches the neighbours on the GPU, the same lists; not with --octant] [--block-size dx,dy,dz --block-disc nx,ny,nz] [--latent] local nodes model samples).\n"
            << "block :\n \t To estimate the average over blocks (--block-size dx,dy,dz --block-disc nx,ny,nz [--latent]) and its standard deviation.\n"
            << "sim :\n \t To draw realisations at nodes or blocks given the data (--realisations S and --seed n or --xi file; [--nugget v] [--latent]; sim --method path [--features F] with --seed n: any number of nodes, the prior from F random frequencies per term).\n";
}

void GP_Cntrl::train() {
  incArg();
  setMode("train");
  bool yscale = true, Knoise = true;
  std::string optimiser = "LBFGS", modelName = "gp_model", groupsFile;
  FoldOptions fo;
  fo.seed_set = sim_seed_set;
  if (sim_seed_set) fo.seed = sim_seed;
  std::vector<std::string> KernT;
  int iters = 100;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-mf", "--meanfunction")) { incArg(); if (getArg() != "mean_zero") ErrorTermination("Unrecognised mean function"); }
      else if (isArg("-lf", "--likefunction")) { incArg(); if (getArg() != "Gauss") ErrorTermination("Only the Gauss likelihood is reachable (gp_ss_ak.cpp:192-196)"); }
      else if (isArg("-k", "--kernel")) { incArg(); KernT.push_back(getArg()); }
      else if (isArg("-o", "--optimiser")) { incArg(); optimiser = getArg(); }
      else if (isArg("-#", "--iterations")) { incArg(); iters = getIntArg(); }
      else if (isArg("-kn", "--Knoise")) { incArg(); Knoise = getIntArg() != 0; }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else if (isArg("--groups", "--groups")) {
        incArg();
        if (getArgNo() >= argc) ErrorTermination("--groups takes a file of labels");
        groupsFile = getArg();
      }
      else if (foldOption(fo)) {}
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if ((int)!groupsFile.empty() + (int)!fo.file.empty() + (int)fo.kfold_set > 1)
    ErrorTermination("--groups, --folds and --kfold exclude each other: give one of them");
  if (fo.seed_set && !fo.kfold_set && (fo.seed_here || !fo.file.empty())) ErrorTermination("--seed goes with --kfold");
  if (lgo_objective && groupsFile.empty() && !fo.given())
    ErrorTermination("--objective lgo needs the groups to leave out: train --groups FILE (one integer label per training sample)");
  if (!lgo_objective && !groupsFile.empty())
    ErrorTermination("train --groups goes with --objective lgo (training on the leave-group-out criterion)");
  if (!lgo_objective && fo.given())
    ErrorTermination(std::string("train ") + (fo.kfold_set ? "--kfold" : "--folds") +
                     " goes with --objective lgo (training on the leave-group-out criterion)");
  if (getArgNo() >= argc) ErrorTermination("There are not enough input parameters.");
  std::string trainFileName = getArg();
  if (getArgNo() + 1 < argc) modelName = argv[getArgNo() + 1];
  int ds[2];
  readDataSize(trainFileName, ds);
  if (lgo_objective) {   // the labels of row i of the file are those of training sample i: see the header comment
    std::vector<long long> labels, values;
    std::vector<int> group;
    if (fo.given()) {
      foldLabelsOf(fo, ds[0], labels, values, group);
      GP_utils::setFoldObjective(group, (int)values.size());
    } else {
      groupLabelsOf(groupsFile, ds[0], labels, values, group);
      GP_utils::setGroupObjective(group, (int)values.size());
    }
  }
  mat X, y;
  readDataFile(X, y, ds, trainFileName);
  prepareData(X, y, yscale, modelName);

  HybKerns Kerns(X);
  for (auto &k : KernT) {
    if (k == "ExpAns") { Kern_ExpAnisotropic e(X); Kerns.addNewKernel(&e); }
    else if (k == "Bias") { Kern_Bias b(X); Kerns.addNewKernel(&b); }
    else if (k == "RBF") { Kern_RBF r(X); Kerns.addNewKernel(&r); }
    else if (k == "Exp") { Kern_Exponential e(X); Kerns.addNewKernel(&e); }
    else if (k == "White") { Kern_White w(X); Kerns.addNewKernel(&w); }
    else ErrorTermination("Unknown covariance function: " + k);
  }
  if (Kerns.getNumKerns() == 0) { Kern_ExpAnisotropic e(X); Kerns.addNewKernel(&e); }
  if (Knoise) { Kern_Bias b(X); Kerns.addNewKernel(&b); }

  GP_utils *GPModel = new GP_utils(&Kerns, X, y, GP_utils::inf_laplace, GP_utils::likeL_Gaussian, GP_utils::mean_zero,
                                   8, 1, 0, getVerbose());
  std::cout << "The inital value of the kernel parameters are as follows :" << std::endl;
  std::cout << "There are " << GPModel->KerenlW->getNPars() << " parameters to be optimized" << std::endl;
  for (unsigned i = 0; i < GPModel->KerenlW->getNPars(); i++)
    std::cout << GPModel->KerenlW->getParamName(i) << " : " << GPModel->KerenlW->getParam(i) << std::endl;
  if (!no_prompt) {
    std::cout << "Do you want to change the defult kernel parameters (Yes|Y|y or press any key)?" << std::endl;
    std::string res = "No";
    std::cin >> res;
    if (res == "Yes" || res == "Y" || res == "y") {
      for (unsigned i = 0; i < GPModel->KerenlW->getNPars(); i++) {
        if (GPModel->KerenlW->getParamName(i) == "InversewidthR_ExpAns" && X.n_cols == 3) continue;
        std::cout << " Please input an initial value for " << GPModel->KerenlW->getParamName(i) << " (Default value was "
                  << GPModel->KerenlW->getParam(i) << ") : " << std::endl;
        double d = GPModel->KerenlW->getParam(i);
        std::cin >> d;
        GPModel->KerenlW->setParam(d, i);
      }
    }
  }
  std::cout << "The inital value of the likelihood function are as follows :" << std::endl;
  std::cout << "likelihood hyperparameter : " << GPModel->getHyperlfVal(0) << std::endl;
  if (!no_prompt) {
    std::cout << "Do you want to change the defult likelihood function parameters (Yes|Y|y or press any key)?" << std::endl;
    std::string res = "No";
    std::cin >> res;
    if (res == "Yes" || res == "Y" || res == "y") {
      std::cout << "Please input an initial value for Gauss likelihood function : " << std::endl;
      double d = GPModel->getHyperlfVal(0);
      std::cin >> d;
      GPModel->setHyperlfVal(d, 0);
    }
  }
  if (optimiser == "LBFGS") GPModel->setOptimiser(GP_utils::LBFGS);
  else if (optimiser == "BFGS" || optimiser == "SCG") {
    std::cout << "Optimiser " << optimiser << " is not built on the HIP path; using LBFGS." << std::endl;
    GPModel->setOptimiser(GP_utils::LBFGS);
  } else ErrorTermination("Unrecognised optimiser type: " + optimiser);
  // gp_ss_ak.cpp:295: the iteration count travels only through OptimisePars, which applies it when verbosity > 2
  // (GP_Utils.cpp:1295-1296); otherwise the constructor's 100 (Opt_pars.h:35) stays.  Reproduced as written.
  GPModel->OptimisePars(iters);

  writeGPFile(*GPModel, modelName, "# GP_SS_AK Model File ");
  // the reference evaluates the model on its own training set (gp_ss_ak.cpp:301-325)
  mat EstVals(X.n_rows, 1), EstVals_Var(X.n_rows, 1);
  GPModel->Calc_Out(EstVals, EstVals_Var, X);
  postData(X, EstVals, yscale, modelName);
  postData_var(EstVals_Var, yscale, modelName);
  postData(y, yscale, modelName);
  double mse = 0, ym = 0, vy = 0;
  for (size_t i = 0; i < y.n_elem; i++) { mse += (y[i] - EstVals[i]) * (y[i] - EstVals[i]); ym += y[i]; }
  mse /= X.n_rows; ym /= y.n_elem;
  for (size_t i = 0; i < y.n_elem; i++) vy += (y[i] - ym) * (y[i] - ym);
  vy /= y.n_elem;
  if (getVerbose() > 0) { std::cout << "Mean Square Error of training: " << mse << "\n"; std::cout << "Var MSE Train: " << vy << "\n"; }
  else { std::cout << mse << "\n" << vy << "\n"; }
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

void GP_Cntrl::test() {
  incArg();
  setMode("test");
  bool yscale = true;
  std::string modelName = "model", trFile;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if (getArgNo() >= argc) ErrorTermination("There are not enough input parameters.");
  std::string teFile = getArg();
  if (getArgNo() + 1 < argc) modelName = argv[getArgNo() + 1];
  if (getArgNo() + 2 < argc) trFile = argv[getArgNo() + 2];
  else ErrorTermination("Please provide training data");
  std::string PredictOut = modelName + "_predict.txt";
  if (getArgNo() + 3 < argc) PredictOut = argv[getArgNo() + 3];
  int ds[2];
  readDataSize(teFile, ds);
  mat X, y;
  readDataFile(X, y, ds, teFile);
  prepareData(X, y, yscale, modelName);
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // parameters at 6 significant digits (Q5)
  readDataSize(trFile, ds);
  mat Xtr, ytr;
  readDataFile(Xtr, ytr, ds, trFile);
  prepareData(Xtr, ytr, yscale, modelName);
  GPModel->yTarg = ytr;
  GPModel->Xinp = Xtr;
  GPModel->setNumData((unsigned)Xtr.n_rows);
  GPModel->initialize_vars();
  GPModel->logLikelihood();
  if (X.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  mat EstVals(y.n_rows, 1), EstVals_Var(y.n_rows, 1);
  GPModel->Calc_Out(EstVals, EstVals_Var, X);
  postData(X, EstVals, yscale, modelName);
  postData_var(EstVals_Var, yscale, modelName);
  postData(y, yscale, modelName);
  double mse = 0, ym = 0, vy = 0;
  for (size_t i = 0; i < y.n_elem; i++) { mse += (y[i] - EstVals[i]) * (y[i] - EstVals[i]); ym += y[i]; }
  mse /= X.n_rows; ym /= y.n_elem;
  for (size_t i = 0; i < y.n_elem; i++) vy += (y[i] - ym) * (y[i] - ym);
  vy /= y.n_elem;
  if (getVerbose() > 0) { std::cout << "Mean Square Error of testing: " << mse << "\n"; std::cout << "Var MSE Test: " << vy << "\n"; }
  else { std::cout << mse << "\n" << vy << "\n"; }
  // rows sorted by ascending y (gp_ss_ak.cpp:434-481)
  std::vector<size_t> idx(y.n_elem);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return y[a] < y[b]; });
  std::ofstream out(PredictOut.c_str());
  out << "# SampleNo, Y,  Yh, StdYh, Inputs" << "\n";
  for (size_t r = 0; r < idx.size(); r++) {
    size_t i = idx[r];
    out << (r + 1) << "\t" << y[i] << "\t" << EstVals[i] << "\t" << EstVals_Var[i] << "\t";
    for (size_t j = 0; j < X.n_cols; j++) out << X(i, j) << "\t";
    out << "\n";
  }
  out.close();
  std::ofstream gnu((modelName + "_gnu.plt").c_str());
  gnu << "#gnuplot -persist output.plt\n set term pdf transparent enhanced \n set output '" << modelName << "_predict.pdf'  \n"
      << "set title \"Observed vs Estimated\"\n set xlabel \"Sample\"\n"
      << "plot \"" << PredictOut << "\" using 1:($3 + $4):($3 - $4) with filledcurve fc rgb \"green\" title '95% CI', "
      << "\"\" using 1:3 with lines lc rgb \"red\" t \"Estimated\", \"\" using 1:2 lc rgb \"blue\" t \"Observed\" with lines \n";
  gnu.close();
  if (!no_prompt && system("command -v gnuplot > /dev/null 2>&1") == 0) {
    std::string cmd = "gnuplot -persist " + modelName + "_gnu.plt";
    if (system(cmd.c_str()) != 0) std::cerr << "gnuplot failed" << std::endl;
  }
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

// one integer label per line (or several, separated by blanks, tabs or commas); `#` lines are skipped.  option: the
// command-line option the file came with, for the error text
void GP_Cntrl::readGroupLabels(const std::string &file, std::vector<long long> &labels, const std::string &option) const {
  std::ifstream in(file.c_str());
  if (!in.is_open()) ErrorTermination("File is " + file + " not readable");
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line[0] == '#') continue;
    for (char &ch : line) if (ch == '\t' || ch == ',' || ch == '\r') ch = ' ';
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      char *end = nullptr;
      errno = 0;
      const long long v = strtoll(tok.c_str(), &end, 10);
      if (end == tok.c_str() || *end != '\0' || errno == ERANGE)
        ErrorTermination(option + ": '" + tok + "' in " + file + " is not an integer label");
      labels.push_back(v);
    }
  }
}

void GP_Cntrl::groupLabelsOf(const std::string &file, int n, std::vector<long long> &labels, std::vector<long long> &values,
                             std::vector<int> &group) const {
  readGroupLabels(file, labels, "--groups");
  if ((int)labels.size() != n)
    ErrorTermination("--groups: " + file + " holds " + std::to_string(labels.size()) + " labels for " + std::to_string(n) +
                     " training samples");
  values = labels;
  std::sort(values.begin(), values.end());
  values.erase(std::unique(values.begin(), values.end()), values.end());
  std::vector<int> count(values.size(), 0);
  group.resize(labels.size());
  for (size_t i = 0; i < labels.size(); i++) {
    group[i] = (int)(std::lower_bound(values.begin(), values.end(), labels[i]) - values.begin());
    if (++count[group[i]] == GPAK_CV_GROUP_MAX + 1)
      ErrorTermination("--groups: group " + std::to_string(labels[i]) + " has more than " + std::to_string(GPAK_CV_GROUP_MAX) +
                       " samples (leave-group-out holds a group in one workgroup's memory)");
  }
}

bool GP_Cntrl::foldOption(FoldOptions &o) {
  if (isArg("--folds", "--folds")) {
    incArg();
    if (getArgNo() >= argc) ErrorTermination("--folds takes a file of labels");
    o.file = getArg();
    return true;
  }
  if (isArg("--kfold", "--kfold")) {
    incArg();
    char *end = nullptr;
    const std::string tok = getArg();
    o.kfold = strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end != '\0') ErrorTermination("--kfold takes the number of folds");
    o.kfold_set = true;
    return true;
  }
  if (isArg("--seed", "--seed")) {
    incArg();
    char *end = nullptr;
    const std::string tok = getArg();
    o.seed = strtoull(tok.c_str(), &end, 10);
    if (tok.empty() || *end != '\0') ErrorTermination("--seed takes a non-negative integer");
    o.seed_set = o.seed_here = true;
    return true;
  }
  return false;
}

void GP_Cntrl::foldLabelsOf(const FoldOptions &o, int n, std::vector<long long> &labels, std::vector<long long> &values,
                            std::vector<int> &group) const {
  if (o.kfold_set) {
    if (o.kfold < 2 || o.kfold > n)
      ErrorTermination("--kfold: " + std::to_string(o.kfold) + " folds for " + std::to_string(n) +
                       " training samples (2 <= K <= N is needed)");
    gpak_kfold_assign(o.seed, (size_t)n, (int)o.kfold, group);
    labels.assign(group.begin(), group.end());
  } else {
    readGroupLabels(o.file, labels, "--folds");
    if ((int)labels.size() != n)
      ErrorTermination("--folds: " + o.file + " holds " + std::to_string(labels.size()) + " labels for " + std::to_string(n) +
                       " training samples");
  }
  values = labels;
  std::sort(values.begin(), values.end());
  values.erase(std::unique(values.begin(), values.end()), values.end());
  group.resize(labels.size());
  for (size_t i = 0; i < labels.size(); i++)
    group[i] = (int)(std::lower_bound(values.begin(), values.end(), labels[i]) - values.begin());
}

void GP_Cntrl::cv() {
  incArg();
  setMode("cv");
  if (gpus > 1)
    ErrorTermination("cv runs on one GPU only (leave-one-out cross-validation is not built for multi-GPU contexts): drop --gpus");
  bool yscale = true;
  std::string groupsFile;
  FoldOptions fo;
  fo.seed_set = sim_seed_set;
  if (sim_seed_set) fo.seed = sim_seed;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else if (isArg("--groups", "--groups")) {
        incArg();
        if (getArgNo() >= argc) ErrorTermination("--groups takes a file of labels");
        groupsFile = getArg();
      }
      else if (foldOption(fo)) {}
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if ((int)!groupsFile.empty() + (int)!fo.file.empty() + (int)fo.kfold_set > 1)
    ErrorTermination("--groups, --folds and --kfold exclude each other: give one of them");
  if (fo.seed_set && !fo.kfold_set) ErrorTermination("--seed goes with --kfold");
  if (getArgNo() + 1 >= argc) ErrorTermination("There are not enough input parameters: cv needs the training data and the model.");
  std::string trFile = getArg(), modelName = argv[getArgNo() + 1];
  const bool grouped = !groupsFile.empty(), folded = fo.given();
  std::string LooOut = modelName + (grouped ? "_lgo.txt" : folded ? "_folds.txt" : "_loo.txt");
  if (getArgNo() + 2 < argc) LooOut = argv[getArgNo() + 2];
  int ds[2];
  readDataSize(trFile, ds);
  std::vector<long long> labels, values;   // as read; the sorted unique labels
  std::vector<int> group;                  // rank of each sample's label among them
  if (grouped) groupLabelsOf(groupsFile, ds[0], labels, values, group);   // refused before a context exists
  if (folded) foldLabelsOf(fo, ds[0], labels, values, group);             // the same
  mat X, y;
  readDataFile(X, y, ds, trFile);
  prepareData(X, y, yscale, modelName);                         // the model's _Statistics.txt, as `test`
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // parameters at 6 significant digits (Q5)
  if (X.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  GPModel->yTarg = y;
  GPModel->Xinp = X;
  GPModel->setNumData((unsigned)X.n_rows);
  GPModel->initialize_vars();
  GPModel->logLikelihood();
  mat LooVals(y.n_rows, 1), LooVals_Var(y.n_rows, 1);
  if (folded) {
    mat logp(values.size(), 1);
    gpak_cv_groups_summary gs;
    GPModel->FoldCV(group, (int)values.size(), LooVals, LooVals_Var, logp, gs);
    postData(X, LooVals, yscale, modelName);
    postData_var(LooVals_Var, yscale, modelName);
    postData(y, yscale, modelName);
    double mse = 0, ym = 0, vy = 0;
    for (size_t i = 0; i < y.n_elem; i++) { mse += (y[i] - LooVals[i]) * (y[i] - LooVals[i]); ym += y[i]; }
    mse /= X.n_rows; ym /= y.n_elem;
    for (size_t i = 0; i < y.n_elem; i++) vy += (y[i] - ym) * (y[i] - ym);
    vy /= y.n_elem;
    if (getVerbose() > 0) {
      std::cout << "Mean Square Error of k-fold: " << mse << "\n" << "Var MSE Train: " << vy << "\n"
                << "Mean standardised squared residual: " << gs.mssr << "\n" << "Mean squared Mahalanobis residual: " << gs.msmd << "\n"
                << "Log predictive density of the groups: " << gs.log_pl << "\n" << "Folds: " << gs.groups << "\n"
                << "CV ms: " << gs.ms << "\n";
    } else { std::cout << mse << "\n" << vy << "\n" << gs.mssr << "\n" << gs.msmd << "\n" << gs.log_pl << "\n"; }
    // rows in input order; the fifth column is what postData_var returns, as StdYh of _predict.txt
    std::ofstream out(LooOut.c_str());
    out << "# SampleNo, Fold, Y, Ycv, StdYcv, Inputs" << "\n";
    for (size_t i = 0; i < y.n_elem; i++) {
      out << (i + 1) << "\t" << labels[i] << "\t" << y[i] << "\t" << LooVals[i] << "\t" << LooVals_Var[i] << "\t";
      for (size_t j = 0; j < X.n_cols; j++) out << X(i, j) << "\t";
      out << "\n";
    }
    out.close();
    writeTiming(*GPModel);
    delete GPModel;
    exit(0);
  }
  if (grouped) {
    mat logp(values.size(), 1);
    gpak_cv_groups_summary gs;
    GPModel->GroupCV(group, (int)values.size(), LooVals, LooVals_Var, logp, gs);
    postData(X, LooVals, yscale, modelName);
    postData_var(LooVals_Var, yscale, modelName);
    postData(y, yscale, modelName);
    double mse = 0, ym = 0, vy = 0;
    for (size_t i = 0; i < y.n_elem; i++) { mse += (y[i] - LooVals[i]) * (y[i] - LooVals[i]); ym += y[i]; }
    mse /= X.n_rows; ym /= y.n_elem;
    for (size_t i = 0; i < y.n_elem; i++) vy += (y[i] - ym) * (y[i] - ym);
    vy /= y.n_elem;
    if (getVerbose() > 0) {
      std::cout << "Mean Square Error of leave-group-out: " << mse << "\n" << "Var MSE Train: " << vy << "\n"
                << "Mean standardised squared residual: " << gs.mssr << "\n" << "Mean squared Mahalanobis residual: " << gs.msmd << "\n"
                << "Log predictive density of the groups: " << gs.log_pl << "\n" << "Groups: " << gs.groups << "\n"
                << "LGO ms: " << gs.ms << "\n";
    } else { std::cout << mse << "\n" << vy << "\n" << gs.mssr << "\n" << gs.msmd << "\n" << gs.log_pl << "\n"; }
    // rows in input order; the fifth column is what postData_var returns, as StdYh of _predict.txt
    std::ofstream out(LooOut.c_str());
    out << "# SampleNo, Group, Y, Ylgo, StdYlgo, Inputs" << "\n";
    for (size_t i = 0; i < y.n_elem; i++) {
      out << (i + 1) << "\t" << labels[i] << "\t" << y[i] << "\t" << LooVals[i] << "\t" << LooVals_Var[i] << "\t";
      for (size_t j = 0; j < X.n_cols; j++) out << X(i, j) << "\t";
      out << "\n";
    }
    out.close();
    writeTiming(*GPModel);
    delete GPModel;
    exit(0);
  }
  gpak_loo_summary s;
  GPModel->LooCV(LooVals, LooVals_Var, s);
  postData(X, LooVals, yscale, modelName);
  postData_var(LooVals_Var, yscale, modelName);
  postData(y, yscale, modelName);
  double mse = 0, ym = 0, vy = 0;
  for (size_t i = 0; i < y.n_elem; i++) { mse += (y[i] - LooVals[i]) * (y[i] - LooVals[i]); ym += y[i]; }
  mse /= X.n_rows; ym /= y.n_elem;
  for (size_t i = 0; i < y.n_elem; i++) vy += (y[i] - ym) * (y[i] - ym);
  vy /= y.n_elem;
  if (getVerbose() > 0) {
    std::cout << "Mean Square Error of leave-one-out: " << mse << "\n" << "Var MSE Train: " << vy << "\n"
              << "Mean standardised squared residual: " << s.mssr << "\n" << "Log pseudo-likelihood: " << s.log_pl << "\n"
              << "LOO ms: " << s.ms << "\n";
  } else { std::cout << mse << "\n" << vy << "\n" << s.mssr << "\n" << s.log_pl << "\n"; }
  // rows in input order; the fourth column is what postData_var returns, as StdYh of _predict.txt
  std::ofstream out(LooOut.c_str());
  out << "# SampleNo, Y, Yloo, VarYloo, Inputs" << "\n";
  for (size_t i = 0; i < y.n_elem; i++) {
    out << (i + 1) << "\t" << y[i] << "\t" << LooVals[i] << "\t" << LooVals_Var[i] << "\t";
    for (size_t j = 0; j < X.n_cols; j++) out << X(i, j) << "\t";
    out << "\n";
  }
  out.close();
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

void GP_Cntrl::block() {
  incArg();
  setMode("block");
  if (gpus > 1)
    ErrorTermination("gpak_predict_block is built for the single-GPU context (gpak_create) only: drop --gpus");
  bool yscale = true;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if (getArgNo() + 2 >= argc)
    ErrorTermination("There are not enough input parameters: block needs the block centres, the model and the training data.");
  std::string blFile = getArg(), modelName = argv[getArgNo() + 1], trFile = argv[getArgNo() + 2];
  std::string BlockOut = modelName + "_block.txt";
  if (getArgNo() + 3 < argc) BlockOut = argv[getArgNo() + 3];
  int ds[2];
  readDataSize(blFile, ds);
  mat C, y;
  readDataFile(C, y, ds, blFile);
  if (C.n_cols != 3 && C.n_cols != 4) ErrorTermination("Block centres need 3 or 4 input columns.");
  // discretise in the file's units, then standardise every point like a test point: the symmetric standardisation
  // shares one half-range over x, y and z, so a block keeps its shape
  std::vector<double> pts;
  const int nd = gpak_block_points(C.memptr(), C.n_rows, C.n_cols, block_size, block_disc, pts);
  mat Xd(C.n_rows * nd, C.n_cols), ydummy(C.n_rows * nd, 1);
  for (size_t i = 0; i < pts.size(); i++) Xd[i] = pts[i];
  prepareData(C, y, yscale, modelName);            // the model's _Statistics.txt, as `test`
  prepareData(Xd, ydummy, false, modelName);
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // parameters at 6 significant digits (Q5)
  readDataSize(trFile, ds);
  mat Xtr, ytr;
  readDataFile(Xtr, ytr, ds, trFile);
  prepareData(Xtr, ytr, yscale, modelName);
  GPModel->yTarg = ytr;
  GPModel->Xinp = Xtr;
  GPModel->setNumData((unsigned)Xtr.n_rows);
  GPModel->initialize_vars();
  GPModel->logLikelihood();
  if (C.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  mat BlockVals(y.n_rows, 1), BlockVals_Var(y.n_rows, 1);
  GPModel->BlockMeanVar(BlockVals, BlockVals_Var, Xd, nd, block_latent);
  postData(C, BlockVals, yscale, modelName);
  postData_var(BlockVals_Var, yscale, modelName);
  postData(y, yscale, modelName);
  if (getVerbose() > 0)
    std::cout << "Blocks: " << y.n_rows << " of " << nd << " points (" << block_disc[0] << " x " << block_disc[1] << " x "
              << block_disc[2] << ")" << (block_latent ? ", latent variance" : "") << "\n";
  // rows in input order; the fourth column is what postData_var returns, as StdYh of _predict.txt
  std::ofstream out(BlockOut.c_str());
  out << "# BlockNo, Y, Yblock, StdYblock, Inputs" << "\n";
  for (size_t i = 0; i < y.n_elem; i++) {
    out << (i + 1) << "\t" << y[i] << "\t" << BlockVals[i] << "\t" << BlockVals_Var[i] << "\t";
    for (size_t j = 0; j < C.n_cols; j++) out << C(i, j) << "\t";
    out << "\n";
  }
  out.close();
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

// local (not a reference verb): moving-neighbourhood kriging (gpak_predict_local; one GPU only) -- every node from its k
// nearest samples, so train.txt may hold any number of them (train on a subsample, estimate from all the assays):
//   gp_ss_ak --neighbours k [--radius r] [--octant n] [--kriging simple|ordinary] [--search host|device]
//            [--block-size dx,dy,dz --block-disc nx,ny,nz]
//            [--latent] local nodes.txt model train.txt [out]
// nodes.txt is read as block reads its centres (without the two block options the nodes are points); train.txt is
// standardised with the model's _Statistics.txt.  The neighbours are searched from the node centres in the metric of the
// model's first stationary term (gpak_local_metric), in which --radius is measured: 1 is one range.  Everything is checked
// before a context exists.  Written to <model>_local.txt in input order.  --octant n keeps at most n samples from each of
// the eight octants around a node (gpak_local_neighbours_octant; it needs --radius, and 1 <= n <= k).  --kriging ordinary
// re-estimates the mean from every node's own samples (gpak_predict_local_ok) and adds the column LocalMean; a node
// without a sample then has no estimate and prints nan.  --search device takes the lists from the device search
// (gpak_local_neighbours_dev): the same lists, so the same file; the octant search stays on the host.
void GP_Cntrl::local() {
  incArg();
  setMode("local");
  if (gpus > 1)
    ErrorTermination("gpak_predict_local is built for the single-GPU context (gpak_create) only: drop --gpus");
  bool yscale = true;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if (!local_neighbours_set || local_neighbours < 1 || local_neighbours > GPAK_LOCAL_MAX)
    ErrorTermination("local needs --neighbours k, the samples per node, between 1 and 128");
  if (local_radius_set && !(local_radius > 0.0)) ErrorTermination("--radius takes a positive distance (1 is one range of the model's first term)");
  if (block_size_set != block_disc_set)
    ErrorTermination("local takes --block-size and --block-disc together (neither: the nodes are points)");
  if (local_kriging != "simple" && local_kriging != "ordinary") ErrorTermination("--kriging takes simple or ordinary");
  if (local_octant_set && !local_radius_set)
    ErrorTermination("--octant needs --radius: the octant search looks for samples inside a radius only");
  if (local_octant_set && (local_octant < 1 || local_octant > local_neighbours))
    ErrorTermination("--octant takes the samples per octant, between 1 and --neighbours");
  if (local_search != "host" && local_search != "device") ErrorTermination("--search takes host or device");
  if (local_search == "device" && local_octant_set)
    ErrorTermination("--search device does not take --octant: the octant search runs on the host");
  const bool ordinary = local_kriging == "ordinary", search_dev = local_search == "device";
  if (getArgNo() + 2 >= argc)
    ErrorTermination("There are not enough input parameters: local needs the nodes, the model and the samples.");
  std::string ndFile = getArg(), modelName = argv[getArgNo() + 1], trFile = argv[getArgNo() + 2];
  std::string LocalOut = modelName + "_local.txt";
  if (getArgNo() + 3 < argc) LocalOut = argv[getArgNo() + 3];
  const int k = (int)local_neighbours;
  int ds[2];
  readDataSize(ndFile, ds);
  mat C, y;
  readDataFile(C, y, ds, ndFile);
  if (C.n_cols != 3 && C.n_cols != 4) ErrorTermination("Nodes need 3 or 4 input columns.");
  readDataSize(trFile, ds);
  mat Xtr, ytr;
  readDataFile(Xtr, ytr, ds, trFile);
  if (Xtr.n_cols != C.n_cols) ErrorTermination("The samples need the nodes' input columns.");
  // as block: discretise in the file's units, then standardise every point like a test point
  const double point_size[3] = {0, 0, 0};
  const int point_disc[3] = {1, 1, 1};
  std::vector<double> pts;
  const int nd = gpak_block_points(C.memptr(), C.n_rows, C.n_cols, block_size_set ? block_size : point_size,
                                   block_disc_set ? block_disc : point_disc, pts);
  mat Xd(C.n_rows * nd, C.n_cols), ydummy(C.n_rows * nd, 1);
  for (size_t i = 0; i < pts.size(); i++) Xd[i] = pts[i];
  prepareData(C, y, yscale, modelName);            // the model's _Statistics.txt, as `test`
  prepareData(Xd, ydummy, false, modelName);
  prepareData(Xtr, ytr, yscale, modelName);
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // the kernel only: the context gets no training set
  if (C.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  double G[16];
  GPModel->LocalMetric(G);
  std::vector<int> nbr, used;
  const auto t0 = std::chrono::steady_clock::now();
  gpak_local_search_summary ss;
  if (search_dev) GPModel->LocalNeighboursDev(Xtr, C, G, k, local_radius_set ? local_radius : 0.0, nbr, used, ss);
  else if (local_octant_set) GP_utils::LocalNeighboursOctant(Xtr, C, G, k, (int)local_octant, local_radius, nbr, used);
  else GP_utils::LocalNeighbours(Xtr, C, G, k, local_radius_set ? local_radius : 0.0, nbr, used);
  const double search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  mat LocalVals(y.n_rows, 1), LocalVals_Var(y.n_rows, 1), LocalMu(ordinary ? y.n_rows : 0, 1);
  gpak_local_summary s;
  if (ordinary) GPModel->LocalMeanVarOk(LocalVals, LocalVals_Var, LocalMu, Xtr, ytr, Xd, nd, nbr, k, block_latent, s);
  else GPModel->LocalMeanVar(LocalVals, LocalVals_Var, Xtr, ytr, Xd, nd, nbr, k, block_latent, s);
  postData(C, LocalVals, yscale, modelName);
  postData_var(LocalVals_Var, yscale, modelName);
  postData(y, yscale, modelName);
  if (ordinary) postData(LocalMu, yscale, modelName);
  if (getVerbose() > 0)
    std::cout << "Nodes: " << s.nodes << " of " << nd << " points from " << Xtr.n_rows << " samples, " << k << " neighbours at most"
              << (local_octant_set ? ", " + std::to_string(local_octant) + " per octant" : std::string())
              << (ordinary ? ", ordinary kriging" : "")
              << (block_latent ? ", latent variance" : "") << "; without a neighbour " << s.empty << ", not positive definite "
              << s.notpd << "; search " << search_ms << " ms"
              << (search_dev ? " on the device (grid " + std::to_string(ss.grid_ms) + " ms, upload " + std::to_string(ss.upload_ms) +
                                   " ms, search " + std::to_string(ss.search_ms) + " ms)"
                             : std::string())
              << ", device " << (s.upload_ms + s.krige_ms) << " ms\n";
  // rows in input order; the fourth column is what postData_var returns, as StdYblock of _block.txt
  std::ofstream out(LocalOut.c_str());
  out << (ordinary ? "# NodeNo, Y, Ylocal, StdYlocal, Neighbours, LocalMean, Inputs" : "# NodeNo, Y, Ylocal, StdYlocal, Neighbours, Inputs")
      << "\n";
  for (size_t i = 0; i < y.n_elem; i++) {
    if (ordinary && std::isnan(LocalVals[i])) {   // no sample or no factor: `nan` whatever sign the NaN carries
      out << (i + 1) << "\t" << y[i] << "\tnan\tnan\t" << used[i] << "\tnan\t";
    } else {
      out << (i + 1) << "\t" << y[i] << "\t" << LocalVals[i] << "\t" << LocalVals_Var[i] << "\t" << used[i] << "\t";
      if (ordinary) out << LocalMu[i] << "\t";
    }
    for (size_t j = 0; j < C.n_cols; j++) out << C(i, j) << "\t";
    out << "\n";
  }
  out.close();
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

void GP_Cntrl::sim() {
  incArg();
  setMode("sim");
  if (gpus > 1)
    ErrorTermination("gpak_sample_joint is built for the single-GPU context (gpak_create) only: drop --gpus");
  bool yscale = true;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else if (isArg("--method", "--method")) {
        incArg();
        if (getArgNo() >= argc || (getArg() != "joint" && getArg() != "path")) ErrorTermination("--method takes joint or path");
        sim_method = getArg();
      }
      else if (isArg("--features", "--features")) {
        incArg();
        char *end = nullptr;
        const std::string tok = getArgNo() < argc ? getArg() : std::string();
        const long v = strtol(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || v < 1 || v > 1000000) ErrorTermination("--features takes the number of frequencies per stationary term (1 or more)");
        sim_features = (int)v;
      }
      // the verb's own options may also follow it
      else if (isArg("--realisations", "--realizations")) { incArg(); sim_realisations = getIntArg(); sim_realisations_set = true; }
      else if (isArg("--seed", "--seed")) { incArg(); sim_seed = strtoull(getArg().c_str(), nullptr, 10); sim_seed_set = true; }
      else if (isArg("--latent", "--latent")) { block_latent = true; }
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  const bool path = sim_method == "path";
  // what --method path cannot take is refused here, before any file is read and before a context exists
  if (path && !sim_xi_file.empty())
    ErrorTermination("sim --method path draws every normal from --seed (frequencies, amplitudes, noise): drop --xi");
  if (path && sim_nugget_set)
    ErrorTermination("sim --method path factors no covariance of the nodes, so there is nothing for --nugget to regularise: drop --nugget");
  if (path && !sim_seed_set) ErrorTermination("sim --method path needs --seed n");
  if (getArgNo() + 2 >= argc)
    ErrorTermination("There are not enough input parameters: sim needs the nodes, the model and the training data.");
  if (!sim_realisations_set || sim_realisations <= 0) ErrorTermination("sim needs --realisations S with S > 0");
  if (!path && sim_seed_set == !sim_xi_file.empty()) ErrorTermination("sim needs exactly one of --seed n and --xi file");
  if (block_size_set != block_disc_set)
    ErrorTermination("sim takes --block-size and --block-disc together (neither: the nodes are points)");
  std::string ndFile = getArg(), modelName = argv[getArgNo() + 1], trFile = argv[getArgNo() + 2];
  std::string SimOut = modelName + "_sim.txt";
  if (getArgNo() + 3 < argc) SimOut = argv[getArgNo() + 3];
  int ds[2];
  readDataSize(ndFile, ds);
  mat C, y;
  readDataFile(C, y, ds, ndFile);
  if (C.n_cols != 3 && C.n_cols != 4) ErrorTermination("Nodes need 3 or 4 input columns.");
  const size_t M = C.n_rows, S = (size_t)sim_realisations;
  // the normals, M x S column-major: realisation s is column s (--method path draws its own, gp_utils.cpp)
  mat Xi(path ? 0 : M, path ? 0 : S);
  if (path) {
  } else if (!sim_xi_file.empty()) {
    std::ifstream in(sim_xi_file.c_str());
    if (!in.is_open()) ErrorTermination("File is " + sim_xi_file + " not readable");
    std::vector<double> vals;
    size_t rows = 0;
    bool shape_ok = true;
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '#') continue;
      std::istringstream ls(line);
      size_t n = 0;
      double v;
      while (ls >> v) { vals.push_back(v); n++; }
      if (n == 0) continue;
      if (n != S) shape_ok = false;
      rows++;
    }
    if (!shape_ok || rows != M)
      ErrorTermination("--xi needs an M x S matrix: one row per node (" + std::to_string(M) + ") of " + std::to_string(S) + " normals");
    for (size_t i = 0; i < M; i++)
      for (size_t s = 0; s < S; s++) Xi(i, s) = vals[i * S + s];
  } else {
    std::vector<double> z;
    gpak_sim_normals(sim_seed, M * S, z);
    for (size_t i = 0; i < M * S; i++) Xi[i] = z[i];
  }
  // as block: discretise in the file's units, then standardise every point like a test point
  const double point_size[3] = {0, 0, 0};
  const int point_disc[3] = {1, 1, 1};
  std::vector<double> pts;
  const int nd = gpak_block_points(C.memptr(), C.n_rows, C.n_cols, block_size_set ? block_size : point_size,
                                   block_disc_set ? block_disc : point_disc, pts);
  mat Xd(C.n_rows * nd, C.n_cols), ydummy(C.n_rows * nd, 1);
  for (size_t i = 0; i < pts.size(); i++) Xd[i] = pts[i];
  prepareData(C, y, yscale, modelName);            // the model's _Statistics.txt, as `test`
  prepareData(Xd, ydummy, false, modelName);
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // parameters at 6 significant digits (Q5)
  readDataSize(trFile, ds);
  mat Xtr, ytr;
  readDataFile(Xtr, ytr, ds, trFile);
  prepareData(Xtr, ytr, yscale, modelName);
  GPModel->yTarg = ytr;
  GPModel->Xinp = Xtr;
  GPModel->setNumData((unsigned)Xtr.n_rows);
  GPModel->initialize_vars();
  GPModel->logLikelihood();
  if (C.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  mat MeanVals(M, 1), SimVals(M, S);
  gpak_condition_summary ps = {0.0, 0.0, 0.0, 0, 1};
  if (path) {
    if (!GPModel->PathSample(SimVals, MeanVals, Xd, nd, sim_seed, sim_features, block_latent, ps))
      std::cerr << "The training factor failed: the realisations are NaN" << std::endl;
  } else if (!GPModel->JointSample(SimVals, MeanVals, Xd, nd, Xi, sim_nugget, block_latent))
    std::cerr << "The joint covariance of the nodes is not positive definite: the realisations are NaN (try --nugget)" << std::endl;
  postData(C, MeanVals, yscale, modelName);
  postData(SimVals, yscale, modelName);
  postData(y, yscale, modelName);
  if (getVerbose() > 0 && path)
    std::cout << "Nodes: " << M << " of " << nd << " points, " << S << " realisations" << (block_latent ? ", latent" : "")
              << ", spectral prior of " << sim_features << " frequencies per term (its covariance is the prior's to O(1/sqrt(F)); "
              << "the conditioning on the data is exact); device ms: solves " << ps.solve_ms << ", prior " << ps.prior_ms
              << ", product " << ps.product_ms << " in " << ps.batches << " batch(es)\n";
  else if (getVerbose() > 0)
    std::cout << "Nodes: " << M << " of " << nd << " points, " << S << " realisations"
              << (block_latent ? ", latent" : "") << ", nugget " << sim_nugget << "\n";
  std::ofstream out(SimOut.c_str());
  out << "# NodeNo, Y, Ymean";
  for (size_t s = 0; s < S; s++) out << ", Sim" << (s + 1);
  out << ", Inputs" << "\n";
  for (size_t i = 0; i < M; i++) {
    out << (i + 1) << "\t" << y[i] << "\t" << MeanVals[i] << "\t";
    for (size_t s = 0; s < S; s++) out << SimVals(i, s) << "\t";
    for (size_t j = 0; j < C.n_cols; j++) out << C(i, j) << "\t";
    out << "\n";
  }
  out.close();
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

void GP_Cntrl::design() {
  incArg();
  setMode("design");
  if (gpus > 1)
    ErrorTermination("gpak_design is built for the single-GPU context (gpak_create) only: drop --gpus");
  bool yscale = true;
  std::string candFile, holeFile;
  while (isFlgs()) {
    if (isArgFlg()) {
      if (isArg("-?", "--?") || isArg("-h", "--help")) { Help(); exit(0); }
      else if (isArg("-np", "--no-prompt")) { no_prompt = true; }
      else if (isArg("--candidates", "--candidates")) {
        incArg();
        if (getArgNo() >= argc) ErrorTermination("--candidates takes a file of candidate points");
        candFile = getArg();
      }
      else if (isArg("--holes", "--holes")) {
        incArg();
        if (getArgNo() >= argc) ErrorTermination("--holes takes a file of labels");
        holeFile = getArg();
      }
      else UnkFlg();
      incArg();
    } else setFlgs(false);
  }
  if (candFile.empty() || holeFile.empty())
    ErrorTermination("design needs --candidates FILE (the candidate points) and --holes FILE (one integer label per candidate point)");
  if (block_size_set != block_disc_set)
    ErrorTermination("design takes --block-size and --block-disc together (neither: the targets are points)");
  if (getArgNo() + 2 >= argc)
    ErrorTermination("There are not enough input parameters: design needs the targets, the model and the training data.");
  std::string tgFile = getArg(), modelName = argv[getArgNo() + 1], trFile = argv[getArgNo() + 2];
  const std::string DesignOut = modelName + "_design.txt";
  int ds[2];
  readDataSize(tgFile, ds);
  mat C, y;
  readDataFile(C, y, ds, tgFile);
  if (C.n_cols != 3 && C.n_cols != 4) ErrorTermination("Targets need 3 or 4 input columns.");
  readDataSize(candFile, ds);
  mat Xc, yc;
  readDataFile(Xc, yc, ds, candFile);              // the last column is read and ignored
  if (Xc.n_cols != C.n_cols) ErrorTermination("--candidates: the candidate points need the targets' input columns.");
  const size_t T = C.n_rows, Mc = Xc.n_rows;
  // the labels with the checks of `cv --groups`, in the words of this verb
  std::vector<long long> labels, values;
  readGroupLabels(holeFile, labels, "--holes");
  if (labels.size() != Mc)
    ErrorTermination("--holes: " + holeFile + " holds " + std::to_string(labels.size()) + " labels for " + std::to_string(Mc) +
                     " candidate points");
  values = labels;
  std::sort(values.begin(), values.end());
  values.erase(std::unique(values.begin(), values.end()), values.end());
  std::vector<int> hole(Mc), count(values.size(), 0);
  for (size_t i = 0; i < Mc; i++) {
    hole[i] = (int)(std::lower_bound(values.begin(), values.end(), labels[i]) - values.begin());
    if (++count[hole[i]] == GPAK_CV_GROUP_MAX + 1)
      ErrorTermination("--holes: hole " + std::to_string(labels[i]) + " has more than " + std::to_string(GPAK_CV_GROUP_MAX) +
                       " points (the design holds a hole in one workgroup's memory)");
  }
  const int H = (int)values.size();
  if (design_pick > H)
    ErrorTermination("--pick: " + std::to_string(design_pick) + " holes to plan out of " + std::to_string(H));
  std::vector<double> wt;
  if (!design_weights_file.empty()) {
    std::ifstream in(design_weights_file.c_str());
    if (!in.is_open()) ErrorTermination("File is " + design_weights_file + " not readable");
    std::string line;
    while (std::getline(in, line)) {
      if (!line.empty() && line[0] == '#') continue;
      for (char &ch : line) if (ch == '\t' || ch == ',' || ch == '\r') ch = ' ';
      std::istringstream ss(line);
      std::string tok;
      while (ss >> tok) {
        char *end = nullptr;
        const double v = strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end != '\0' || !(v >= 0.0) || !std::isfinite(v))
          ErrorTermination("--weights: '" + tok + "' in " + design_weights_file + " is not a non-negative number");
        wt.push_back(v);
      }
    }
    if (wt.size() != T)
      ErrorTermination("--weights: " + design_weights_file + " holds " + std::to_string(wt.size()) + " weights for " +
                       std::to_string(T) + " targets");
  }
  // as block: discretise in the file's units, then standardise every point like a test point
  const double point_size[3] = {0, 0, 0};
  const int point_disc[3] = {1, 1, 1};
  std::vector<double> pts;
  const int nd = gpak_block_points(C.memptr(), C.n_rows, C.n_cols, block_size_set ? block_size : point_size,
                                   block_disc_set ? block_disc : point_disc, pts);
  mat Xd(C.n_rows * nd, C.n_cols), ydummy(C.n_rows * nd, 1);
  for (size_t i = 0; i < pts.size(); i++) Xd[i] = pts[i];
  prepareData(Xd, ydummy, false, modelName);       // the model's _Statistics.txt, as `test`
  prepareData(Xc, yc, false, modelName);
  GP_utils *GPModel = readGpFromFile(modelName, getVerbose());  // parameters at 6 significant digits (Q5)
  readDataSize(trFile, ds);
  mat Xtr, ytr;
  readDataFile(Xtr, ytr, ds, trFile);
  prepareData(Xtr, ytr, yscale, modelName);
  GPModel->yTarg = ytr;
  GPModel->Xinp = Xtr;
  GPModel->setNumData((unsigned)Xtr.n_rows);
  GPModel->initialize_vars();
  GPModel->logLikelihood();
  if (C.n_cols != GPModel->getInpDim()) ErrorTermination("Incorrect dimension of input data.");
  std::vector<double> gain, pick_gain;
  std::vector<int> picked;
  gpak_design_summary s;
  if (!GPModel->DesignHoles(Xd, nd, Xc, hole, H, wt.empty() ? nullptr : wt.data(), design_pick, gain, picked, pick_gain, s))
    std::cerr << "The covariance of a candidate hole's assays is not positive definite: its gain is NaN" << std::endl;
  // variances in the units of the model's standardised grade; Share and Pick carry no unit
  std::cout << "Targets: " << T << " of " << nd << " points, candidate holes: " << H << " (" << Mc << " points, the largest "
            << s.max_size << ")\nvar_before " << s.var_before << "  var_after " << s.var_after << "  device time " << s.ms
            << " ms\n";
  std::vector<int> rank((size_t)H, 0);
  for (int p = 0; p < s.picks; p++) {
    rank[picked[p]] = p + 1;
    std::cout << "pick " << (p + 1) << ": hole " << values[picked[p]] << "  conditional gain " << pick_gain[p] << "\n";
  }
  std::ofstream out(DesignOut.c_str());
  out << "# Hole, Samples, Gain, Share, Pick" << "\n";
  for (int h = 0; h < H; h++) {
    out << values[h] << "\t" << count[h] << "\t" << gain[h] << "\t" << gain[h] / s.var_before << "\t" << rank[h];
    if (rank[h]) out << "\t" << pick_gain[rank[h] - 1];
    out << "\n";
  }
  out.close();
  writeTiming(*GPModel);
  delete GPModel;
  exit(0);
}

int main(int argc, char **argv) {
  GP_Cntrl ctl(argc, argv);
  if (ctl.getArgNo() >= argc) { ctl.Help(); return 1; }
  std::string verb = ctl.getArg();
  if (verb != "local" && verb != "-h" && verb != "--help" && verb != "-?") ctl.localOptionsOnlyWithLocal();
  if (verb == "train") ctl.train();
  else if (verb == "test") ctl.test();
  else if (verb == "cv") ctl.cv();
  else if (verb == "block") ctl.block();
  else if (verb == "sim") ctl.sim();
  else if (verb == "design") ctl.design();
  else if (verb == "local") ctl.local();
  else if (verb == "-h" || verb == "--help" || verb == "-?") { ctl.Help(); return 0; }
  else ctl.ErrorTermination("Invalid command provided.");
  return 0;
}
