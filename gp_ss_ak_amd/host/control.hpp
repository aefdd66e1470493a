// control.hpp -- argument walker, data reader and (de)standardisation of the reference's
// Control class (Control.h:23-169, Control.cpp:5-337): host glue around the hot path.
#pragma once
#include <string>

#include "gpak_mat.hpp"

using gpak_host::mat;

class Control {
 public:
  Control(int argc, char **argv);
  virtual ~Control() {}
  bool isArg(const std::string &shortName, const std::string &longName) const;
  bool isArgFlg() const { return argNo < argc && argv[argNo][0] == '-'; }
  bool isFlgs() const { return flgs && argNo < argc; }
  void setFlgs(bool v) { flgs = v; }
  void incArg() { argNo++; }
  int getArgNo() const { return argNo; }
  std::string getArg() const { return argNo < argc ? argv[argNo] : ""; }
  int getIntArg() const { return atoi(getArg().c_str()); }
  size_t getArgLen() const { return getArg().size(); }
  void UnkFlg() const;
  void setMode(const std::string &m) { mode = m; }
  std::string getMode() const { return mode; }
  int getVerbose() const { return verbose; }

  // last column = y, separators tab or comma, '#' comment lines (Control.cpp:27-141)
  void readDataSize(const std::string &file, int data_size[2]) const;
  void readDataFile(mat &X, mat &y, const int data_size[2], const std::string &file) const;
  // prepareM: 0 mean/std, 1 symmetric (default), 2 zero-and-one (Control.cpp:142-324)
  void prepareData(mat &X, mat &y, bool yscale, const std::string &ModelN);
  void postData(mat &X, mat &y, bool yscale, const std::string &ModelN);
  void postData(mat &y, bool yscale, const std::string &ModelN);
  void postData_var(mat &v, bool yscale, const std::string &ModelN);
  void ErrorTermination(const std::string &error) const;

  int argc;
  char **argv;

 protected:
  void loadStatistics(const std::string &ModelN, size_t d);
  int argNo = 1;
  bool flgs = true;
  int verbose = 0;
  int prepareM = 1;
  bool no_prompt = false;
  int gpus = 1;                  // --gpus n: block-column-cyclic multi-GPU context (gpak_create_multi)
  int precision = 0;             // --precision f64|f32: GPAK_F64 / GPAK_F32 (fp32 prediction work)
  bool exact_gradient = false;   // --gradient reference|exact: GradLL as the reference writes it / the derivative of nlZ
  bool gradient_set = false;     // --gradient was given (an explicit `reference` cannot go with --objective loo / lgo)
  bool loo_objective = false;    // --objective nlz|loo: train on nlZ / on -log_pl of the leave-one-out predictions (gpak_loo_grad)
  bool lgo_objective = false;    // --objective lgo: on -log_pl of the leave-group-out predictions (gpak_cv_groups_grad; train --groups FILE)
  std::string timing_file;       // --timing file|-: JSON of gpak_phase_times after the verb
  // the `block` verb: --block-size dx,dy,dz (the file's units), --block-disc nx,ny,nz, --latent (no sn2 / nd)
  double block_size[3] = {0, 0, 0};
  int block_disc[3] = {1, 1, 1};
  bool block_latent = false;
  bool block_size_set = false, block_disc_set = false;
  // the `sim` verb: --realisations S, --seed n | --xi file (M x S normals), --nugget v (added to the covariance's diagonal)
  int sim_realisations = 0;
  bool sim_realisations_set = false, sim_seed_set = false;
  unsigned long long sim_seed = 0;
  std::string sim_xi_file;
  double sim_nugget = 0.0;
  bool sim_nugget_set = false;
  // sim --method joint (gpak_sample_joint, the default) | path (gpak_sample_path: any node count), --features F per stationary term
  std::string sim_method = "joint";
  int sim_features = 4096;
  // the `design` verb: --pick k (a greedy plan of k holes), --weights file (one non-negative number per target)
  int design_pick = 0;
  std::string design_weights_file;
  // the `local` verb: --neighbours k (1..128 samples per node), --radius r (in ranges of the model's first term)
  long local_neighbours = 0;
  double local_radius = 0.0;
  bool local_neighbours_set = false, local_radius_set = false;
  // --kriging simple|ordinary (ordinary: gpak_predict_local_ok), --octant n (at most n samples per octant; needs --radius)
  std::string local_kriging = "simple";
  long local_octant = 0;
  bool local_kriging_set = false, local_octant_set = false;
  // --search host|device (device: the lists come from gpak_local_neighbours_dev; the octant search stays on the host)
  std::string local_search = "host";
  bool local_search_set = false;
  std::string mode = "gp";
  mat params, MinData, MaxData, MeanData, StData;
  double MaxTotalin = 0, MinTotalin = 0, MaxTotalo = 0, MinTotalo = 0;
};
