// ctx_state.h -- what of a single-GPU context's device contents is current.  Plain C++, nothing of HIP (as potrf_plan.h):
// tests/ctx_state_driver.cpp replays event lists through it on the CPU, against tests/ctx_model.py::CachingModel.
//
// The facts form a ladder.  The transformed training points U stand under the factor in dM, the factor under alpha, alpha
// under the nlZ terms; three side facts hang off the factor.  Dropping a rung drops everything above it and the side facts
// of what was dropped.  The members below are the EVENTS of api.hip / potrf.hip / predict.hip, named for what happened;
// nothing else writes a fact.
#pragma once

struct CtxState {
  enum Rung { NONE, FACTOR, ALPHA, NLZ };
  // what gpak_backsolve (solve.hip) may use with the current factor
  enum Backsolve {
    BS_BLOCKS128,            // the inverted 128-blocks only
    BS_INV_STEP,             // explicit inverses in dInv512, three launches per step (bwd_fused 0)
    BS_INV_FAR,              // ... far column dots under the diagonal step (bwd_fused 1)
    BS_RT                    // [R_b ; T_b] in dT512, one launch per step (bwd_fused 2)
  };

  // -- the facts (read-only outside this struct) --
  bool points = false;       // U holds the training points under the stored kernel.  A flag beside the rungs and not the
                             // lowest of them, because an IMPORTED factor stands without them
  Rung rung = NONE;          // the highest of factor / alpha / nlZ terms that is current
  bool z = false;            // side fact: dWork[Np..2Np) holds L^-1 (y/sn2)
  Backsolve backsolve = BS_BLOCKS128;   // side fact
  bool image = false;        // side fact: the fp32 image of the factor (GPAK_F32 prediction) is current
  int failed_col = 0;        // first failing column (1-based) of the last factorisation, 0: it succeeded
  int factorisations = 0;    // since the last training set (gpak_phase_times::evaluations)
  bool memoise = false;      // GPAK_OPT_MEMOISE: an identical gpak_set_params is the event same_kernel

  bool has(Rung r) const { return rung >= r; }

  // -- the events --
  void set_memoise(bool on) { memoise = on; }
  void new_training_set() { points = false; drop_factor(); factorisations = 0; }
  void new_kernel() { points = false; drop_factor(); }   // GP_Utils.cpp:132-133: setKUpdateStat(false)
  void same_kernel() {}                                  // memoised: everything stands
  void points_built() { points = true; }
  void matrix_overwritten() { drop_factor(); }           // gpak_gram: dM holds K
  void factorisation_started() { drop_factor(); factorisations++; }
  // the explicit inverses are built beside the forward substitution only (gpak_potrf_plan)
  void factorisation_succeeded(bool fwd_in_factor, bool inv512, int bwd_fused) {
    rung = FACTOR;
    z = fwd_in_factor;
    backsolve = !(fwd_in_factor && inv512) ? BS_BLOCKS128 : bwd_fused == 2 ? BS_RT : bwd_fused == 1 ? BS_INV_FAR : BS_INV_STEP;
    failed_col = 0;
  }
  void factorisation_failed(int col) { drop_factor(); failed_col = col; }
  // gpak_import_factor: the 128-blocks, alpha and the nlZ terms of a group's rank; no wider inverses, no image, no z
  void factor_imported() { drop_factor(); rung = NLZ; failed_col = 0; }
  void work_vectors_overwritten() { z = false; }         // a back substitution or gpak_solve_chol used dWork
  void alpha_built() { rung = ALPHA; }
  void nlz_built() { rung = NLZ; }
  void image_built() { image = true; }

 private:
  void drop_factor() { rung = NONE; z = false; backsolve = BS_BLOCKS128; image = false; }
};
