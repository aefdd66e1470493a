// dist_core.h -- what the two multi-GPU rank types have in common: gpak_dist (dist.hip, block-column-cyclic) and
// gpak_grid (grid.hip, row-block x column-block) both derive from RankCore.  The core holds the engine / transport
// tables, the replicated vectors, parameters, results, statistics and the event pools, and every step that does not
// depend on the layout is a function over it (defined in dist.hip, next to the built-in HIP engine and the RCCL binding
// they use).  The schedules themselves -- who owns what, which stream carries what -- stay with the layouts.
#ifndef GPAK_DIST_CORE_H
#define GPAK_DIST_CORE_H
#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/gpak_dev.h"
#include "../../include/gpak_dist.h"
#include "gpak_internal.h"

#pragma GCC visibility push(hidden)   // shared between two translation units, not exported from the library

struct HipEngineState {
  int device = 0;
  int cu_mask_skip = 8;
  bool mask_failed = false;
};

// built-in RCCL transport: the world communicator, and for a process grid its row and column communicators
// (indexed by GPAK_GROUP_ROW / GPAK_GROUP_COL)
struct RcclTransport {
  void *comm[3] = {nullptr, nullptr, nullptr};
  int world = 1;
};

struct RankCore {
  int rank = 0, P = 1, device = 0;
  gpak_dist_engine E;
  gpak_dist_transport T;
  HipEngineState hip_state;
  RcclTransport rccl_state;
  bool builtin_engine = false, builtin_transport = false;
  std::string err;
  void *s_bulk = nullptr, *s_panel = nullptr;
  int flags = 0;                      // GPAK_DIST_FLAG_* (only the 1-D schedule ever sets one)

  // problem
  int N = 0, Np = 0, nb = 512, nJ = 0, cap = 0;
  double xsum[4] = {0, 0, 0, 0};
  int d = 3;                          // input columns: 3, or 4 with a rock-type column
  double *x_soa = nullptr, *y = nullptr, *u = nullptr, *scratch = nullptr, *small = nullptr, *alpha = nullptr;
  double *rhs = nullptr, *f = nullptr, *ld_slots = nullptr, *bwd_scratch = nullptr;
  int *info = nullptr;

  // parameters
  bool have_params = false;
  double expans[8] = {0}, bias = 0, sn2 = 0;
  int mode = GPAK_DIST_DIRECT;
  bool hyb = false;                         // a general composition (gpak_dist_set_kernel): `kern` is what the engine gets
  double kern[GPAK_KERN_SERIAL_MAX] = {0};  // serialized: children, kinds, Sigma_White, parameters (gpak_dev.h)
  double white = 0;

  // results
  bool have_result = false;
  double quad = 0, sumlp = 0, logdet = 0, nlz = 0;
  int failed_col = 0;                 // 1-based failing column of the last factorisation, min-reduced: the same on every rank
  gpak_dist_stats stats;

  // event pools, and the time stamps of the current step
  std::vector<void *> ev_sync, ev_time;
  size_t sync_used = 0, time_used = 0;
  struct Span { size_t e0, e1; int kind; };   // kind 0 bulk, 1 chain, 2 comm
  std::vector<Span> spans;
  bool profile = true;
  double t_start = 0;
  size_t tp[5] = {0, 0, 0, 0, 0};     // fill | factor | solve | nlZ | end, on the bulk stream

  int kmode() const { return mode | (d == 4 ? GPAK_DIST_D4 : 0) | (hyb ? GPAK_DIST_HYB : 0); }   // what the engine calls get
  const double *kpars() const { return hyb ? kern : expans; }
  int width(int b) const { return std::min(nb, Np - b * nb); }
  int start(int b) const { return b * nb; }

  void *sync_event() {
    if (sync_used == ev_sync.size()) ev_sync.push_back(E.event_create(E.self, 0));
    return ev_sync[sync_used++];
  }
  size_t time_event(void *stream) {
    if (time_used == ev_time.size()) ev_time.push_back(E.event_create(E.self, 1));
    E.event_record(E.self, ev_time[time_used], stream);
    return time_used++;
  }
};

// the one status check: `h` is the rank at hand
#define RCHK(call)                                                                    \
  do {                                                                                \
    int rc_ = (call);                                                                 \
    if (rc_ != GPAK_OK) {                                                             \
      h->err = std::string(#call) + " failed with status " + std::to_string(rc_);     \
      return rc_ < 0 ? rc_ : GPAK_EHIP;                                               \
    }                                                                                 \
  } while (0)

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- handle -----------------------------------------------------------------------------------------------------
// engine == NULL: the built-in HIP engine on `device` (GPAK_EHIP without one: there is no CPU fallback); with
// `cu_mask` its bulk stream leaves GPAK_DIST_MASK (default 8) compute units idle.  transport == NULL: the RCCL one.
int core_attach(RankCore *h, int rank, int world, int device, const gpak_dist_engine *engine,
                const gpak_dist_transport *transport, bool cu_mask);
void core_set_device(RankCore *h);
void core_release(RankCore *h);        // the replicated vectors; N = 0
void core_detach(RankCore *h);         // events and communicators (the streams are the layout's to destroy first)
// ncclCommInitRank on a helper thread with a bounded wait (GPAK_RCCL_INIT_TIMEOUT_S); Pr > 0: then the row and column
// communicators of a Pr x P/Pr grid (ncclCommSplit).  Any failure leaves the handle with no communicator at all.
int core_init_rccl(RankCore *h, const char *id, int Pr);

// ---- training set and parameters --------------------------------------------------------------------------------
int core_train_check(RankCore *h, const double *X, const double *y, int N, int d, int *nb);   // + device, h->d
bool core_train_alloc(RankCore *h, int N, int nb);   // N, Np, nb, nJ, cap and the replicated vectors; false: out of memory
int core_train_upload(RankCore *h, const double *X, const double *y);   // X, y, column sums; alpha = small = 0; stats header
int core_set_params(RankCore *h, const double *expans, double bias, double sn2, int dist_mode);

// ---- one step ---------------------------------------------------------------------------------------------------
int core_step_transform(RankCore *h);  // pools and stats reset, tp[0], pooled mean, transform / transform_k
// after the layout's factorisation: the failing column, tp[2]; GPAK_ENOTPD (Chol_fail) when there is one
int core_step_factored(RankCore *h, int failed_col);
// event edge `from` -> `to`; nothing when they are the same stream
int core_hop(RankCore *h, void *from, void *to);
// a diagonal block for the log-determinant: logdiag_block(a, ld, J, W)
struct DiagBlock { const double *a; long ld; int J, W; };
// From f = K alpha to the filled statistics.  The collectives go to `s_coll`: the 1-D rank's communication stream
// (ordered against the bulk stream by core_hop), or the bulk stream itself.  tp[1..3] are the layout's.
int core_step_finish(RankCore *h, void *s_coll, const std::vector<DiagBlock> &diag, double *nlz);
int core_nlz_terms(RankCore *h, double *quad, double *sumlp, double *logdet);   // of a finished step
int core_get_alpha(RankCore *h, double *alpha_host);
int core_get_stats(RankCore *h, gpak_dist_stats *out);

// The start of a step: transform, the layout's fill of B = I + K/sn2, rhs = y / sn2.
template <class Fill> int core_step_begin(RankCore *h, Fill fill) {
  int rc = core_step_transform(h);
  if (rc == GPAK_OK) rc = fill();
  if (rc) return rc;
  RCHK(h->E.vec_scale(h->s_bulk, h->Np, h->y, 1.0 / h->sn2, h->rhs));
  return GPAK_OK;
}

#pragma GCC visibility pop
#endif
