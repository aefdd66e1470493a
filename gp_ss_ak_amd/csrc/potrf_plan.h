// potrf_plan.h -- the schedule of the single-GPU blocked Cholesky (gpak_potrf_blocked, potrf.hip) as data.
// Plain C++17, no HIP: gpak_potrf_plan() is a pure function of the padded size, the context's schedule set and the
// queues the context has, so the schedule can be printed and checked on a machine without a GPU
// (tests/test_potrf_plan.py).  potrf.hip only executes the steps: every threshold lives here.
#pragma once
#include <algorithm>
#include <vector>

#define GPAK_TILE 128       // every matrix dimension on the device is padded to this
#define GPAK_PANEL_MID 512  // panels wider than this are factored in pieces of this width (potrf.hip)

// ---- tuning, part 1: the schedule set -----------------------------------------------------------------------
// The knobs that are read through a CONTEXT.  The process-wide defaults below (each the measured best at N = 32768
// on MI355X, DESIGN.md sections 4.1-4.4) are overridden once, at the first use, by the GPAK_* environment variables
// of the same names (A/B tooling; gpak_reload_tuning() re-reads them).  gpak_create copies the set into the context,
// gpak_set_option changes that copy only, and nothing but the context's copy is ever read.
// (Part 2, what the context-free kernel launchers read, is GpakKernelTuning in gpak_internal.h.)
struct GpakSchedule {
  // gpak_potrf_plan
  int nb_outer = 512;          // GPAK_NB_OUTER      outer panel width
  int nb_wide = 1024;          // GPAK_NB_WIDE       panel width while more than nb_wide_rows rows are left (0: off)
  int nb_wide_rows = 16384;    // GPAK_NB_WIDE_ROWS
  int nb_xwide = 2048;         // GPAK_NB_XWIDE      ... and while more than nb_xwide_rows rows are left (0: off)
  int nb_xwide_rows = 32768;   // GPAK_NB_XWIDE_ROWS
  bool first_narrow = true;    // GPAK_FIRST_NARROW  the very first panel is nb_outer wide
  int tail_rows = 12288;       // GPAK_TAIL_ROWS     rows left from which the bulk updates use the CU-masked queue
  bool sub_next = false;       // GPAK_SUB_NEXT      tail: next block column updated sub-panel by sub-panel
  int next_split_rows = 0;     // GPAK_NEXT_SPLIT_ROWS  rows left from which only the first 128 columns of the next block column are
                               //                    updated in the panel chain, the others beside the next panel's first step (0: off)
  bool inv512 = true;          // GPAK_INV512        explicit diagonal-block inverses for the back substitution
  int bwd_fused = 2;           // GPAK_BWD_FUSED     back substitution: 0 three launches per step, 1 far column dots under the diagonal
                               //                    step (two launches), 2 one launch (coupling blocks T_b): solve.hip
  bool lookahead = true;       // GPAK_LOOKAHEAD     0: everything on one stream
  bool fwd_in_factor = true;   // GPAK_FWD_IN_FACTOR forward substitution of y/sn2 rides along with the factorisation
  // gpak_potrf_blocked, gpak_create, gpak_set_train
  int bwd_block = 512;         // GPAK_BWD_BLOCK     ... of this width: 512, 1024 or 2048 columns per back-substitution step
                               //                    (measured round 3: solve 1.72 / 1.42 / 1.33 ms at N = 32768, but the wider inverses cost
                               //                    the factorisation as much or more: profiles/r03_bwd_block.txt)
  int potrf_co = 1;            // GPAK_POTRF_CO      0 always the 8-wave block kernel, 2 always the 4-wave one, 1 as asked
  int tail_mask = 8;           // GPAK_TAIL_MASK     compute units the tail's bulk queue leaves idle (0: no such queue)
  int tail_mask_stride = 1;    // GPAK_TAIL_MASK_STRIDE
  bool bulk_queue = true;      // GPAK_BULK_QUEUE    bulk updates on a queue made by hipExtStreamCreateWithCUMask
  long ld_pad = -1;            // GPAK_LD_PAD        leading-dimension skew in doubles (-1: 32 from Np = 1024 on)
  bool bulk_tickets = true;    // GPAK_BULK_TICKETS  factorisation's bulk update: tiles claimed per XCD at run time (0: static blockIdx map)
  int bulk_surplus = 6;        // GPAK_BULK_SURPLUS  ... with this many percent more workgroups than tiles
  int tail_queue_max_np = 0;   // GPAK_TAIL_MAX_NP   padded sizes above this factor without the CU-masked tail queue (0: no limit);
                               //                    read by gpak_potrf_caps, not by the plan
  // prediction
  int fs_levels[8] = {128, 512, 2048, 8192, 0, 0, 0, 0};   // GPAK_FS_LEVELS_F32  ladder of the substitution with many right-hand sides (fp32 and fp64 prediction)
  int pred_batch = 0;          // GPAK_PRED_BATCH    test points per batch (0: 16384 fp64, 65536 fp32)
  int pred_ld_skew = 1;        // GPAK_PRED_LD_SKEW  leading dimensions of the test-major batch and of the fp32 factor image
                               //                    are skewed by this many 256-byte units (0: powers of two, as in round 2)
};

// Which of the optional queues the context has (look-ahead itself is GpakSchedule::lookahead; without it nothing
// below is used and the panel, substitution and update roles all collapse onto the main stream).
struct PotrfCaps {
  bool tail_queue = false;   // CU-masked copy of the main stream (gpak_ctx::stream_tail)
  bool bulk_queue = false;   // the bulk updates' own queue (gpak_ctx::stream_bulk)
  bool side_stream = false;  // gpak_ctx::stream_x
};

// What gpak_potrf_blocked hands to the plan as "the queues the context has": the streams that exist, less the tail
// queue where the schedule set withholds it by matrix size (GpakSchedule::tail_queue_max_np).  Without the tail queue
// the plan keeps every bulk update on the bulk queue and every later panel beside_bulk.  The only place this rule lives.
inline PotrfCaps gpak_potrf_caps(int Np, const GpakSchedule &s, bool have_tail, bool have_bulk, bool have_side) {
  PotrfCaps caps;
  caps.tail_queue = have_tail && (s.tail_queue_max_np <= 0 || Np <= s.tail_queue_max_np);
  caps.bulk_queue = have_bulk;
  caps.side_stream = have_side;
  return caps;
}

// One panel b = columns [J, J + W) and everything its factorisation triggers.  With J1 = J + W:
//   panel stream :  F(b) | update of the next panel's columns [J1, J2) | F(b+1) ...
//   bulk queue   :         update of [J2, Np) with panel b (after F(b)), in the order of b
struct PotrfStep {
  int J = 0, W = 0;
  int J2 = 0;                 // end of the next panel (Np when there is none)
  // how the panel is factored
  bool tail_panel = false;    // factor_panel_tail: the next block column is updated per 128-column sub-panel on the side stream
  bool beside_bulk = false;   // (not tail_panel) the bulk update of panel b-1 runs beside it: only the 4-wave block kernel fits
  // how the next block column [J1, J2) gets this panel's update
  enum Next { NEXT_NONE,      // last panel
              NEXT_PANEL,     // one K = W product on the panel stream
              NEXT_SPLIT,     // first 128 columns there, the rest on the side stream; the next panel's first in-panel update waits (gate)
              NEXT_DONE       // tail_panel already applied it
  } next = NEXT_NONE;
  // the bulk update of [J2, Np)
  enum Queue { Q_NONE, Q_MAIN, Q_BULK, Q_TAIL } bulk = Q_NONE;
  int ticket = -1;            // its index in the ticket ring (eight list words each) = its number among the bulk updates
  // the bwd_bw-wide diagonal blocks [inv_begin, inv_end) are complete after this panel: their explicit inverses
  // become due (empty unless fwd_in_factor and inv512)
  int inv_begin = 0, inv_end = 0;
};

inline std::vector<PotrfStep> gpak_potrf_plan(int Np, const GpakSchedule &s, const PotrfCaps &caps, int bwd_bw) {
  const int PB = GPAK_TILE;
  const int NB = std::max(s.nb_outer, PB) / PB * PB;
  // Panel widths.  While the trailing matrix is large the bulk update hides any panel chain, and a wider panel makes
  // it more efficient (K = 1024: 73.7 TFLOP/s in the kernel, K = 512: 71.4); later the narrower panel keeps the chain
  // short (N=32768: 180.8 -> 178.5 ms).  A third tier for trailing matrices beyond N = 32768: 2048-column panels while
  // more than 32768 rows are left (N=65536: 1295.0 -> 1285.5 ms, tools/time_sizes.py; nothing changes at N <= 32768).
  // A tier only applies when it is wider than the one below it.
  const int nb_wide = s.nb_wide / PB * PB, nb_xwide = s.nb_xwide / PB * PB;   // 0: off
  std::vector<PotrfStep> plan;
  for (int J = 0; J < Np;) {
    // the very first panel has nothing to hide behind: keep it narrow so that the first bulk update starts early
    // (measured at N=32768, 30-step A/B inside one box: 182.46 -> 181.90 ms)
    const bool first = s.first_narrow && J == 0;
    const int W = (nb_xwide > NB && nb_xwide > nb_wide && Np - J > s.nb_xwide_rows && !first) ? nb_xwide
                  : (nb_wide > NB && Np - J > s.nb_wide_rows && !first)                       ? nb_wide
                                                                                              : NB;
    PotrfStep st;
    st.J = J;
    st.W = std::min(W, Np - J);
    plan.push_back(st);
    J += W;
  }
  const bool la = s.lookahead, side = la && caps.side_stream;
  int done = 0, bulk = 0;
  for (size_t b = 0; b < plan.size(); b++) {
    PotrfStep &st = plan[b];
    const int J1 = st.J + st.W, J2 = b + 1 < plan.size() ? J1 + plan[b + 1].W : Np;
    st.J2 = J2;
    // sub-panel updates of the next block column in the tail: measured 183.07 -> 183.73 ms at N=32768 -- the four
    // K=128 products re-read and re-write the column four times and the chain gains nothing measurable; off unless
    // GPAK_SUB_NEXT=1 (kept: the multi-GPU schedule is built the same way and tests compare)
    st.tail_panel = s.sub_next && side && st.W <= GPAK_PANEL_MID && J1 < Np && Np - J1 <= s.tail_rows;
    // on the unmasked queue the bulk update of panel b-1 holds two 210-VGPR waves on every SIMD of the chip, and only
    // the 4-wave, 80-VGPR potrf128 fits beside it
    st.beside_bulk = !st.tail_panel && la && b > 0 && !(caps.tail_queue && Np - J1 <= s.tail_rows);
    st.inv_begin = done;
    if (s.fwd_in_factor && s.inv512)
      while (done * bwd_bw < Np && std::min(Np, (done + 1) * bwd_bw) <= J1) done++;
    st.inv_end = done;
    if (J1 >= Np) break;
    // GPAK_NEXT_SPLIT_ROWS: in the chain-bound tail only the first 128 columns of the next block column take this
    // panel's K = W update in the panel chain
    st.next = st.tail_panel ? PotrfStep::NEXT_DONE
              : (side && s.next_split_rows > 0 && Np - J1 <= s.next_split_rows && J2 - J1 > PB && J2 - J1 <= GPAK_PANEL_MID)
                  ? PotrfStep::NEXT_SPLIT
                  : PotrfStep::NEXT_PANEL;
    if (J2 < Np) {
      // chain-bound tail: the bulk update is off the critical path there; on the CU-masked queue it leaves idle
      // compute units to potrf128 and the small panel products
      st.bulk = (caps.tail_queue && la && Np - J2 <= s.tail_rows) ? PotrfStep::Q_TAIL
                : (caps.bulk_queue && la)                          ? PotrfStep::Q_BULK
                                                                   : PotrfStep::Q_MAIN;
      st.ticket = bulk++;
    }
  }
  return plan;
}

// Workgroups of the bulk update of a trailing matrix of mt tile rows: one per lower tile plus, with the ticketed map,
// surplus_pct percent more, rounded up per XCD (the grid gpak_launch_gemm_nt makes for it; pass 0 for the static map,
// whose workgroups beyond the tiles exit at once).
inline long gpak_bulk_workgroups(int mt, int surplus_pct) {
  if (mt <= 0) return 0;
  const long tiles = (long)mt * (mt + 1) / 2;
  return tiles + 8 * ((tiles * (surplus_pct > 0 ? surplus_pct : 0) + 799) / 800);
}

// Which 128 x 128 block kernel the panel takes: true = the co-resident 4-wave build.  A beside_bulk panel needs it
// while the bulk update beside it (panel b-1's, bulk_workgroups_beside workgroups) fills the chip; once that launch has
// no more workgroups than the chip has compute units, whole CUs are free or hold one bulk workgroup, and the 8-wave
// build fits there (2 x 134 + 210 VGPRs per SIMD; the bulk kernel uses no LDS to speak of).  potrf_co 0 / 2 force one build.
inline bool gpak_potrf_block_co(const PotrfStep &st, int potrf_co, long bulk_workgroups_beside, int cu_count) {
  if (potrf_co != 1) return potrf_co == 2;
  return st.beside_bulk && !(cu_count > 0 && bulk_workgroups_beside <= cu_count);
}
