// grid.hip -- the ROW-BLOCK x COLUMN-BLOCK layout of north_star: one rank of a Pr x Pc process grid
// (include/gpak_dist.h, gpak_grid_*), distributing GP_utils::ldB2_exact / solve_chol / logLikelihood
// (GP_Utils.cpp:841-845, 872-915, 1138-1162).  What a rank is apart from its layout -- engine, transport, replicated
// vectors, the start and the end of a step -- is the RankCore of dist_core.h, shared with the 1-D schedule of dist.hip.
//
// Ownership: block (i, j), i >= j, of B = I + K/sn2 (nb x nb blocks) lives on rank (i % Pr) + Pr * (j % Pc).  A rank
// stores its blocks as one local matrix: local block row li = i / Pr, local block column lj = j / Pc.
//
// Step b (block column b, width W; "prb, pcb" = b % Pr, b % Pc):
//   D   owner (prb, pcb)        factor the diagonal block (factor_panel restricted to its W rows) -> L_bb, inverses
//   Bc  column group pcb        broadcast [L_bb | inverses] down the process column (root prb)
//   S   ranks (., pcb)          P_local := A_local,b L_bb^-T for the local row blocks i > b          (solve_rows)
//   Br  every row group         broadcast the solved rows along the process row (root pcb) -> `rowpanel`
//   Bt  every column group      for every root pr': the pieces P_j, j > b, j % Pr == pr', j % Pc == pc, packed into
//                               one buffer and broadcast down the column -> `colpiece[pr']` (the transposed operand)
//   U   every rank              block (i, j) -= P_i P_j^T for its local blocks i >= j > b            (update_rect)
// One block column of look-ahead: the local part of block column b+1 is updated first, on the panel stream, and step
// b+1's D / Bc / S / Br / Bt run there while the bulk stream updates the rest with step b's panels (two sets of panel
// buffers).  Collectives are issued on the panel stream, in the same order on every member of a group.
//
// Triangular solves: distributed.  Forward, block by block: the partial sums acc_b of the ranks of process row prb are
// all-reduced over that row group, the owner of (b, b) solves its W unknowns and broadcasts them to the WORLD (so z and
// alpha end up replicated, as the 1-D schedule has them), the ranks of process column pcb add L_ib z_b to their partial
// sums.  Backward: the same with column groups and transposed products.
#include "dist_core.h"

struct gpak_grid : RankCore {
  int Pr = 1, Pc = 1, pr = 0, pc = 0;
  int nLr = 0, nLc = 0;      // local block rows / columns
  int rows_loc = 0, cols_loc = 0;
  long ld = 0;
  double *local = nullptr, *z = nullptr, *acc = nullptr, *xloc = nullptr, *tmp = nullptr;
  double *rowpanel[2] = {nullptr, nullptr};
  double *diagbuf[2] = {nullptr, nullptr};
  std::vector<double *> colpiece[2];     // per root pr': packed P_j pieces of this rank's block columns
  std::vector<double *> diag_inv;        // per owned diagonal block: its inverted 128-blocks (kept for the solves)

  int owner(int i, int j) const { return (i % Pr) + Pr * (j % Pc); }
  // first local block row / column whose global index is >= g
  int li0(int g) const { return (g + Pr - 1 - pr) / Pr; }
  int lj0(int g) const { return (g + Pc - 1 - pc) / Pc; }
  int rows_from(int li) const { return li >= nLr ? 0 : rows_loc - li * nb; }   // local rows from local block row li on
  double *blk(int li, int lj) const { return local + (size_t)li * nb + (size_t)lj * nb * ld; }
};

static void grid_release(gpak_grid *h) {
  gpak_dist_engine &E = h->E;
  auto rel = [&](double *&p) { if (p) E.release(E.self, p); p = nullptr; };
  rel(h->local); rel(h->z); rel(h->acc); rel(h->xloc); rel(h->tmp);
  for (int k = 0; k < 2; k++) {
    rel(h->rowpanel[k]); rel(h->diagbuf[k]);
    for (double *&p : h->colpiece[k]) rel(p);
    h->colpiece[k].clear();
  }
  for (double *&p : h->diag_inv) rel(p);
  h->diag_inv.clear();
  core_release(h);
}

extern "C" {

int gpak_grid_create(gpak_grid **out, int rank, int world, int Pr, int Pc, int device, const gpak_dist_engine *engine,
                     const gpak_dist_transport *transport) {
  if (!out || world < 1 || rank < 0 || rank >= world || Pr < 1 || Pc < 1 || Pr * Pc != world) return GPAK_EINVAL;
  *out = nullptr;
  if (Pr == 1) return GPAK_EINVAL;   // 1 x P is the block-column-cyclic layout: gpak_dist_create
  gpak_grid *h = new gpak_grid();
  h->Pr = Pr; h->Pc = Pc; h->pr = rank % Pr; h->pc = rank / Pr;
  int rc = core_attach(h, rank, world, device, engine, transport, true);
  if (!rc && (!h->E.fill_rect || !h->E.solve_rows || !h->E.update_rect || !h->E.gemv_n_add || !h->E.gemv_t || !h->E.vec_axpy))
    rc = GPAK_EINVAL;   // the engine lacks the pieces of the 2-D layout
  if (!rc && (!h->T.grid_setup || !h->T.bcast_group || !h->T.allreduce_sum_group))
    rc = GPAK_EINVAL;   // the transport has no sub-groups
  if (!rc) rc = h->T.grid_setup(h->T.self, Pr, Pc);
  if (rc) { delete h; return rc; }
  *out = h;
  return GPAK_OK;
}

void gpak_grid_destroy(gpak_grid *h) {
  if (!h) return;
  core_set_device(h);
  gpak_dist_engine &E = h->E;
  if (h->s_bulk) { E.stream_sync(E.self, h->s_bulk); E.stream_sync(E.self, h->s_panel); }
  grid_release(h);
  if (h->s_panel) E.stream_destroy(E.self, h->s_panel);
  if (h->s_bulk) E.stream_destroy(E.self, h->s_bulk);
  core_detach(h);
  delete h;
}

const char *gpak_grid_last_error(const gpak_grid *h) { return h ? h->err.c_str() : "null handle"; }

int gpak_grid_init_rccl(gpak_grid *h, const char *id) { return h ? core_init_rccl(h, id, h->Pr) : GPAK_EINVAL; }

int gpak_grid_set_train(gpak_grid *h, const double *X, const double *y, int N, int d, int nb) {
  int rc = core_train_check(h, X, y, N, d, &nb);
  if (rc) return rc;
  gpak_dist_engine &E = h->E;
  if (!h->s_bulk) {
    h->s_bulk = E.stream_create(E.self, 0);
    h->s_panel = E.stream_create(E.self, 1);
    if ((!h->s_bulk || !h->s_panel) && h->builtin_engine) { h->err = "stream creation failed"; return GPAK_EHIP; }
  }
  E.stream_sync(E.self, h->s_bulk); E.stream_sync(E.self, h->s_panel);
  grid_release(h);
  bool ok = core_train_alloc(h, N, nb);
  h->nLr = h->li0(h->nJ); h->nLc = h->lj0(h->nJ);
  // local rows / columns: every local block is nb wide except the globally last one
  auto extent = [&](int nL, int Pq, int q) {
    int e = 0;
    for (int l = 0; l < nL; l++) e += h->width(l * Pq + q);
    return e;
  };
  h->rows_loc = extent(h->nLr, h->Pr, h->pr);
  h->cols_loc = extent(h->nLc, h->Pc, h->pc);
  h->ld = std::max(h->rows_loc, GPAK_TILE) + (h->rows_loc >= 1024 ? 32 : 0);
  const size_t Np = h->Np;
  auto dalloc = [&](size_t n) { return (double *)E.alloc(E.self, sizeof(double) * (n ? n : 1)); };
  h->local = dalloc((size_t)h->ld * std::max(h->cols_loc, GPAK_TILE));
  h->z = dalloc(Np); h->acc = dalloc(std::max<size_t>(h->rows_loc, h->cols_loc) + nb);
  h->xloc = dalloc((size_t)h->rows_loc + nb); h->tmp = dalloc(Np);
  ok = ok && h->local && h->z && h->acc && h->xloc && h->tmp;
  const size_t inv_n = (size_t)nb / GPAK_TILE * 2 * GPAK_TILE * GPAK_TILE;
  for (int k = 0; k < 2 && ok; k++) {
    h->rowpanel[k] = dalloc((size_t)std::max(h->rows_loc, GPAK_TILE) * nb);
    h->diagbuf[k] = dalloc((size_t)nb * nb + inv_n);
    h->colpiece[k].assign(h->Pr, nullptr);
    // root pr' holds the pieces of my block columns j with j % Pr == pr': at most ceil(nLc / 1) blocks; sized exactly
    for (int q = 0; q < h->Pr && ok; q++) {
      size_t blocks = 0;
      for (int lj = 0; lj < h->nLc; lj++) if ((lj * h->Pc + h->pc) % h->Pr == q) blocks++;
      h->colpiece[k][q] = dalloc(std::max<size_t>(1, blocks) * nb * nb);
      ok = h->colpiece[k][q] != nullptr;
    }
    ok = ok && h->rowpanel[k] && h->diagbuf[k];
  }
  h->diag_inv.assign(h->nJ, nullptr);
  for (int b = 0; b < h->nJ && ok; b++)
    if (h->owner(b, b) == h->rank) { h->diag_inv[b] = dalloc(inv_n); ok = h->diag_inv[b] != nullptr; }
  if (!ok) { h->err = "device allocation failed for the distributed training set"; grid_release(h); return GPAK_ENOMEM; }
  rc = core_train_upload(h, X, y);
  if (rc) return rc;
  for (int b = 0; b < h->nJ; b++)
    if (h->diag_inv[b]) RCHK(E.zero(E.self, h->s_bulk, h->diag_inv[b], sizeof(double) * inv_n));
  for (int k = 0; k < 2; k++) RCHK(E.zero(E.self, h->s_bulk, h->diagbuf[k], sizeof(double) * ((size_t)nb * nb + inv_n)));
  RCHK(E.stream_sync(E.self, h->s_bulk));
  return GPAK_OK;
}

int gpak_grid_set_params(gpak_grid *h, const double *expans, double bias, double sn2, int dist_mode) {
  return core_set_params(h, expans, bias, sn2, dist_mode);
}

}  // extern "C"

// D / Bc / S / Br / Bt of step b on the panel stream, into buffer set b & 1
static int grid_produce(gpak_grid *h, int b) {
  gpak_dist_engine &E = h->E;
  gpak_dist_transport &T = h->T;
  const int J = h->start(b), W = h->width(b), nb = h->nb, k = b & 1;
  const int prb = b % h->Pr, pcb = b % h->Pc;
  const long ld = h->ld;
  void *sp = h->s_panel;
  const size_t inv_n = (size_t)W / GPAK_TILE * 2 * GPAK_TILE * GPAK_TILE;
  double *Lbb = h->diagbuf[k], *inv = h->diagbuf[k] + (size_t)nb * nb;
  size_t t0 = h->time_event(sp);
  if (h->pc == pcb) {
    if (h->pr == prb) {
      // D: the diagonal block alone (rows J .. J+W): a virtual base makes global row J the block's first local row
      double *dblk = h->blk(b / h->Pr, b / h->Pc);
      RCHK(E.factor_panel(sp, dblk - J, ld, J + W, J, W, inv, h->info));
      RCHK(E.pack(sp, dblk, ld, 0, W, W, Lbb));
      RCHK(E.copy(E.self, sp, h->diag_inv[b], inv, sizeof(double) * inv_n));
    }
    // Bc: [L_bb | inverses] down the process column (one buffer: nb*nb doubles for L_bb whatever W is)
    RCHK(T.bcast_group(T.self, sp, h->diagbuf[k], (size_t)nb * nb + inv_n, prb, GPAK_GROUP_COL));
    if (h->pr != prb) h->stats.bytes_broadcast += 8.0 * ((double)nb * nb + inv_n);
    // S: my rows of panel b
    const int li = h->li0(b + 1), nrows = h->rows_from(li);
    if (nrows > 0) {
      double *P = h->blk(li, b / h->Pc);
      RCHK(E.solve_rows(sp, P, ld, nrows, W, Lbb, W, inv));
      RCHK(E.pack(sp, h->blk(0, b / h->Pc), ld, li * nb, nrows, W, h->rowpanel[k]));
    }
  }
  // Br: the solved rows along the process row (every rank of the row has the same local rows)
  {
    const int li = h->li0(b + 1), nrows = h->rows_from(li);
    if (nrows > 0) {
      RCHK(T.bcast_group(T.self, sp, h->rowpanel[k], (size_t)nrows * W, pcb, GPAK_GROUP_ROW));
      if (h->pc != pcb) h->stats.bytes_broadcast += 8.0 * nrows * W;
    }
  }
  // Bt: the pieces P_j of my block columns j > b, from the rank of my process column that holds row block j
  for (int q = 0; q < h->Pr; q++) {
    // the list is the same on every rank of the column group: j > b, j % Pc == pc, j % Pr == q, ascending
    size_t off = 0;
    int count = 0;
    for (int lj = h->lj0(b + 1); lj < h->nLc; lj++) {
      const int j = lj * h->Pc + h->pc;
      if (j % h->Pr != q) continue;
      if (h->pr == q) {   // I hold P_j in my row panel: local block row j / Pr, rows relative to the panel's first row
        const int li = h->li0(b + 1), nrows = h->rows_from(li);
        RCHK(E.pack(sp, h->rowpanel[k], nrows, (j / h->Pr - li) * nb, h->width(j), W, h->colpiece[k][q] + off));
      }
      off += (size_t)h->width(j) * W;
      count++;
    }
    if (count == 0) continue;
    RCHK(T.bcast_group(T.self, sp, h->colpiece[k][q], off, q, GPAK_GROUP_COL));
    if (h->pr != q) h->stats.bytes_broadcast += 8.0 * off;
  }
  h->spans.push_back({t0, h->time_event(sp), 1});
  return GPAK_OK;
}

// U: block columns [lj_from, lj_to) of my local storage get step b's update on `stream`
static int grid_update(gpak_grid *h, int b, void *stream, int lj_from, int lj_to, bool count_flops) {
  gpak_dist_engine &E = h->E;
  const int W = h->width(b), nb = h->nb, k = b & 1;
  const int li_p = h->li0(b + 1), nrows_p = h->rows_from(li_p);   // the row panel covers local block rows li_p ..
  if (nrows_p <= 0) return GPAK_OK;
  std::vector<size_t> off(h->Pr, 0);
  // offsets of the pieces inside colpiece[q]: walk my block columns > b in order, as grid_produce packed them
  for (int lj = h->lj0(b + 1); lj < h->nLc; lj++) {
    const int j = lj * h->Pc + h->pc, q = j % h->Pr, Wj = h->width(j);
    const double *Pj = h->colpiece[k][q] + off[q];
    off[q] += (size_t)Wj * W;
    if (lj < lj_from || lj >= lj_to) continue;
    const int li = h->li0(j), mrows = h->rows_from(li);
    if (mrows <= 0) continue;
    const bool diag_first = (j % h->Pr) == h->pr;   // my first local block row >= j IS block row j
    RCHK(E.update_rect(stream, h->rowpanel[k] + (size_t)(li - li_p) * nb, nrows_p, Pj, Wj, W, h->blk(li, lj), h->ld, mrows, Wj,
                       diag_first ? 1 : 0));
    if (count_flops) {
      const double mt = mrows / GPAK_TILE, wt = Wj / GPAK_TILE;
      const double tiles = diag_first ? wt * mt - wt * (wt - 1) / 2.0 : wt * mt;
      h->stats.bulk_flops += tiles * 2.0 * GPAK_TILE * GPAK_TILE * W;
      h->stats.bulk_bytes += tiles * 2.0 * GPAK_TILE * GPAK_TILE * 8.0;
      h->stats.bulk_launches += 1;
    }
  }
  return GPAK_OK;
}

static int grid_factor(gpak_grid *h, int *failed_col) {
  gpak_dist_engine &E = h->E;
  gpak_dist_transport &T = h->T;
  const int nJ = h->nJ;
  const int init = 0x7fffffff;
  RCHK(E.upload(E.self, h->s_bulk, h->info, &init, sizeof(int)));
  void *e_fill = h->sync_event();
  RCHK(E.event_record(E.self, e_fill, h->s_bulk));
  RCHK(E.stream_wait_event(E.self, h->s_panel, e_fill));
  void *e_bulk[2] = {nullptr, nullptr};   // bulk update of step b (b & 1): it reads buffer set b & 1
  int rc = grid_produce(h, 0);
  if (rc) return rc;
  for (int b = 0; b < nJ; b++) {
    const int nxt = b + 1;
    if (nxt >= nJ) break;
    // panel stream: my part of block column b+1 first (it was last touched by bulk update b-1), then step b+1's panel
    if (e_bulk[(b + 1) & 1]) RCHK(E.stream_wait_event(E.self, h->s_panel, e_bulk[(b + 1) & 1]));
    const bool mine = (nxt % h->Pc) == h->pc;
    const int ljn = nxt / h->Pc;
    if (mine) {
      rc = grid_update(h, b, h->s_panel, ljn, ljn + 1, false);
      if (rc) return rc;
    }
    // the bulk stream needs step b's panels: everything queued on the panel stream so far
    void *e_panel = h->sync_event();
    RCHK(E.event_record(E.self, e_panel, h->s_panel));
    RCHK(E.stream_wait_event(E.self, h->s_bulk, e_panel));
    // step b+1 overwrites buffer set (b+1) & 1, which bulk update b-1 read: waited for above
    rc = grid_produce(h, nxt);
    if (rc) return rc;
    // bulk stream: the rest of my block columns with step b's panels
    const int lj_rest = mine ? ljn + 1 : h->lj0(nxt);
    size_t t0 = h->time_event(h->s_bulk);
    rc = grid_update(h, b, h->s_bulk, lj_rest, h->nLc, true);
    if (rc) return rc;
    h->spans.push_back({t0, h->time_event(h->s_bulk), 0});
    e_bulk[b & 1] = h->sync_event();
    RCHK(E.event_record(E.self, e_bulk[b & 1], h->s_bulk));
  }
  void *e_end = h->sync_event();
  RCHK(E.event_record(E.self, e_end, h->s_panel));
  RCHK(E.stream_wait_event(E.self, h->s_bulk, e_end));
  RCHK(T.allreduce_min_int(T.self, h->s_bulk, h->info, 1));
  int info = init;
  RCHK(E.download(E.self, h->s_bulk, &info, h->info, sizeof(int)));
  *failed_col = info == init ? 0 : info;
  return GPAK_OK;
}

// forward (trans = false: z = L^-1 rhs) and backward (trans = true: out = L^-T in) substitution on the distributed
// factor; `out` ends up replicated on every rank
static int grid_solve(gpak_grid *h, bool trans, const double *in, double *out) {
  gpak_dist_engine &E = h->E;
  gpak_dist_transport &T = h->T;
  void *st = h->s_bulk;
  const int nJ = h->nJ, nb = h->nb;
  RCHK(E.zero(E.self, st, h->acc, sizeof(double) * (std::max(h->rows_loc, h->cols_loc) + nb)));
  RCHK(E.zero(E.self, st, out, sizeof(double) * h->Np));
  if (trans) RCHK(E.zero(E.self, st, h->xloc, sizeof(double) * (h->rows_loc + nb)));
  for (int s = 0; s < nJ; s++) {
    const int b = trans ? nJ - 1 - s : s;
    const int J = h->start(b), W = h->width(b);
    const int prb = b % h->Pr, pcb = b % h->Pc;
    const bool in_group = trans ? (h->pc == pcb) : (h->pr == prb);
    // partial sums of block b: forward -- indexed by my local block row of b; backward -- by my local block column of b
    double *accb = h->acc + (size_t)(trans ? b / h->Pc : b / h->Pr) * nb;
    if (trans && h->pc == pcb) {
      // acc_b = sum over my local rows i > b of L_ib^T x_i
      const int li = h->li0(b + 1), nrows = h->rows_from(li);
      RCHK(E.gemv_t(st, h->blk(li, b / h->Pc), h->ld, nrows, W, h->xloc + (size_t)li * nb, accb));
    }
    if (in_group) RCHK(T.allreduce_sum_group(T.self, st, accb, (size_t)W, trans ? GPAK_GROUP_COL : GPAK_GROUP_ROW));
    if (h->rank == h->owner(b, b)) {
      // t = in_b - acc_b, then the W x W triangular solve with the diagonal block (restricted calls of the 1-D ops)
      RCHK(E.copy(E.self, st, h->tmp + J, in + J, sizeof(double) * W));
      RCHK(E.vec_axpy(st, W, -1.0, accb, h->tmp + J));
      double *dblk = h->blk(b / h->Pr, b / h->Pc);
      if (!trans) RCHK(E.trsv_fwd_block(st, dblk - J, h->ld, J + W, J, W, h->diag_inv[b], h->tmp, out));
      else RCHK(E.trsv_bwd_packed(st, dblk, h->ld, J, J + W, J, W, h->diag_inv[b], h->tmp, h->bwd_scratch, out, nullptr));
    }
    RCHK(T.bcast(T.self, st, out + J, (size_t)W, h->owner(b, b)));
    if (!trans) {
      if (h->pc == pcb) {   // acc_i += L_ib z_b for my local rows i > b
        const int li = h->li0(b + 1), nrows = h->rows_from(li);
        if (nrows > 0) RCHK(E.gemv_n_add(st, h->blk(li, b / h->Pc), h->ld, nrows, W, out + J, h->acc + (size_t)li * nb));
      }
    } else if (h->pr == prb) {
      RCHK(E.copy(E.self, st, h->xloc + (size_t)(b / h->Pr) * nb, out + J, sizeof(double) * W));   // x in local row order
    }
  }
  return GPAK_OK;
}

extern "C" {

int gpak_grid_nlz(gpak_grid *h, double *nlz) {
  if (!h || !nlz) return GPAK_EINVAL;
  *nlz = std::numeric_limits<double>::quiet_NaN();
  if (!h->N) { h->err = "no training set (gpak_grid_set_train)"; return GPAK_ESTATE; }
  if (!h->have_params) { h->err = "no parameters (gpak_grid_set_params)"; return GPAK_ESTATE; }
  if (h->have_result) { *nlz = h->nlz; return GPAK_OK; }
  core_set_device(h);
  gpak_dist_engine &E = h->E;
  // ---- fill: my blocks, block by block (no communication)
  int rc = core_step_begin(h, [&]() -> int {
    for (int lj = 0; lj < h->nLc; lj++) {
      const int j = lj * h->Pc + h->pc;
      for (int li = h->li0(j); li < h->nLr; li++) {
        const int i = li * h->Pr + h->pr;
        RCHK(E.fill_rect(h->s_bulk, h->u, h->cap, h->N, h->start(i), h->width(i), h->start(j), h->width(j), h->expans,
                         h->bias, h->sn2, h->kmode(), h->blk(li, lj), h->ld));
      }
    }
    return GPAK_OK;
  });
  if (rc) return rc;
  h->tp[1] = h->time_event(h->s_bulk);
  int bad = 0;
  rc = grid_factor(h, &bad);
  if (!rc) rc = core_step_factored(h, bad);
  if (rc) return rc;
  // ---- solve_chol (GP_Utils.cpp:841-845) on the distributed factor
  rc = grid_solve(h, false, h->rhs, h->z);
  if (rc) return rc;
  rc = grid_solve(h, true, h->z, h->alpha);
  if (rc) return rc;
  h->tp[3] = h->time_event(h->s_bulk);
  // ---- f = K alpha, the log-determinant from my diagonal blocks, nlZ; the collectives ride on the bulk stream
  std::vector<DiagBlock> diag;
  for (int b = 0; b < h->nJ; b++)
    if (h->owner(b, b) == h->rank) diag.push_back({h->blk(b / h->Pr, b / h->Pc) - h->start(b), h->ld, h->start(b), h->width(b)});
  return core_step_finish(h, h->s_bulk, diag, nlz);
}

int gpak_grid_nlz_terms(gpak_grid *h, double *quad, double *sumlp, double *logdet) {
  double v;
  int rc = gpak_grid_nlz(h, &v);
  return rc ? rc : core_nlz_terms(h, quad, sumlp, logdet);
}

int gpak_grid_get_alpha(gpak_grid *h, double *alpha_host) {
  double v;
  int rc = alpha_host ? gpak_grid_nlz(h, &v) : (int)GPAK_EINVAL;
  return rc ? rc : core_get_alpha(h, alpha_host);
}

int gpak_grid_get_stats(gpak_grid *h, gpak_dist_stats *out) { return core_get_stats(h, out); }
int gpak_grid_failed_column(const gpak_grid *h) { return h ? h->failed_col : 0; }

}  // extern "C"
