// local_search_dev.hip -- the exact k-nearest-sample search of moving-neighbourhood kriging on the device:
// gpak_dev_local_search (include/gpak_dev_local_search.h), the kernel alone on caller-owned buffers, and
// gpak_local_neighbours_dev (include/gpak_local_search.h), the context-level call around it.
//
// The lists are those of the host search (local_search.cpp) byte for byte: they are ordered by (dist2, index), a total
// order, and dist2 is formed in the one stated arithmetic -- no fused multiply-add (the pragma below; hipcc contracts by
// default) -- from coordinates that the HOST transformed (local_grid.h, shared with the host search).  What a ring walk
// visits first changes nothing of that; only the bound that ends it must hold, and it is the host's (visit_rings).
//
// Shape: one wave per centre, four centres per 256-thread workgroup; a wave never waits for another wave or workgroup and
// there is no barrier (a wave whose centre is past the batch just leaves).  The best list lives sorted in registers, entry q
// in lane q & 63, slot q >> 6; an insertion is one compare per slot and a shift by one lane.  A ring's rows (a0, a1) are
// taken 64 at a time, one row per lane: a shell row is ONE contiguous span of `start`, an interior row its two face cells.
// The wave then walks the rows that hold anything, 64 samples at a time, one candidate per lane; it filters by the radius
// and by the list's worst entry, and takes the survivors from a 64-bit ballot in lane order.  Every loop is bounded by
// r_end, by a ring's row count or by a span's length, all known on entry; nothing spins on memory.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/gpak_dev_local_search.h"
#include "../../include/gpak_local_search.h"
#include "gpak_internal.h"
#include "local_grid.h"

#define LS_MAX 128          // GPAK_LOCAL_MAX of include/gpak_local.h
#define LS_WAVE_CENTRES 4   // centres per workgroup

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool ls_before(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }

// the value of the lane before (lane 0: that of lane 63)
__device__ __forceinline__ double ls_prev(double v, int lane) { return __shfl(v, (lane + 63) & 63); }
__device__ __forceinline__ int ls_prev(int v, int lane) { return __shfl(v, (lane + 63) & 63); }

template <int D>
__global__ __launch_bounds__(256) void gpak_local_search_f64(
    const double *__restrict__ pts, const int *__restrict__ ids, const int *__restrict__ start, int n, double lo0, double lo1,
    double lo2, double h, int n0, int n1, int n2, double scale, const double *__restrict__ tc, int nB, int k, double radius,
    int *__restrict__ nbr, int *__restrict__ used, double *__restrict__ dist2, unsigned long long *__restrict__ visited) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * LS_WAVE_CENTRES + (threadIdx.x >> 6);
  if (b >= nB) return;   // the whole wave: no barrier follows
  const double inf = __builtin_huge_val();
  double c[D], cmax = 0.0;
  bool fine = true;
  for (int j = 0; j < D; j++) {
    c[j] = tc[(size_t)b * D + j];
    fine = fine && isfinite(c[j]);
    cmax = fmax(cmax, fabs(c[j]));
  }
  // the list: entry q in lane q & 63, slot q >> 6; (inf, INT_MAX) where nothing is yet, which sorts after every sample
  double d0 = inf, d1 = inf;
  int i0 = INT_MAX, i1 = INT_MAX;
  int cnt = 0;
  double wd = inf;   // entry k - 1: the worst of a full list
  int wi = INT_MAX;
  unsigned long long seen = 0;
  const int klane = (k - 1) & 63;
  const bool two = k > 64;
  const double r2max = radius * radius;

  const double lo[3] = {lo0, lo1, lo2};
  const int nn[3] = {n0, n1, n2};
  int ic[3], r0 = 0, r_end = 0;
  for (int j = 0; j < 3; j++) {
    // a centre outside the grid is taken to the layer of cells just outside it, as on the host
    const double f = floor((c[j] - lo[j]) / h);
    fine = fine && !isnan(f);   // an origin that is not finite: no cell, no list
    ic[j] = !(f >= -1.0) ? -1 : (f > (double)nn[j] ? nn[j] : (int)f);
    r0 = max(r0, max(-ic[j], ic[j] - (nn[j] - 1)));
    r_end = max(r_end, max(ic[j], nn[j] - 1 - ic[j]));
  }
  if (fine) {
    const double slack = 1e-10 * (scale + cmax + h);
    for (int r = r0; r <= r_end; r++) {
      if (r > 0) {   // every sample not yet seen is at least (r - 1) h away
        const double lb = (double)(r - 1) * h - slack;
        if (lb > 0.0 && ((cnt == k && wd < lb * lb) || (radius > 0.0 && lb > radius))) break;
      }
      const int a0lo = max(0, ic[0] - r), a0hi = min(n0 - 1, ic[0] + r);
      const int a1lo = max(0, ic[1] - r), a1hi = min(n1 - 1, ic[1] + r);
      const int a2lo = max(0, ic[2] - r), a2hi = min(n2 - 1, ic[2] + r);
      const int w1 = a1hi - a1lo + 1;
      const long nrow = (long)(a0hi - a0lo + 1) * w1;
      for (long base = 0; base < nrow; base += 64) {
        // one row per lane: its samples are slots [b0, e0) and [b1, e1) of pts
        const long row = base + lane;
        int b0 = 0, e0 = 0, b1 = 0, e1 = 0;
        if (row < nrow) {
          const int a0 = a0lo + (int)(row / w1), a1 = a1lo + (int)(row % w1);
          const size_t cell = ((size_t)a0 * n1 + a1) * n2;
          if (abs(a0 - ic[0]) == r || abs(a1 - ic[1]) == r) {
            if (a2lo <= a2hi) { b0 = start[cell + a2lo]; e0 = start[cell + a2hi + 1]; }
          } else {   // only the two faces ic2 - r and ic2 + r (r > 0 here: ring 0 is one shell row)
            const int f0 = ic[2] - r, f1 = ic[2] + r;
            if (f0 >= 0 && f0 < n2) { b0 = start[cell + f0]; e0 = start[cell + f0 + 1]; }
            if (f1 >= 0 && f1 < n2) { b1 = start[cell + f1]; e1 = start[cell + f1 + 1]; }
          }
          // whatever `start` holds, no slot outside pts is read
          b0 = max(b0, 0); e0 = min(e0, n); b1 = max(b1, 0); e1 = min(e1, n);
        }
        const int len0 = max(e0 - b0, 0), len1 = max(e1 - b1, 0);
        unsigned long long rows = __ballot(len0 + len1 > 0);
        while (rows) {
          const int src = __ffsll((long long)rows) - 1;
          rows &= rows - 1;
          const int sb0 = __shfl(b0, src), sl0 = __shfl(len0, src), sb1 = __shfl(b1, src), len = sl0 + __shfl(len1, src);
          for (int q0 = 0; q0 < len; q0 += 64) {   // the row's two spans as one, 64 samples at a time
            const int q = q0 + lane;
            const bool have = q < len;
            double s = inf;
            int id = INT_MAX;
            if (have) {
              const int p = q < sl0 ? sb0 + q : sb1 + (q - sl0);
              const double *t = pts + (size_t)p * D;
              double e = t[0] - c[0];
              s = e * e;
              for (int j = 1; j < D; j++) {
                e = t[j] - c[j];
                s = s + e * e;
              }
              id = ids[p];
            }
            seen += (unsigned long long)min(len - q0, 64);
            const bool pass = have && !(radius > 0.0 && !(s <= r2max)) && ls_before(s, id, wd, wi);
            unsigned long long take = __ballot(pass);
            while (take) {
              const int from = __ffsll((long long)take) - 1;
              take &= take - 1;
              const double cs = __shfl(s, from);
              const int ci = __shfl(id, from);
              if (!ls_before(cs, ci, wd, wi)) continue;   // the worst entry has moved since the ballot
              // every entry that sorts after the candidate moves up by one; the candidate takes the first of their places
              const double p0d = ls_prev(d0, lane);
              const int p0i = ls_prev(i0, lane);
              if (two) {
                const double x1d = ls_prev(d1, lane);
                const int x1i = ls_prev(i1, lane);
                const double p1d = lane ? x1d : p0d;   // slot 1 of lane 0 follows slot 0 of lane 63
                const int p1i = lane ? x1i : p0i;
                if (!ls_before(d1, i1, cs, ci)) {
                  const bool first = ls_before(p1d, p1i, cs, ci);
                  d1 = first ? cs : p1d;
                  i1 = first ? ci : p1i;
                }
              }
              if (!ls_before(d0, i0, cs, ci)) {
                const bool first = lane == 0 || ls_before(p0d, p0i, cs, ci);
                d0 = first ? cs : p0d;
                i0 = first ? ci : p0i;
              }
              cnt = min(cnt + 1, k);
              wd = __shfl(two ? d1 : d0, klane);
              wi = __shfl(two ? i1 : i0, klane);
            }
          }
        }
      }
    }
  }

  int *out = nbr + (size_t)k * b;
  if (lane < k) out[lane] = lane < cnt ? i0 : -1;
  if (64 + lane < k) out[64 + lane] = 64 + lane < cnt ? i1 : -1;
  if (dist2) {
    double *od = dist2 + (size_t)k * b;
    if (lane < k) od[lane] = lane < cnt ? d0 : 0.0;
    if (64 + lane < k) od[64 + lane] = 64 + lane < cnt ? d1 : 0.0;
  }
  if (lane == 0) {
    if (used) used[b] = cnt;
    if (visited) atomicAdd(visited, seen);
  }
}

struct Timer {   // device ms between two points of a stream
  hipEvent_t a = nullptr, b = nullptr;
  double ms = 0.0;
  bool ok() { return (a || hipEventCreate(&a) == hipSuccess) && (b || hipEventCreate(&b) == hipSuccess); }
  void start(hipStream_t st) { hipEventRecord(a, st); }
  void stop(hipStream_t st) { hipEventRecord(b, st); }
  void collect() { float v = 0; if (hipEventElapsedTime(&v, a, b) == hipSuccess) ms += v; }
  ~Timer() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

}  // namespace

extern "C" {

int gpak_dev_local_search(void *stream, const double *pts, const int *ids, const int *start, int n, int d, double lo0, double lo1,
                          double lo2, double h, int n0, int n1, int n2, double scale, const double *tc, int nB, int k,
                          double radius, int *nbr, int *used, double *dist2, unsigned long long *visited) {
  if (!pts || !ids || !start || !tc || !nbr || n < 1 || nB < 1 || (d != 3 && d != 4) || k < 1 || k > LS_MAX || n0 < 1 || n1 < 1 ||
      n2 < 1 || !(h > 0.0) || !std::isfinite(h) || std::isnan(radius))
    return GPAK_EINVAL;
  const dim3 grid((unsigned)((nB + LS_WAVE_CENTRES - 1) / LS_WAVE_CENTRES)), block(64 * LS_WAVE_CENTRES);
  if (d == 3)
    hipLaunchKernelGGL(gpak_local_search_f64<3>, grid, block, 0, (hipStream_t)stream, pts, ids, start, n, lo0, lo1, lo2, h, n0, n1,
                       n2, scale, tc, nB, k, radius, nbr, used, dist2, visited);
  else
    hipLaunchKernelGGL(gpak_local_search_f64<4>, grid, block, 0, (hipStream_t)stream, pts, ids, start, n, lo0, lo1, lo2, h, n0, n1,
                       n2, scale, tc, nB, k, radius, nbr, used, dist2, visited);
  return hipGetLastError() == hipSuccess ? GPAK_OK : GPAK_EHIP;
}

int gpak_local_neighbours_dev(gpak_ctx *ctx, const double *Xs, long Ns, int d, const double *Xc, long M, const double *G, int k,
                              double radius, int *nbr, int *used, double *dist2, gpak_local_search_summary *summary) {
  if (!ctx) return GPAK_EINVAL;
  auto refuse = [&](int rc, const std::string &what) { ctx->err = "gpak_local_neighbours_dev: " + what; return rc; };
  if (!Xs || !Xc || !nbr) return refuse(GPAK_EINVAL, std::string(!Xs ? "Xs" : !Xc ? "Xc" : "nbr") + " is NULL");
  if (d != 3 && d != 4) return refuse(GPAK_EINVAL, "d = " + std::to_string(d) + ": the samples have 3 or 4 columns");
  if (k < 1 || k > LS_MAX) return refuse(GPAK_EINVAL, "k = " + std::to_string(k) + " is outside 1..128");
  if (Ns < 1 || M < 1 || Ns > (long)INT_MAX - 128)
    return refuse(GPAK_EINVAL, "Ns = " + std::to_string(Ns) + ", M = " + std::to_string(M) + " must be positive (Ns at most INT_MAX - 128)");
  if (std::isnan(radius)) return refuse(GPAK_EINVAL, "the radius is NaN");
  if (ctx->multi) return refuse(GPAK_ENOTIMPL, "built for the single-GPU context (gpak_create) only");
  for (size_t i = 0; i < (size_t)Ns * d; i++)
    if (!std::isfinite(Xs[i])) return refuse(GPAK_EINVAL, "a sample coordinate is not finite");
  for (size_t i = 0; i < (size_t)M * d; i++)
    if (!std::isfinite(Xc[i])) return refuse(GPAK_EINVAL, "a centre coordinate is not finite");
  for (int i = 0; G && i < d * d; i++)
    if (!std::isfinite(G[i])) return refuse(GPAK_EINVAL, "an entry of G is not finite");

  // the grid and both transforms on the host, by the host search's own code: the same cells, the same bytes
  const auto t0 = std::chrono::steady_clock::now();
  gpak_local_grid::Grid g;
  if (!gpak_local_grid::build_grid(Xs, Ns, d, G, g)) return refuse(GPAK_EINVAL, "a transformed sample coordinate is not finite");
  const size_t nc = g.start.size() - 1;
  std::vector<int> start(g.start.begin(), g.start.end());   // Ns fits an int
  const double grid_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::vector<double> tc((size_t)M * d);
  for (long b = 0; b < M; b++) {
    gpak_local_grid::transform_point(Xc, M, b, d, G, &tc[(size_t)b * d]);
    for (int j = 0; j < d; j++)
      if (!std::isfinite(tc[(size_t)b * d + j])) return refuse(GPAK_EINVAL, "a transformed centre coordinate is not finite");
  }

  GPAK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int cap = (int)std::min<long>(ctx->sched.pred_batch > 0 ? ctx->sched.pred_batch : 16384, M);
  // buffers of the call's own: nothing of the context's is touched
  DevBuf<double> dPts, dTc, dDist;
  DevBuf<int> dIds, dStart, dNbr, dUsed;
  DevBuf<unsigned long long> dVisited;
  const bool ok = dPts.reserve((size_t)Ns * d) && dIds.reserve((size_t)Ns) && dStart.reserve(nc + 1) && dTc.reserve((size_t)cap * d) &&
                  dNbr.reserve((size_t)k * cap) && dUsed.reserve((size_t)cap) && (!dist2 || dDist.reserve((size_t)k * cap)) &&
                  dVisited.reserve(1);
  if (!ok) {
    (void)hipGetLastError();
    return refuse(GPAK_ENOMEM, "device allocation failed for the grid (d doubles and an int per sample, an int per cell) or a centre batch");
  }
  Timer t_up, t_search;
  if (!t_up.ok() || !t_search.ok()) { ctx->err = "hipEventCreate failed"; return GPAK_EHIP; }
  t_up.start(st);
  GPAK_HIP(hipMemcpyAsync(dPts, g.pts.data(), sizeof(double) * (size_t)Ns * d, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dIds, g.ids.data(), sizeof(int) * (size_t)Ns, hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemcpyAsync(dStart, start.data(), sizeof(int) * (nc + 1), hipMemcpyHostToDevice, st));
  GPAK_HIP(hipMemsetAsync(dVisited, 0, sizeof(unsigned long long), st));
  t_up.stop(st);

  std::vector<int> counts((size_t)cap);
  int batches = 0, max_used = 0;
  t_search.start(st);
  for (long b0 = 0; b0 < M; b0 += cap, batches++) {
    const int mb = (int)std::min<long>(cap, M - b0);
    GPAK_HIP(hipMemcpyAsync(dTc, &tc[(size_t)b0 * d], sizeof(double) * (size_t)mb * d, hipMemcpyHostToDevice, st));
    const int rc = gpak_dev_local_search(st, dPts, dIds, dStart, (int)Ns, d, g.lo[0], g.lo[1], g.lo[2], g.h, g.n[0], g.n[1], g.n[2],
                                         g.scale, dTc, mb, k, radius, dNbr, dUsed, dist2 ? (double *)dDist : nullptr, dVisited);
    if (rc != GPAK_OK) { ctx->err = "gpak_local_neighbours_dev: the search kernel did not launch"; return rc; }
    GPAK_HIP(hipMemcpyAsync(nbr + (size_t)k * b0, dNbr, sizeof(int) * (size_t)k * mb, hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipMemcpyAsync(counts.data(), dUsed, sizeof(int) * (size_t)mb, hipMemcpyDeviceToHost, st));
    if (dist2) GPAK_HIP(hipMemcpyAsync(dist2 + (size_t)k * b0, dDist, sizeof(double) * (size_t)k * mb, hipMemcpyDeviceToHost, st));
    GPAK_HIP(hipStreamSynchronize(st));
    GPAK_HIP(hipGetLastError());
    for (int b = 0; b < mb; b++) max_used = std::max(max_used, counts[b]);
    if (used) std::copy(counts.begin(), counts.begin() + mb, used + b0);
  }
  t_search.stop(st);
  unsigned long long visited = 0;
  GPAK_HIP(hipMemcpyAsync(&visited, dVisited, sizeof(visited), hipMemcpyDeviceToHost, st));
  GPAK_HIP(hipStreamSynchronize(st));
  t_up.collect(); t_search.collect();
  if (summary) {
    summary->grid_ms = grid_ms;
    summary->upload_ms = t_up.ms;
    summary->search_ms = t_search.ms;
    summary->centres = M;
    summary->cells = (long)nc;
    summary->visited = visited;
    summary->batches = batches;
    summary->max_used = max_used;
  }
  return GPAK_OK;
}

}  // extern "C"
