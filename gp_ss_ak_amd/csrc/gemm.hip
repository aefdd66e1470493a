// gemm.hip -- fp64 MFMA tile kernel  C = beta*C + alpha * A * B^T  for gfx950.
//
// This is the arithmetic of LAPACK dpotrf's level-3 part, which the reference reaches
// through arma::chol (GP_Utils.cpp:881, 903): the trailing-submatrix update
// (syrk/gemm, alpha=-1, beta=1), the panel triangular solve as a product with the
// pre-inverted 128x128 diagonal block (alpha=1, beta=0), and the forward substitution
// with many right-hand sides of _postVar (GP_Utils.cpp:991).
//
// Three kernels, all 128x128 output tiles of 4x4 v_mfma_f64_16x16x4_f64 accumulators per wave:
//   gpak_gemm_nt_f64_rs    (default)  operands streamed through registers, no LDS, no barriers
//   gpak_gemm_nt_f64_rs32<MI, WROWS>  the same with 32x32 or 16x32 per wave for small tile grids (panel chain)
//   gpak_gemm_nt_f64       (GPAK_GEMM=lds, kept for comparison) K staged 16 deep through double-buffered
//                          LDS with LDS-DMA ([k][row] images, row stride 144 doubles so that the four
//                          k-planes a wave reads per fragment land on disjoint bank halves)
// All operands are column-major, so one k-column of a tile is 1 KiB contiguous (16 B per lane).
//
// MFMA operand roles are swapped (the B-matrix fragment is the instruction's A operand):
// the f64 16x16x4 result layout is col=lane&15,row=(lane>>4)+4*reg, so with the swap a
// lane group holds consecutive matrix rows of one column.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gpak_internal.h"

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

#define TM 128
#define TN 128
#define KB 16
#define LDS_LD 144

// ---------------------------------------------------------------------------------------
// Register-streaming kernel (the default): no LDS, no barriers.  Every lane fetches the elements of
// its own MFMA fragments straight from global memory with 16-B loads, RS_D k-steps ahead in a
// register ring; the four waves of a workgroup (2x2 over the 128x128 tile) never wait for one
// another, and operand sharing between the waves of a CU is left to the vector L1 / the XCD's L2
// (the super-tile map keeps the 64 workgroups of an XCD on the same 8+8 operand panels).
// Against the LDS-staged kernel above: 71.4 vs 66.3 TFLOP/s at N=32768, K=512 (74.1 vs 68.6 for
// K -> inf; back-to-back MFMA issue alone reaches 77.7): what the LDS version loses is not memory
// latency (an L2-resident operand set runs no faster) but the barrier per stage and the LDS-DMA /
// ds_read issue slots next to the MFMAs.
// ---------------------------------------------------------------------------------------
// Super-tile walk shared by the static map and the ticketed one: tile slot `slot` (0..63) of super-tile `ssel`, in the
// order of the super-tiles of the lower triangle (lower_skip == 1) or of the whole grid; false for a slot with no tile.
__device__ __forceinline__ bool gpak_super_tile(int ssel, int slot, int lr, int lower_skip, int mt, int nt, int rb0,
                                                int cb0, int &ti, int &tj) {
  // super-tile = 2^lr rows x 2^(6 - lr) columns of tiles (64 workgroups: what one XCD keeps resident);
  // 3 = 8 x 8, the default (4 x 16 and 16 x 4 measured in round 3: profiles/r03_supertile_shapes.txt)
  const int lc = 6 - lr;
  const int SR = (mt + (1 << lr) - 1) >> lr, SC = (nt + (1 << lc) - 1) >> lc;
  int si, sj = 0;
  if (lower_skip == 1) {   // 1: super-tiles that touch the lower triangle only; 2: all super-tiles, per-tile rule below
    int rem = ssel;
    int first = 0;
    for (; sj < SC; sj++) {   // first super row of column sj whose last tile row reaches the diagonal: (sj << lc) >> lr
      first = (sj << lc) >> lr;
      const int cnt = SR - first;
      if (cnt <= 0) { sj = SC; break; }
      if (rem < cnt) break;
      rem -= cnt;
    }
    si = first + rem;
  } else {
    sj = ssel / SR;
    si = ssel - sj * SR;
  }
  if (sj >= SC) return false;
  ti = (si << lr) + (slot & ((1 << lr) - 1));
  tj = (sj << lc) + (slot >> lr);
  if (ti >= mt || tj >= nt) return false;
  if (lower_skip && (rb0 + ti) < (cb0 + tj)) return false;
  return true;
}

// TRAILING only names the instantiation (the bulk trailing update gets its own line in rocprofv3 statistics).
// K0MAP (the distributed gradient's B^-1 = G G^T on row-cyclic slabs of G): the k-loop of tile row ti starts at global
// row block ti * cyc_tpb + cyc_lt0 (the cyc_* parameters are reused; no cyclic column map in that instantiation).
// TICKET (the bulk update of the factorisation, GpakSchedule::bulk_tickets): which workgroup computes which tile is
// decided at run time instead of by blockIdx.  The static map takes workgroup b to XCD b & 7 and gives it slot
// (b >> 3) & 63 of that XCD's super-tiles, so every XCD has to finish exactly its eighth of the launch however many of its
// slots a CU mask or a co-resident panel kernel has taken.  With tickets, XCD x (read from HW_REG_XCC_ID) owns the same
// list -- super-tiles x, x + 8, ..., 64 slots each, in the static order -- and its workgroups claim entries from the
// front of it; once it is used up they claim entries from the back of the other XCDs' lists, so an XCD with more free
// slots computes more tiles.  Front and back counts of a list share one 64-bit word (tk[x]: front in the low half, back
// in the high half), so one returning atomic add decides every claim: entry front / share - 1 - back is taken iff
// front + back < share before the add.  The launcher starts a few more workgroups than there are tiles; one that finds
// every list used up exits.  Every tile is still computed by one workgroup, by the same instructions in the same k order.
template <int RS_D, int RS_OCC, bool TRAILING, bool K0MAP = false, bool SBASE = false, bool TICKET = false>
__global__ __launch_bounds__(256, RS_OCC) void gpak_gemm_nt_f64_rs(int K, double alpha, const double *A, long lda,
                                                               const double *B, long ldb, double beta, double *C,
                                                               long ldc, int rb0, int cb0, int lower_skip, int mt,
                                                               int nt, int k0_by_row, int cyc_P, int cyc_rank,
                                                               int cyc_tpb, int cyc_lt0, int super_lr,
                                                               unsigned long long *tk, int nsuper) {
  int ti, tj;
  if constexpr (TICKET) {
    __shared__ int tile_sh;
    if (threadIdx.x == 0) {
      // HW_REG_XCC_ID (hardware register 20), bits 3:0
      const int x = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7;
      int got = -1;
      for (int i = 0; i < 8 && got < 0; i++) {
        const int y = (x + i) & 7;
        const unsigned share = nsuper > y ? 64u * (unsigned)((nsuper - 1 - y) / 8 + 1) : 0u;
        while (true) {
          // a vector global atomic (one lane), device scope: the lists are shared by all XCDs
          const unsigned long long old = atomicAdd(tk + y, i == 0 ? 1ull : (1ull << 32));
          const unsigned f = (unsigned)old, bk = (unsigned)(old >> 32);
          if (f + bk >= share) break;   // list y used up
          const unsigned e = i == 0 ? f : share - 1 - bk;
          int a, c;
          if (gpak_super_tile((int)(e >> 6) * 8 + y, (int)(e & 63), super_lr, lower_skip, mt, nt, rb0, cb0, a, c)) {
            got = a | (c << 16);
            break;
          }
        }
      }
      tile_sh = got;
    }
    __syncthreads();
    const int got = __builtin_amdgcn_readfirstlane(tile_sh);
    if (got < 0) return;
    ti = got & 0xffff;
    tj = got >> 16;
  } else {
    const int b = blockIdx.x, q = b >> 3;
    if (!gpak_super_tile((q >> 6) * 8 + (b & 7), q & 63, super_lr, lower_skip, mt, nt, rb0, cb0, ti, tj)) return;
  }
  int gct = tj, art = ti;
  if (!K0MAP && cyc_P) {
    const int lt = cyc_lt0 + tj;
    gct = ((lt / cyc_tpb) * cyc_P + cyc_rank) * cyc_tpb + (lt % cyc_tpb);
    art = rb0 + ti;
    if (art < gct) return;
  }
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w & 1, wc = w >> 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  if (!TRAILING) __builtin_amdgcn_s_setprio(2);  // panel-chain products go ahead of the bulk update's waves
  const int kstep0 = K0MAP ? (ti * cyc_tpb + cyc_lt0) * (TM / 4) : (k0_by_row ? (rb0 + ti) * (TM / 4) : 0);
  const int nk = K / 4;
  // One 16-B load feeds TWO fragments: lane (l15, l4) fetches rows 32h + 2*l15, +1 of k-column 4s + l4 and
  // uses them as its element of tiles 2h and 2h+1, i.e. MFMA tile i covers the rows 32(i>>1) + 2j + (i&1),
  // j = 0..15, of the wave's 64 -- a fixed permutation that the epilogue undoes (16 lanes = 256 B contiguous).
  // Operand addresses = a wave-uniform 64-bit base in scalar registers, advanced on the SCALAR unit, + a fixed 32-bit
  // lane offset (the SADDR form of global_load): no vector instruction in the loop but the MFMAs and the loads.  Every
  // vector ALU instruction beside the MFMAs holds the matrix pipe for 8-16 cycles (tools/mfma_f32_loop.hip: the fp32
  // loop with the two v_lshl_add_u64 per k-step the compiler makes of per-lane pointers 146 TFLOP/s, with v_add_co
  // pairs 142, with scalar bases 155.6 of 157).  RS_LAUNDER keeps loop-strength reduction from turning base + offset
  // back into per-lane 64-bit pointers.
  // SBASE is chosen by the launcher for the bulk update while the trailing matrix is large (GpakKernelTuning::sbase_rows):
  // alone the kernel gains 1.2-1.6 % at K >= 512 and LOSES 4-13 % at K = 128 / 256 (more issue-stall cycles per wave
  // around the short loop, tools/ab_pmc.sh), and in situ the tighter loop starves the panel chain beside it -- with
  // scalar bases in every bulk update the step was 2 ms SLOWER at N = 32768 and 10 % slower at N = 8192, where the chain
  // is all there is (profiles/r03_scalar_base.txt).
  constexpr bool SB = SBASE;
  const char *Ac = reinterpret_cast<const char *>(A + (size_t)art * TM + wr * 64 + (size_t)(4 * kstep0) * lda);
  const char *Bc = reinterpret_cast<const char *>(B + (size_t)gct * TN + wc * 64 + (size_t)(4 * kstep0) * ldb);
  unsigned aoff = (unsigned)((2 * l15 + (size_t)l4 * lda) * sizeof(double));
  unsigned boff = (unsigned)((2 * l15 + (size_t)l4 * ldb) * sizeof(double));
  const size_t sa = 4 * (size_t)lda * sizeof(double), sb = 4 * (size_t)ldb * sizeof(double);  // 4 k-columns, in bytes
  const char *Apl = Ac + aoff, *Bpl = Bc + boff;   // the per-lane pointers of the !SB build
#define RS_LAUNDER if (SB) asm volatile("" : "+v"(aoff), "+v"(boff));

  d4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};

  d2 ra[RS_D][2], rbv[RS_D][2];
#define RS_LD16(p_) (*reinterpret_cast<const d2 *>(p_))
#define RS_LOAD(slot_)                                                                                          \
  _Pragma("unroll") for (int h = 0; h < 2; h++) ra[slot_][h] = SB ? RS_LD16(Ac + 256 * h + aoff) : RS_LD16(Apl + 256 * h);  \
  _Pragma("unroll") for (int h = 0; h < 2; h++) rbv[slot_][h] = SB ? RS_LD16(Bc + 256 * h + boff) : RS_LD16(Bpl + 256 * h); \
  if (SB) { Ac += sa; Bc += sb; } else { Apl += sa; Bpl += sb; }
#define RS_MFMA(slot_)                                                             \
  _Pragma("unroll") for (int mi = 0; mi < 4; mi++)                                 \
      _Pragma("unroll") for (int ni = 0; ni < 4; ni++)                             \
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(rbv[slot_][ni >> 1][ni & 1], ra[slot_][mi >> 1][mi & 1], \
                                                             acc[mi][ni], 0, 0, 0);

  // ring of RS_D k-steps in flight; n >= 32 k-steps always (K >= 128, k0_by_row leaves >= one tile)
  const int n = nk - kstep0;
#pragma unroll
  for (int s = 0; s < RS_D; s++) { RS_LOAD(s) }
  int g = 0;
  for (; g + 2 * RS_D <= n; g += RS_D) {
    RS_LAUNDER
#pragma unroll
    for (int s = 0; s < RS_D; s++) {
      RS_MFMA(s)
      RS_LOAD(s)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int r = n - (g + RS_D);  // k-steps not yet requested: 0 .. RS_D-1
#pragma unroll
  for (int s = 0; s < RS_D; s++) {
    RS_MFMA(s)
    if (s < r) { RS_LOAD(s) }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < RS_D; s++)
    if (s < r) { RS_MFMA(s) }
#undef RS_LOAD
#undef RS_MFMA
#undef RS_LAUNDER

  // in-place product (the panel solve P <- P * inv^T, one tile column): the workgroup's C rows are its
  // own A rows, which the neighbouring wave is still reading -- the only place the waves must meet
  if (A == C) __syncthreads();
  // lane holds, of tile (mi, ni): C row 32(mi>>1) + 2*l15 + (mi&1), C columns 32(ni>>1) + 2(l4 + 4r) + (ni&1)
  double *Cg = C + (size_t)art * TM + wr * 64 + 2 * l15 + ((size_t)tj * TN + wc * 64) * ldc;
#define RS_COL(ni_, r_) ((size_t)(32 * ((ni_) >> 1) + 2 * (l4 + 4 * (r_)) + ((ni_) & 1)) * ldc)
  if (beta == 0.0) {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int ni = 0; ni < 4; ni++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          d2 v = {alpha * acc[2 * h][ni][r], alpha * acc[2 * h + 1][ni][r]};
          *reinterpret_cast<d2 *>(Cg + 32 * h + RS_COL(ni, r)) = v;
        }
  } else {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int nh = 0; nh < 2; nh++) {
        d2 c[2][4];
#pragma unroll
        for (int n2 = 0; n2 < 2; n2++)
#pragma unroll
          for (int r = 0; r < 4; r++) c[n2][r] = *reinterpret_cast<const d2 *>(Cg + 32 * h + RS_COL(2 * nh + n2, r));
#pragma unroll
        for (int n2 = 0; n2 < 2; n2++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            d2 v;
            if (alpha == -1.0 && beta == 1.0) {
              // every update of the factorisation: c - acc is the same number as fma(-1, acc, 1 * c) in one fp64
              // instruction instead of two (the FMA units these share with the MFMAs are the kernel's bottleneck)
              v = (d2){c[n2][r].x - acc[2 * h][2 * nh + n2][r], c[n2][r].y - acc[2 * h + 1][2 * nh + n2][r]};
            } else {
              v = (d2){fma(alpha, acc[2 * h][2 * nh + n2][r], beta * c[n2][r].x),
                       fma(alpha, acc[2 * h + 1][2 * nh + n2][r], beta * c[n2][r].y)};
            }
            *reinterpret_cast<d2 *>(Cg + 32 * h + RS_COL(2 * nh + n2, r)) = v;
          }
      }
  }
#undef RS_COL
}

// ---------------------------------------------------------------------------------------
// Latency variant of the register-streaming kernel for SMALL tile grids (the panel chain of the
// factorisation: panel solve, in-panel update, update of the next block column near the end).
// A wave of the kernel above needs 16 MFMAs x 64 clk per k-step, i.e. >= 13.6 us for K=128 and
// 54.6 us for K=512 however empty the GPU is.  Here a wave owns 32x32 (4 accumulators), eight waves
// (2x4) cover 64 rows x 128 columns, and a 128x128 tile is spread over two workgroups / 16 waves:
// a quarter of the MFMA chain per wave.  Plain (ti, tj) grid, no super-tiles (nothing to reuse).
// ---------------------------------------------------------------------------------------
// The wave tile shrinks with the grid: MI = 2 m-tiles (32 rows) or 1 (16 rows) per wave, WROWS = 2 or 1 waves along
// the rows, always 4 waves along the 128 columns -- 64, 32 or 16 rows x 128 columns per workgroup.  A panel solve at
// 4096 rows is 64 workgroups of the first kind (2 waves per SIMD, 2 x 128 MFMAs = 7 us of matrix pipe on a quarter of
// the CUs) and 256 of the last (1 wave per SIMD, 64 MFMAs = 1.8 us); the last is the default.
#define RS32_D 8
template <int MI, int WROWS>
__global__ __launch_bounds__(256 * WROWS) void gpak_gemm_nt_f64_rs32(int K, double alpha, const double *A, long lda,
                                                                      const double *B, long ldb, double beta, double *C,
                                                                      long ldc, int rb0, int cb0, int lower_skip, int mtw,
                                                                      int nt, int k0_by_row) {
  constexpr int WGROWS = 16 * MI * WROWS;   // rows per workgroup
  const int tiw = blockIdx.x % mtw, tj = blockIdx.x / mtw;
  const int ti = tiw / (TM / WGROWS);  // 128-row tile index (skip rule and k-start are defined on 128-tiles)
  if (tj >= nt) return;
  if (lower_skip && (rb0 + ti) < (cb0 + tj)) return;
  __builtin_amdgcn_s_setprio(2);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w % WROWS, wc = w / WROWS;  // WROWS x 4 waves
  const int l15 = lane & 15, l4 = lane >> 4;
  const int kstep0 = k0_by_row ? (rb0 + ti) * (TM / 4) : 0;
  const int n = K / 4 - kstep0;
  typedef typename std::conditional<MI == 2, d2, double>::type ta;
  const ta *Ap = reinterpret_cast<const ta *>(A + (size_t)tiw * WGROWS + wr * 16 * MI + MI * l15 + (size_t)(4 * kstep0 + l4) * lda);
  const d2 *Bp = reinterpret_cast<const d2 *>(B + (size_t)tj * TN + wc * 32 + 2 * l15 + (size_t)(4 * kstep0 + l4) * ldb);
  const size_t sa = (4 / (sizeof(ta) / sizeof(double))) * (size_t)lda, sb = 2 * (size_t)ldb;
  d4 acc[MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};
  ta ra[RS32_D];
  d2 rbv[RS32_D];
  auto a_of = [](const ta &v, int mi) -> double {
    if constexpr (MI == 2) return v[mi]; else return v;
  };
#define RS_LOAD(slot_) \
  ra[slot_] = *Ap;     \
  rbv[slot_] = *Bp;    \
  Ap += sa;            \
  Bp += sb;
#define RS_MFMA(slot_)                                                                                       \
  _Pragma("unroll") for (int mi = 0; mi < MI; mi++) _Pragma("unroll") for (int ni = 0; ni < 2; ni++)         \
      acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(rbv[slot_][ni], a_of(ra[slot_], mi), acc[mi][ni], 0, 0, 0);
#pragma unroll
  for (int s = 0; s < RS32_D; s++) { RS_LOAD(s) }  // n >= 32 k-steps always
  int g = 0;
  for (; g + 2 * RS32_D <= n; g += RS32_D) {
#pragma unroll
    for (int s = 0; s < RS32_D; s++) {
      RS_MFMA(s)
      RS_LOAD(s)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int r = n - (g + RS32_D);
#pragma unroll
  for (int s = 0; s < RS32_D; s++) {
    RS_MFMA(s)
    if (s < r) { RS_LOAD(s) }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < RS32_D; s++)
    if (s < r) { RS_MFMA(s) }
#undef RS_LOAD
#undef RS_MFMA
  // in-place panel solve: the workgroup owns its rows across all 128 columns, so one barrier orders
  // every wave's operand reads before anybody's stores
  if (A == C) __syncthreads();
  // lane holds of tile (mi, ni): C row MI*l15 + mi, C columns 2(l4 + 4r) + ni of the wave's (16 MI) x 32
  double *Cg = C + (size_t)tiw * WGROWS + wr * 16 * MI + MI * l15 + ((size_t)tj * TN + wc * 32) * ldc;
#pragma unroll
  for (int ni = 0; ni < 2; ni++)
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
      ta *p = reinterpret_cast<ta *>(Cg + (size_t)(2 * (l4 + 4 * r4) + ni) * ldc);
      if constexpr (MI == 2) {
        d2 v = {alpha * acc[0][ni][r4], alpha * acc[1][ni][r4]};
        if (beta != 0.0) {
          const d2 c = *p;
          if (alpha == -1.0 && beta == 1.0) {   // the in-panel update: one fp64 instruction per element, same number
            v.x = c.x - acc[0][ni][r4];
            v.y = c.y - acc[1][ni][r4];
          } else {
            v.x = fma(alpha, acc[0][ni][r4], beta * c.x);
            v.y = fma(alpha, acc[1][ni][r4], beta * c.y);
          }
        }
        *p = v;
      } else {
        double v = alpha * acc[0][ni][r4];
        if (beta != 0.0) v = (alpha == -1.0 && beta == 1.0) ? *p - acc[0][ni][r4] : fma(alpha, acc[0][ni][r4], beta * *p);
        *p = v;
      }
    }
}

// Trailing update of ALL block columns a rank owns beyond local tile column lt0, in one launch:
// C_local[rows >= rt0*128, local tile columns lt0..] -= Pv[rows] * Pv[global column rows]^T where
// Pv is the panel addressed by global row (virtual base).  See the cyc_* comment in the kernel.
void gpak_launch_gemm_cyclic(hipStream_t st, int mt, int nt, int K, const double *Pv, long ldp, double *Clocal,
                             long ldc, int rt0, int P, int rank, int tpb, int lt0) {
  if (mt <= 0 || nt <= 0) return;
  const int SR = (mt + 7) / 8, SC = (nt + 7) / 8;
  const long nsuper = (long)SR * SC;
  dim3 grid((unsigned)((nsuper + 7) / 8 * 8 * 64)), block(256);
  hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, true>), grid, block, 0, st, K, -1.0, Pv, ldp, Pv, ldp, 1.0, Clocal, ldc,
                     rt0, 0, 0, mt, nt, 0, P, rank, tpb, lt0, 3, nullptr, 0);
}

// C (mt x nt tiles) = alpha * A * B^T with the k-loop of tile row ti started at global row block ti*k0_mul + k0_add
// (A and B are rows of an upper-triangular matrix held in row-cyclic slabs); tile (ti, tj) is skipped when
// ti < tj + skip_shift.
void gpak_launch_gemm_nt_k0map(hipStream_t st, int mt, int nt, int K, double alpha, const double *A, long lda,
                               const double *B, long ldb, double *C, long ldc, int skip_shift, int k0_mul, int k0_add) {
  if (mt <= 0 || nt <= 0) return;
  const int SR = (mt + 7) / 8, SC = (nt + 7) / 8;
  const long nsuper = (long)SR * SC;
  dim3 grid((unsigned)((nsuper + 7) / 8 * 8 * 64)), block(256);
  // lower_skip = 0 in the super-tile walk (every super-tile is visited); the per-tile rule is rb0 + ti < cb0 + tj
  hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, false, true>), grid, block, 0, st, K, alpha, A, lda, B, ldb, 0.0, C, ldc, 0,
                     skip_shift, 2, mt, nt, 0, 0, 0, k0_mul, k0_add, 3, nullptr, 0);
}

void gpak_launch_gemm_nt(hipStream_t st, int mt, int nt, int K, double alpha, const double *A, long lda,
                         const double *B, long ldb, double beta, double *C, long ldc, int row_block0,
                         int col_block0, bool lower_skip, bool trailing, bool k0_by_row, unsigned long long *tickets,
                         int surplus_pct) {
  if (mt <= 0 || nt <= 0) return;
  // super-tile shape: 8 x 8 unless the bulk trailing update was asked for another one (GpakKernelTuning::super_lr)
  int lr = 3;
  if (trailing && lower_skip && row_block0 == col_block0) {
    lr = gpak_tuning().super_lr;
    if (lr < 1 || lr > 5) lr = 3;
  }
  const int lc = 6 - lr;
  const int SR = (mt + (1 << lr) - 1) >> lr, SC = (nt + (1 << lc) - 1) >> lc;
  long nsuper = 0;
  if (lower_skip) {
    for (int sj = 0; sj < SC; sj++) {
      const int cnt = SR - ((sj << lc) >> lr);
      if (cnt <= 0) break;
      nsuper += cnt;
    }
  } else {
    nsuper = (long)SR * SC;
  }
  dim3 grid((unsigned)((nsuper + 7) / 8 * 8 * 64)), block(256);
  const int small_max = gpak_tuning().gemm_small;
  long tiles = (long)mt * nt;
  if (lower_skip) {  // valid lower 128-tiles
    tiles = 0;
    for (int tj = 0; tj < nt; tj++) {
      int first = col_block0 + tj - row_block0;  // first ti with rb0+ti >= cb0+tj
      if (first < 0) first = 0;
      if (first < mt) tiles += mt - first;
    }
  }
  // (the bulk trailing update keeps its own kernel whatever its size: it is never on the panel chain, and
  //  one kernel name per role keeps the rocprofv3 statistics and bench.py's event timing comparable)
  if (!trailing && tiles <= small_max) {
    // rows per workgroup: the finest split measured best at every size (N = 4096: 2.38 / 2.49 / 2.69 ms per step with
    // 16 / 32 / 64, N = 8192: 6.64 / 6.69 / 6.95, N = 32768: 181.9 / 182.0 / 182.6); GPAK_GEMM_SMALL_ROWS for A/B runs
    const int rows = gpak_tuning().gemm_small_rows;
    const int ls = lower_skip ? 1 : 0, kr = k0_by_row ? 1 : 0;
    if (rows == 64)
      hipLaunchKernelGGL((gpak_gemm_nt_f64_rs32<2, 2>), dim3((unsigned)(2 * mt * nt)), dim3(512), 0, st, K, alpha, A, lda, B,
                         ldb, beta, C, ldc, row_block0, col_block0, ls, 2 * mt, nt, kr);
    else if (rows == 32)
      hipLaunchKernelGGL((gpak_gemm_nt_f64_rs32<2, 1>), dim3((unsigned)(4 * mt * nt)), dim3(256), 0, st, K, alpha, A, lda, B,
                         ldb, beta, C, ldc, row_block0, col_block0, ls, 4 * mt, nt, kr);
    else
      hipLaunchKernelGGL((gpak_gemm_nt_f64_rs32<1, 1>), dim3((unsigned)(8 * mt * nt)), dim3(256), 0, st, K, alpha, A, lda, B,
                         ldb, beta, C, ldc, row_block0, col_block0, ls, 8 * mt, nt, kr);
    return;
  }
  // Scalar-base build (SBASE): for the long products that only occur OUTSIDE the factorisation -- K >= 2048: the upper
  // levels of the prediction's substitution ladder, the gradient's G G^T -- where nothing runs beside the kernel and it
  // is 1.2-1.6 % faster; inside the factorisation (K <= 1024) only on request (GpakKernelTuning::sbase_rows, measured slower).
  const int sbase_rows = gpak_tuning().sbase_rows;
  const bool long_k = K >= 2048;
  if (trailing && (long_k || (sbase_rows > 0 && (long)mt * TM > sbase_rows)))
    hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, true, false, true>), grid, block, 0, st, K, alpha, A, lda, B, ldb, beta, C,
                       ldc, row_block0, col_block0, lower_skip ? 1 : 0, mt, nt, k0_by_row ? 1 : 0, 0, 0, 1, 0, lr, nullptr, 0);
  else if (long_k)
    hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, false, false, true>), grid, block, 0, st, K, alpha, A, lda, B, ldb, beta, C,
                       ldc, row_block0, col_block0, lower_skip ? 1 : 0, mt, nt, k0_by_row ? 1 : 0, 0, 0, 1, 0, lr, nullptr, 0);
  else if (trailing && tickets && lower_skip && row_block0 == col_block0 && !k0_by_row) {
    // ticketed map (the factorisation's bulk update): one workgroup per tile plus surplus_pct % more, spread evenly over
    // the XCDs, so that an XCD with more free slots can run more tiles than its eighth; 8 list words at `tickets`, zero
    const long extra = (tiles * (surplus_pct > 0 ? surplus_pct : 0) + 799) / 800;   // per XCD
    hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, true, false, false, true>), dim3((unsigned)(tiles + 8 * extra)), block, 0,
                       st, K, alpha, A, lda, B, ldb, beta, C, ldc, row_block0, col_block0, 1, mt, nt, 0, 0, 0, 1, 0, lr,
                       tickets, (int)nsuper);
  } else if (trailing)
    hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, true>), grid, block, 0, st, K, alpha, A, lda, B, ldb, beta, C, ldc,
                       row_block0, col_block0, lower_skip ? 1 : 0, mt, nt, k0_by_row ? 1 : 0, 0, 0, 1, 0, lr, nullptr, 0);
  else
    hipLaunchKernelGGL((gpak_gemm_nt_f64_rs<4, 2, false>), grid, block, 0, st, K, alpha, A, lda, B, ldb, beta, C, ldc,
                       row_block0, col_block0, lower_skip ? 1 : 0, mt, nt, k0_by_row ? 1 : 0, 0, 0, 1, 0, lr, nullptr, 0);
}

// ---------------------------------------------------------------------------------------
// Calibration microbenchmarks: back-to-back fp64 MFMA issue and a
// streaming 16-B store, so roofline fractions can be quoted against measured ceilings too.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void gpak_calib_mfma_f64(double *out, int iters) {
  // the register-level shape of the GEMM's inner step: 4 A x 4 B fragments -> 16 accumulators
  d4 acc[4][4];
  double a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    a[i] = 1.0 + (threadIdx.x + 7 * i) * 1e-9;
    b[i] = 1.0 - (threadIdx.x + 3 * i) * 1e-9;
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  }
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[j], a[i], acc[i][j], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  if (s == 12345.678) out[0] = s;  // keep the chain live
}

__global__ __launch_bounds__(256) void gpak_calib_store(double2 *out, size_t n2) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n2; i += stride) out[i] = make_double2(1.0, 2.0);
}

int gpak_calibrate_impl(gpak_ctx *ctx, double *scratch, size_t scratch_bytes, double *tflops, double *gbs) {
  hipEvent_t e0, e1;
  GPAK_HIP(hipEventCreate(&e0));
  GPAK_HIP(hipEventCreate(&e1));
  const int iters = 32768, blocks = 256 * 2;  // 2 workgroups per CU like the GEMM; ~30 ms so that the clock has settled
  hipLaunchKernelGGL(gpak_calib_mfma_f64, dim3(blocks), dim3(256), 0, ctx->stream, scratch, iters / 2);
  GPAK_HIP(hipEventRecord(e0, ctx->stream));
  hipLaunchKernelGGL(gpak_calib_mfma_f64, dim3(blocks), dim3(256), 0, ctx->stream, scratch, iters);
  GPAK_HIP(hipEventRecord(e1, ctx->stream));
  GPAK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  GPAK_HIP(hipEventElapsedTime(&ms, e0, e1));
  double flops = (double)blocks * 4 /*waves*/ * iters * 16.0 * (2.0 * 16 * 16 * 4);
  *tflops = flops / (ms * 1e-3) / 1e12;
  size_t n2 = scratch_bytes / 16;
  // 16384 workgroups over a buffer far larger than the 256 MiB Infinity Cache: 5.5-5.7 TB/s on MI355X (2048 workgroups
  // over 1 GiB, the round-1 yardstick, gave 4.4-5.2; tools/store_bw.hip has the sweep)
  hipLaunchKernelGGL(gpak_calib_store, dim3(16384), dim3(256), 0, ctx->stream, (double2 *)scratch, n2);
  GPAK_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 4; r++)
    hipLaunchKernelGGL(gpak_calib_store, dim3(16384), dim3(256), 0, ctx->stream, (double2 *)scratch, n2);
  GPAK_HIP(hipEventRecord(e1, ctx->stream));
  GPAK_HIP(hipEventSynchronize(e1));
  GPAK_HIP(hipEventElapsedTime(&ms, e0, e1));
  *gbs = 4.0 * (double)(n2 * 16) / (ms * 1e-3) / 1e9;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return GPAK_OK;
}
