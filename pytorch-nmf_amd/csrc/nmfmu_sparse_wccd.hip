// Weighted CCD: the coordinate-descent sweep of nmfmu_sparse_ccd.hip for a target whose UNSTORED entries are zeros observed
// with a confidence omega, 0 < omega < 1 (Hu, Koren, Volinsky 2008; He et al. 2016 with a uniform missing weight) -- the
// beta = 2 half-step of NMF.fit(solver='ccd', unstored=omega), DESIGN.md section 27.  Owner F, panel P (the other factor,
// fixed), gram = P^T P [rank][rank] (nmfmu_gram: symmetric; coordinate k reads its row k only), c = 1 - omega.  Every owner
// row i with stored entries e (panel row j_e, value v_e), on its own -- a row WITHOUT entries too: the Gram term acts on it:
//
//   t_e = fma(-c, s_e, v_e),   s_e = sum_k F[i][k] P[j_e][k]                     (k ascending, one fmaf chain from 0)
//   for k = 0 .. R-1:  d = sum_e P[j_e][k]^2,   n = sum_e t_e P[j_e][k],   q = sum_j F[i][j] gram[k][j]
//                                                                           (j < k: the values this pass wrote; j >= k: old)
//                      D   = fma(c, d, omega * gram[k][k])
//                      num = fma(F[i][k], D, fma(-omega, q, n)) - l1
//                      f'  = max(eps, num / ((D + l2) + eps))
//                      t_e = fma(-(c * (f' - F[i][k])), P[j_e][k], t_e) for every e;   F[i][k] = f'
//
// the exact minimiser along coordinate k of 1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 + l1 sum f + l2/2 |f|^2,
// floored at eps.  c = 1.0f - omega is formed once on the host, in fp32.
//
// Work split, lane layout, the d and n reductions and the place of the residuals are those of nmfmu_sparse_ccd.hip: a row of
// at most wg_rows entries is worked by one wave, a longer one by a workgroup of kWccdWgWaves waves (two launches over one
// order list; which one takes a row is a function of its count and wg_rows -- a row without entries is a one-wave row); with
// NW waves on the row, entry e belongs to lane e mod 64 of wave (e / 64) mod NW as slot e / (64 NW); d and n are per-lane
// fmaf chains over the slots in ascending order, an xor butterfly 32 .. 1 per wave and, with NW > 1, the waves' totals added
// in wave order ((w0 + w1) + w2) + ... by every thread.  A row of at most limit NW entries keeps residuals, indices and the
// coordinate's panel values in registers, a longer one keeps the residuals in ITS slice of scratch; both do the same
// operations in the same order.  P[j_e][k] is gathered from the row-major panel.
//
// q, the third reduction: lane l holds the owner row's coordinates l, l + 64, l + 128, l + 192 in registers and runs
// q = fma(F[i][l + 64 m], gram[k][l + 64 m], q) for m = 0 .. 3 (ascending j, coordinates beyond the rank left out), then the
// same butterfly 32 .. 1, interleaved with the other two.  With NW > 1 every wave computes q on its own from its own
// registers: the same operands in the same order, identical bits, nothing to exchange.
//
// Why the owner row is race-free.  The row is copied to LDS (fs) before the sweep's first barrier and fs is NOT written
// again: it holds the OLD row, read for s_e and as F[i][k] of coordinate k (coordinate k is still old when it is updated).
// The new values live in registers: after the reductions every thread of the workgroup holds the same d, n, q and the same
// old F[i][k], so every thread computes the same f', and lane k mod 64 of EVERY wave puts it into its register slot k / 64.
// No thread ever reads an owner value another thread wrote, so the row needs no barrier of its own; the only LDS traffic
// in the loop is the waves' d / n totals, whose buffer alternates with the coordinate's parity (a wave can write buffer
// k + 2 only after the barrier of coordinate k + 1, which every wave passes after it has read buffer k).  Wave 0 stores
// the row from its registers at the end.
//
// Plain vector stores, no atomics, no fences: the owner row is written by its own wave or workgroup; panel / gram / idx /
// vals are only read.  A row's bits depend on that row, its entries, panel, gram, omega, l1, l2 and wg_rows alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr float kWccdEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps
constexpr int kWccdSlots = 8;                         // residuals a lane keeps in registers
constexpr int kWccdLimit = 64 * kWccdSlots;           // = nmfmu_sp_ccd_limit()
constexpr int kWccdWgWaves = 16;                      // = nmfmu_sp_ccd_wg_waves()
constexpr int kWccdOwn = 4;                           // owner coordinates a lane holds: rank <= 256

struct WccdArgs {
  const int32_t* rowptr;
  const int32_t* idx;
  const float* vals;
  const int32_t* order;    // NULL: rows in their own order
  float* owner;
  const float* panel;
  const float* gram;       // [rank][rank]
  float* scratch;          // [nnz]
  int n_rows, n_panel, rank, limit, wg_rows;
  float omega, c, l1, l2;
};

// REG: residuals, panel-row indices and the coordinate's panel values in registers (at most kWccdSlots slots per lane);
// otherwise residuals in scratch[p0 .. p0 + cnt), indices re-read.  fs: the OLD owner row in LDS, read only; fr: this
// lane's coordinates of the row, new below the current coordinate; red: [2][2][NW] floats of LDS (NW > 1).
template <bool REG, int NW>
__device__ __forceinline__ void wccd_row(const WccdArgs& a, int p0, int cnt, const float* fs, float (&fr)[kWccdOwn],
                                         float* red, int lane, int wave) {
  const int rank = a.rank;
  const float c = a.c, omega = a.omega;
  const int T = (cnt + 64 * NW - 1) / (64 * NW);
  const int first = 64 * wave + lane;      // this lane's entry of slot 0; slot t: first + 64 NW t
  const int32_t* __restrict__ idx = a.idx + p0;
  const float* __restrict__ panel = a.panel;
  float* res = a.scratch + p0;
  float r[kWccdSlots], pk[kWccdSlots];
  int col[kWccdSlots];

  // t_e = v_e - c <F[i], P[j_e]>
  if constexpr (REG) {
#pragma unroll
    for (int t = 0; t < kWccdSlots; ++t) {
      const int e = first + 64 * NW * t;
      r[t] = 0.f, col[t] = 0;
      if (e < cnt) {
        col[t] = idx[e];
        float s = 0.f;
        for (int k = 0; k < rank; ++k) s = fmaf(fs[k], panel[(size_t)col[t] * rank + k], s);
        r[t] = fmaf(-c, s, a.vals[p0 + e]);
      }
    }
  } else {
    for (int t = 0; t < T; ++t) {
      const int e = first + 64 * NW * t;
      if (e < cnt) {
        const int cj = idx[e];
        float s = 0.f;
        for (int k = 0; k < rank; ++k) s = fmaf(fs[k], panel[(size_t)cj * rank + k], s);
        res[e] = fmaf(-c, s, a.vals[p0 + e]);
      }
    }
  }

  for (int k = 0; k < rank; ++k) {
    const float f = fs[k];
    const float* __restrict__ gk = a.gram + (size_t)k * rank;
    float d = 0.f, n = 0.f, q = 0.f;
#pragma unroll
    for (int m = 0; m < kWccdOwn; ++m) {
      const int j = lane + 64 * m;
      if (j < rank) q = fmaf(fr[m], gk[j], q);
    }
    if constexpr (REG) {
#pragma unroll
      for (int t = 0; t < kWccdSlots; ++t) {
        const int e = first + 64 * NW * t;
        pk[t] = 0.f;
        if (e < cnt) {
          pk[t] = panel[(size_t)col[t] * rank + k];
          d = fmaf(pk[t], pk[t], d);
          n = fmaf(r[t], pk[t], n);
        }
      }
    } else {
#pragma unroll 4      // four slots' loads in flight; the chains stay t-ordered
      for (int t = 0; t < T; ++t) {
        const int e = first + 64 * NW * t;
        if (e < cnt) {
          const float p = panel[(size_t)idx[e] * rank + k];
          d = fmaf(p, p, d);
          n = fmaf(res[e], p, n);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // the three butterflies interleaved: three shuffles in flight
      d += __shfl_xor(d, o, 64);
      n += __shfl_xor(n, o, 64);
      q += __shfl_xor(q, o, 64);
    }
    if constexpr (NW > 1) {              // the waves' totals in wave order; the buffer alternates: one barrier per coordinate
      float* rd = red + (k & 1) * 2 * NW;
      if (lane == 0) rd[wave] = d, rd[NW + wave] = n;
      __syncthreads();
      d = rd[0], n = rd[NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) d += rd[w], n += rd[NW + w];
    }
    const float D = fmaf(c, d, omega * gk[k]);
    const float num = fmaf(f, D, fmaf(-omega, q, n)) - a.l1;
    const float den = (D + a.l2) + kWccdEps;
    const float fn = fmaxf(kWccdEps, num / den);   // (a NaN quotient gives eps)
    const float back = -(c * (fn - f));
    if constexpr (REG) {
#pragma unroll
      for (int t = 0; t < kWccdSlots; ++t)
        if (first + 64 * NW * t < cnt) r[t] = fmaf(back, pk[t], r[t]);
    } else {
#pragma unroll 4
      for (int t = 0; t < T; ++t) {
        const int e = first + 64 * NW * t;
        if (e < cnt) res[e] = fmaf(back, panel[(size_t)idx[e] * rank + k], res[e]);
      }
    }
#pragma unroll
    for (int m = 0; m < kWccdOwn; ++m)   // every thread holds the same f': the lane that owns coordinate k keeps it
      if (lane + 64 * m == k) fr[m] = fn;
  }
}

// NW == 1: the rows of at most wg_rows entries (those without entries among them), one wave each; NW > 1: the longer rows,
// one workgroup each.  Every decision before a barrier is a function of the row's count: uniform over the workgroup.
template <int NW>
__global__ void __launch_bounds__(64 * NW) sp_wccd_sweep_kernel(WccdArgs a) {
  __shared__ __attribute__((aligned(16))) float fs[256];
  __shared__ float red[NW > 1 ? 4 * NW : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int at = blockIdx.x;
  if (at >= a.n_rows) return;
  const int row = a.order ? a.order[at] : at;
  const int p0 = a.rowptr[row], cnt = a.rowptr[row + 1] - p0;
  if ((cnt > a.wg_rows) != (NW > 1)) return;   // the other launch's row
  const int rank = a.rank;
  float* frow = a.owner + (size_t)row * rank;
  float fr[kWccdOwn];
#pragma unroll
  for (int m = 0; m < kWccdOwn; ++m) {
    const int j = lane + 64 * m;
    fr[m] = j < rank ? frow[j] : 0.f;
    if (wave == 0 && j < rank) fs[j] = fr[m];
  }
  __syncthreads();
  if (cnt <= a.limit * NW) wccd_row<true, NW>(a, p0, cnt, fs, fr, red, lane, wave);
  else wccd_row<false, NW>(a, p0, cnt, fs, fr, red, lane, wave);
  if (wave == 0) {
#pragma unroll
    for (int m = 0; m < kWccdOwn; ++m) {
      const int j = lane + 64 * m;
      if (j < rank) frow[j] = fr[m];
    }
  }
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_sp_wccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, int n_rows,
                        float* owner, const float* panel, int n_panel, int rank, const float* gram, float omega, float l1,
                        float l2, float* scratch, int limit, int wg_rows, void* stream) {
  if (!rowptr || !idx || !vals || !owner || !panel || !gram || !scratch || owner == panel) return NMFMU_ERR_ARG;
  if (n_rows < 0 || n_panel <= 0 || rank <= 0 || limit < 0 || limit > kWccdLimit || wg_rows < 0) return NMFMU_ERR_ARG;
  if (!(omega > 0.f && omega < 1.f)) return NMFMU_ERR_ARG;   // (a NaN fails both comparisons)
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (n_rows == 0) return NMFMU_OK;
  WccdArgs a;
  a.rowptr = rowptr, a.idx = idx, a.vals = vals, a.order = order, a.owner = owner, a.panel = panel, a.gram = gram;
  a.scratch = scratch;
  a.n_rows = n_rows, a.n_panel = n_panel, a.rank = rank;
  a.limit = limit == 0 ? kWccdLimit : limit;
  a.wg_rows = wg_rows == 0 ? kWccdLimit : wg_rows;
  a.omega = omega, a.c = 1.0f - omega, a.l1 = l1, a.l2 = l2;
  // the long rows first: they are the launch's tail
  hipLaunchKernelGGL(sp_wccd_sweep_kernel<kWccdWgWaves>, dim3((unsigned)n_rows), dim3(64 * kWccdWgWaves), 0, S(stream), a);
  hipLaunchKernelGGL(sp_wccd_sweep_kernel<1>, dim3((unsigned)n_rows), dim3(64), 0, S(stream), a);
  return (int)hipGetLastError();
}

}  // extern "C"
