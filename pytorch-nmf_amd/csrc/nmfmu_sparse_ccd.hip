// CCD: cyclic coordinate descent over the rank on the STORED entries of a sparse target, with a maintained residual (Yu,
// Hsieh, Si, Dhillon, ICDM 2012) -- the beta = 2 half-step of NMF.fit(solver='ccd', unstored='missing'), DESIGN.md section 26.
// Owner F (H or W), panel P (the other factor, fixed).  Every owner row i with stored entries e (panel row j_e, value v_e),
// on its own:
//
//   r_e = v_e - s_e,   s_e = sum_k F[i][k] P[j_e][k]                      (k ascending, one fmaf chain from 0)
//   for k = 0 .. R-1:  d = sum_e P[j_e][k]^2,   n = sum_e r_e P[j_e][k]
//                      f' = max(eps, (fma(F[i][k], d, n) - l1) / ((d + l2) + eps))
//                      r_e = fma(-(f' - F[i][k]), P[j_e][k], r_e) for every e;   F[i][k] = f'
//
// n + F[i][k] d is the numerator of the HALS sweep for the row's own Gram matrix (the W rows of ITS stored columns only).
// A row without entries is not touched.
//
// A row of at most wg_rows entries is worked by one wave (= one workgroup of 64 threads), a longer one by a workgroup of
// kCcdWgWaves waves (a second launch over the same order list; each launch leaves the other's rows alone, so which path a
// row takes is a function of its count and wg_rows only).  Rows are handed out through `order` (longest first).  The lanes
// run across the entries: with NW waves on the row, entry e belongs to lane e mod 64 of wave (e / 64) mod NW, as that lane's
// slot e / (64 NW).  d and n are per-lane fmaf chains over the lane's slots in ascending order, then a fixed-order xor
// butterfly 32 .. 1 per wave -- after it every lane of the wave holds the same bits -- and, with NW > 1, the waves' totals
// go through LDS and are added in wave order by every thread: ((w0 + w1) + w2) + ...
//
// Where the residuals live: a row of at most limit NW (limit <= 64 kCcdSlots) entries keeps them -- and its panel-row
// indices, and P[j_e][k] between the reduction and the update -- in registers; a longer row keeps them in ITS slice
// scratch[p_begin .. p_end) of an fp32 buffer of nnz floats, which only this row's wave or workgroup reads and writes
// (every lane its own entries).  Both do the same operations in the same order: a row's bits do not depend on `limit`.
//
// Where P[j_e][k] comes from -- three sources of the same float, so no bit depends on the choice:
//   stage   the row's panel rows copied once to LDS, row stride rank | 1 (odd: the 32 lanes of a ds_read_b32 group hit 32
//           banks), for a one-wave row of at most lds_rows entries;
//   pt      a transposed copy pt [rank][n_panel], made by this entry once per call: coordinate k gathers from one contiguous
//           vector of n_panel floats;
//   panel   the row-major panel itself (pt == NULL).
// Which one a row uses is a function of its count, lds_rows, wg_rows and pt == NULL alone.
//
// Plain vector stores, no atomics, no fences: the owner row is written by its own wave or workgroup, panel / idx / vals are
// only read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr float kCcdEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps
constexpr int kCcdSlots = 8;                         // residuals a lane keeps in registers
constexpr int kCcdLimit = 64 * kCcdSlots;            // = nmfmu_sp_ccd_limit()
constexpr int kCcdWgWaves = 16;                      // waves of the workgroup a long row takes
constexpr int kCcdLdsFloats = 10240;                 // 40 KiB of staged panel rows per wave: four row-waves per CU
constexpr int kCcdStageU = 4;                        // panel rows in flight while staging

enum { kCcdStage = 0, kCcdPt = 1, kCcdPanel = 2 };

struct CcdArgs {
  const int32_t* rowptr;
  const int32_t* idx;
  const float* vals;
  const int32_t* order;    // NULL: rows in their own order
  float* owner;
  const float* panel;
  const float* pt;         // [rank][n_panel] or NULL
  float* scratch;          // [nnz]
  int n_rows, n_panel, rank, limit, lds_rows, wg_rows;
  float l1, l2;
};

template <int SRC>
__device__ __forceinline__ float ccd_p(const CcdArgs& a, const float* stage, int e, int col, int k) {
  if constexpr (SRC == kCcdStage) return stage[e * (a.rank | 1) + k];
  else if constexpr (SRC == kCcdPt) return a.pt[(size_t)k * a.n_panel + col];
  else return a.panel[(size_t)col * a.rank + k];
}

// f' of one coordinate from the wave's totals; every lane computes the same bits
__device__ __forceinline__ float ccd_minimiser(float f, float d, float n, float l1, float l2) {
  const float num = fmaf(f, d, n) - l1;
  const float den = (d + l2) + kCcdEps;
  return fmaxf(kCcdEps, num / den);   // (a NaN quotient gives eps)
}

// REG: the residuals, the panel-row indices and the coordinate's panel values of the row live in registers (at most
// kCcdSlots slots per lane); otherwise residuals in scratch[p0 .. p0 + cnt), indices re-read.  fs: the owner row in LDS;
// red: [2][2][NW] floats of LDS for the waves' totals (NW > 1).
template <bool REG, int SRC, int NW>
__device__ __forceinline__ void ccd_row(const CcdArgs& a, int p0, int cnt, float* fs, float* red, const float* stage,
                                        int lane, int wave) {
  const int rank = a.rank;
  const int T = (cnt + 64 * NW - 1) / (64 * NW);
  const int first = 64 * wave + lane;      // this lane's entry of slot 0; slot t: first + 64 NW t
  const int32_t* __restrict__ idx = a.idx + p0;
  float* res = a.scratch + p0;
  float r[kCcdSlots], pk[kCcdSlots];
  int col[kCcdSlots];

  // r_e = v_e - <F[i], P[j_e]>
  if constexpr (REG) {
#pragma unroll
    for (int t = 0; t < kCcdSlots; ++t) {
      const int e = first + 64 * NW * t;
      r[t] = 0.f, col[t] = 0;
      if (e < cnt) {
        col[t] = idx[e];
        float s = 0.f;
        for (int k = 0; k < rank; ++k) s = fmaf(fs[k], ccd_p<SRC>(a, stage, e, col[t], k), s);
        r[t] = a.vals[p0 + e] - s;
      }
    }
  } else {
    for (int t = 0; t < T; ++t) {
      const int e = first + 64 * NW * t;
      if (e < cnt) {
        const int c = idx[e];
        float s = 0.f;
        for (int k = 0; k < rank; ++k) s = fmaf(fs[k], ccd_p<SRC>(a, stage, e, c, k), s);
        res[e] = a.vals[p0 + e] - s;
      }
    }
  }

  for (int k = 0; k < rank; ++k) {
    const float f = fs[k];
    float d = 0.f, n = 0.f;
    if constexpr (REG) {
#pragma unroll
      for (int t = 0; t < kCcdSlots; ++t) {
        const int e = first + 64 * NW * t;
        pk[t] = 0.f;
        if (e < cnt) {
          pk[t] = ccd_p<SRC>(a, stage, e, col[t], k);
          d = fmaf(pk[t], pk[t], d);
          n = fmaf(r[t], pk[t], n);
        }
      }
    } else {
#pragma unroll 4      // four slots' loads in flight; the chains stay t-ordered
      for (int t = 0; t < T; ++t) {
        const int e = first + 64 * NW * t;
        if (e < cnt) {
          const float p = ccd_p<SRC>(a, stage, e, idx[e], k);
          d = fmaf(p, p, d);
          n = fmaf(res[e], p, n);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // the two butterflies interleaved: two shuffles in flight
      d += __shfl_xor(d, o, 64);
      n += __shfl_xor(n, o, 64);
    }
    if constexpr (NW > 1) {              // the waves' totals in wave order; the buffer alternates: one barrier per coordinate
      float* rd = red + (k & 1) * 2 * NW;
      if (lane == 0) rd[wave] = d, rd[NW + wave] = n;
      __syncthreads();
      d = rd[0], n = rd[NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) d += rd[w], n += rd[NW + w];
    }
    const float fn = ccd_minimiser(f, d, n, a.l1, a.l2);
    const float back = -(fn - f);
    if constexpr (REG) {
#pragma unroll
      for (int t = 0; t < kCcdSlots; ++t)
        if (first + 64 * NW * t < cnt) r[t] = fmaf(back, pk[t], r[t]);
    } else {
#pragma unroll 4
      for (int t = 0; t < T; ++t) {
        const int e = first + 64 * NW * t;
        if (e < cnt) res[e] = fmaf(back, ccd_p<SRC>(a, stage, e, idx[e], k), res[e]);
      }
    }
    if (lane == 0 && wave == 0) fs[k] = fn;   // (coordinate k is not read again in this sweep)
  }
}

template <int SRC, int NW>
__device__ __forceinline__ void ccd_row_any(const CcdArgs& a, int p0, int cnt, float* fs, float* red, const float* stage,
                                            int lane, int wave) {
  if (cnt <= a.limit * NW) ccd_row<true, SRC, NW>(a, p0, cnt, fs, red, stage, lane, wave);
  else ccd_row<false, SRC, NW>(a, p0, cnt, fs, red, stage, lane, wave);
}

// NW == 1: the rows of at most wg_rows entries, one wave each; NW > 1: the longer rows, one workgroup each.  Every decision
// before a barrier is a function of the row's count: uniform over the workgroup.
template <int NW>
__global__ void __launch_bounds__(64 * NW) sp_ccd_sweep_kernel(CcdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ccd_lds[];
  float* fs = ccd_lds;            // [256]
  float* red = ccd_lds + 256;     // NW > 1: [2][2][NW]
  float* stage = ccd_lds + 256;   // NW == 1: [lds_rows][rank | 1]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int at = blockIdx.x;
  if (at >= a.n_rows) return;
  const int row = a.order ? a.order[at] : at;
  const int p0 = a.rowptr[row], cnt = a.rowptr[row + 1] - p0;
  if (cnt <= 0) return;           // a row without data stays as it is
  if ((cnt > a.wg_rows) != (NW > 1)) return;   // the other launch's row
  const int rank = a.rank, S = rank | 1;
  float* frow = a.owner + (size_t)row * rank;
  for (int c = threadIdx.x; c < rank; c += 64 * NW) fs[c] = frow[c];
  bool staged = false;
  if constexpr (NW == 1) {
    staged = cnt <= a.lds_rows;
    if (staged) {
      for (int e0 = 0; e0 < cnt; e0 += kCcdStageU) {
        float b[kCcdStageU][4];
#pragma unroll
        for (int u = 0; u < kCcdStageU; ++u) {
          const bool ok = e0 + u < cnt;
          const int c = ok ? a.idx[p0 + e0 + u] : 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            b[u][q] = (ok && k < rank) ? a.panel[(size_t)c * rank + k] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < kCcdStageU; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            if (e0 + u < cnt && k < rank) stage[(e0 + u) * S + k] = b[u][q];
          }
      }
    }
  }
  __syncthreads();
  if (staged) ccd_row_any<kCcdStage, NW>(a, p0, cnt, fs, red, stage, lane, wave);
  else if (a.pt) ccd_row_any<kCcdPt, NW>(a, p0, cnt, fs, red, stage, lane, wave);
  else ccd_row_any<kCcdPanel, NW>(a, p0, cnt, fs, red, stage, lane, wave);
  __syncthreads();
  for (int c = threadIdx.x; c < rank; c += 64 * NW) frow[c] = fs[c];
}

// pt[k][j] = p[j][k], 32 x 32 tiles through LDS (pitch 33)
__global__ void __launch_bounds__(256) sp_ccd_transpose_kernel(const float* __restrict__ p, float* __restrict__ pt, int n,
                                                               int rank) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int j0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  for (int i = ty; i < 32; i += 8)
    if (j0 + i < n && k0 + tx < rank) tile[i][tx] = p[(size_t)(j0 + i) * rank + k0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (k0 + i < rank && j0 + tx < n) pt[(size_t)(k0 + i) * n + j0 + tx] = tile[tx][i];
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_sp_ccd_limit(void) { return kCcdLimit; }

int nmfmu_sp_ccd_wg_waves(void) { return kCcdWgWaves; }

int nmfmu_sp_ccd_lds_rows(int rank) {
  if (rank <= 0 || rank > 256) return 0;
  return kCcdLdsFloats / (rank | 1);
}

int nmfmu_sp_ccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, int n_rows,
                       float* owner, const float* panel, int n_panel, int rank, float l1, float l2, float* scratch,
                       float* panel_t, int limit, int lds_rows, int wg_rows, void* stream) {
  if (!rowptr || !idx || !vals || !owner || !panel || !scratch || owner == panel) return NMFMU_ERR_ARG;
  if (n_rows < 0 || n_panel <= 0 || rank <= 0 || limit < 0 || limit > kCcdLimit || lds_rows < 0 ||
      wg_rows < 0)
    return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (n_rows == 0) return NMFMU_OK;
  const int cap = kCcdLdsFloats / (rank | 1);
  CcdArgs a;
  a.rowptr = rowptr, a.idx = idx, a.vals = vals, a.order = order, a.owner = owner, a.panel = panel, a.pt = panel_t;
  a.scratch = scratch;
  a.n_rows = n_rows, a.n_panel = n_panel, a.rank = rank;
  a.limit = limit == 0 ? kCcdLimit : limit;
  a.lds_rows = lds_rows < cap ? lds_rows : cap;
  a.wg_rows = wg_rows == 0 ? kCcdLimit : wg_rows;
  a.l1 = l1, a.l2 = l2;
  if (panel_t) {
    const dim3 grid((unsigned)((n_panel + 31) / 32), (unsigned)((rank + 31) / 32));
    hipLaunchKernelGGL(sp_ccd_transpose_kernel, grid, dim3(256), 0, S(stream), panel, panel_t, n_panel, rank);
  }
  // the long rows first: they are the launch's tail
  hipLaunchKernelGGL(sp_ccd_sweep_kernel<kCcdWgWaves>, dim3((unsigned)n_rows), dim3(64 * kCcdWgWaves),
                     (256 + 4 * kCcdWgWaves) * sizeof(float), S(stream), a);
  const size_t lds_bytes = (size_t)(256 + a.lds_rows * (rank | 1)) * sizeof(float);
  hipLaunchKernelGGL(sp_ccd_sweep_kernel<1>, dim3((unsigned)n_rows), dim3(64), lds_bytes, S(stream), a);
  return (int)hipGetLastError();
}

}  // extern "C"
