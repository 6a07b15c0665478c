// The tile pieces the exact-fp32 MFMA kernels on the fp32 masters share: the weighted dense kernels (nmfmu_wmu.hip) and their
// batched siblings, unweighted and weighted (nmfmu_bmu.hip).  A workgroup (4 waves) owns 128 owner rows x a rank tile of
// <= 128 x one part of the contraction axis; a stage is 32 contraction steps.  Here: the tile plan (WmuCfg), the split rule of
// the contraction, the owner rows in registers, the panel rows on their way to LDS, Y = owner x panel over the full padded
// rank, the weighted stage (V and M on their way to LDS) and the dispatch over the padded rank.  A kernel's seeds and its
// epilogue stay in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "nmfmu_fused.h"

namespace nmfmu {

constexpr int kWmBK = 32;            // contraction steps per stage; a part is a whole number of stages
constexpr int kWmRows = 128;         // owner rows per workgroup
constexpr int kWmLDA = kWmBK + 1;    // sv / sm [i][c]: lanes read a column (second product) or a row (elementwise) conflict free
constexpr int kWmTargetWgs = 512;    // two workgroups on each of the 256 CUs
constexpr int kWmMinStages = 4;      // the library's own parts are at least 128 contraction steps long ...
constexpr int kWmMaxSplit = 64;      // ... and there are at most 64 of them

template <int RP>
struct WmuCfg {
  static constexpr int RT = RP < 128 ? RP : 128;   // rank tile of the two accumulators (grid.y tiles cover r_pad)
  static constexpr int WN = RT >= 64 ? 2 : 1;      // waves across the rank tile
  static constexpr int WM = 4 / WN;                // waves across the 128 owner rows
  static constexpr int TM = 4 / WM;                // 32 x 32 tiles per wave along the rows
  static constexpr int TN = RT / (WN * 32);        // ... and along the rank
  static constexpr int LDB = RP + 1;               // sb [c][r]: the first product reads a column of it per lane
};

inline int wmu_stages(int contraction) { return (contraction + kWmBK - 1) / kWmBK; }

// parts for a wanted split count >= 1: no empty part, only the last one may be short
inline int wmu_parts(int contraction, int nsplit) {
  const int stages = wmu_stages(contraction);
  const int n = std::max(1, std::min(nsplit, stages));
  const int per = (stages + n - 1) / n;
  return (stages + per - 1) / per;
}
inline int wmu_part_len(int contraction, int parts) { return (wmu_stages(contraction) + parts - 1) / parts * kWmBK; }

inline int wmu_auto_split(int64_t tiles, int contraction) {
  const int64_t want = (kWmTargetWgs + tiles - 1) / tiles;
  const int cap = std::max(1, wmu_stages(contraction) / kWmMinStages);
  return wmu_parts(contraction, (int)std::min<int64_t>(std::min<int64_t>(want, cap), kWmMaxSplit));
}
inline int wmu_split(int rows, int contraction, int r_pad, int nsplit) {
  if (nsplit > 0) return wmu_parts(contraction, nsplit);
  return wmu_auto_split((int64_t)((rows + kWmRows - 1) / kWmRows) * ((r_pad + 127) / 128), contraction);
}

// the lane's owner row (row 32 wave + j of the tile), rank slots 2 s + hl: the A operand of the first product
template <int RP>
__device__ __forceinline__ void wmu_load_owner(float (&a)[RP / 2], const float* owner, int rows, int rank, int row, int hl) {
#pragma unroll
  for (int s = 0; s < RP / 2; ++s) {
    const int r = 2 * s + hl;
    a[s] = (row < rows && r < rank) ? owner[(size_t)row * rank + r] : 0.f;
  }
}

// bv -> sb [c][r] = panel[c0 + c][r] over the full padded rank; zero in the padded columns and past the part.  St: the
// kernel's stage registers, with bv[kWmBK * RP / 256]
template <int RP, class St>
__device__ __forceinline__ void wmu_load_panel(St& st, const float* __restrict__ panel, int rank, int c0, int cend, int tid) {
#pragma unroll
  for (int p = 0; p < kWmBK * RP / 256; ++p) {
    const int idx = p * 256 + tid;
    const int c = c0 + idx / RP, r = idx % RP;
    st.bv[p] = (c < cend && r < rank) ? panel[(size_t)c * rank + r] : 0.f;
  }
}

template <int RP, class St>
__device__ __forceinline__ void wmu_store_panel(float* sb, const St& st, int tid) {
#pragma unroll
  for (int p = 0; p < kWmBK * RP / 256; ++p) {
    const int idx = p * 256 + tid;
    sb[(idx / RP) * WmuCfg<RP>::LDB + idx % RP] = st.bv[p];
  }
}

// Y[row (e & 3) + 8 (e >> 2) + 4 hl of the wave's 32][contraction step j] = sum_r owner[row][r] panel[c0 + j][r], r ascending
template <int RP>
__device__ __forceinline__ f32x16 wmu_form_y(const float (&a)[RP / 2], const float* sb, int j, int hl) {
  f32x16 y;
#pragma unroll
  for (int e = 0; e < 16; ++e) y[e] = 0.f;
  const float* pb = sb + j * WmuCfg<RP>::LDB + hl;
#pragma unroll
  for (int s = 0; s < RP / 2; ++s) y = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], pb[2 * s], y, 0, 0, 0);
  return y;
}

__device__ __forceinline__ int wmu_tile_row(int e, int hl) { return (e & 3) + 8 * (e >> 2) + 4 * hl; }

// A stage's V / M (128 x 32 each) and panel rows (32 x r_pad) on their way from HBM to LDS: 4 x 4 + 4 x 4 + r_pad / 8 registers
// per thread.  Loaded one stage ahead, so the loads are in flight while the MFMAs of the current stage run.
template <int RP>
struct WmuStage {
  float av[4][4], mv[4][4], bv[kWmBK * RP / 256];
};

// av / mv = V / M at (owner row i0 + i, contraction step c0 + c); zero outside the matrix and the part (m = 0: the entry is
// selected away).  16-byte loads along the walk's contiguous axis when `vec`, else scalar loads.
template <int RP, bool TRANS>
__device__ __forceinline__ void wmu_load_vm(WmuStage<RP>& st, const float* __restrict__ V, const float* __restrict__ M,
                                            int64_t ld, int rows, int i0, int c0, int cend, bool vec, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid;
    float* av = st.av[p];
    float* mv = st.mv[p];
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = mv[q] = 0.f;
    // TRANS: V[c0 + cr][i0 + i4 ..], contiguous along i; else V[i0 + row][c0 + c4 ..], contiguous along c
    const int c = c0 + (TRANS ? idx >> 5 : (idx & 7) * 4), i = i0 + (TRANS ? (idx & 31) * 4 : idx >> 3);
    if (c < cend && i < rows) {
      const size_t off = TRANS ? (size_t)c * ld + i : (size_t)i * ld + c;
      const int left = TRANS ? rows - i : cend - c;      // elements of the quad inside the matrix and the part
      if (vec && left >= 4) {
        const float4 v = *reinterpret_cast<const float4*>(V + off), m = *reinterpret_cast<const float4*>(M + off);
        av[0] = v.x, av[1] = v.y, av[2] = v.z, av[3] = v.w;
        mv[0] = m.x, mv[1] = m.y, mv[2] = m.z, mv[3] = m.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < left) av[q] = V[off + q], mv[q] = M[off + q];
      }
    }
  }
}

// sv / sm [i][c], a row stride of 33 floats for either walk
template <int RP, bool TRANS>
__device__ __forceinline__ void wmu_store_vm(float* sv, float* sm, const WmuStage<RP>& st, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int at = TRANS ? ((idx & 31) * 4 + q) * kWmLDA + (idx >> 5) : (idx >> 3) * kWmLDA + (idx & 7) * 4 + q;
      sv[at] = st.av[p][q], sm[at] = st.mv[p][q];
    }
  }
}

// f(std::integral_constant<int, r_pad>)
template <class F>
inline void for_rp(int r_pad, F&& f) {
  switch (r_pad) {
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 128: f(std::integral_constant<int, 128>{}); break;
    default: f(std::integral_constant<int, 256>{}); break;
  }
}

}  // namespace nmfmu
