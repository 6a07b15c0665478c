// The protocol the sparse kernels share (nmfmu_sparse.hip, nmfmu_sparse_autograd.hip, nmfmu_sparse_masked.hip,
// nmfmu_sparse_plca.hip), once:
//
//   a wave per owner row or SEGMENT of one, the lanes across the rank, RL rank slots per lane (slot q of a lane is rank
//   column lane + 64 q; r_pad 32 uses half a wave's lanes with zeros beyond the rank); the stored entries of a segment are
//   read 64 at a time, one per lane, and handed to the wave kSpU at a time; entries accumulate in storage order; a split
//   row's segments store partial rows to ws slots and a finishing kernel adds them in segment order; scalar results are
//   double partials per workgroup, summed in block order by sp_reduce_kernel.  No atomics anywhere: a repeated call is
//   bitwise identical.
//
// Nothing here belongs to one kernel only; what a kernel does with an entry (its g, its loss term, its epilogue) stays
// in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nmfmu.h"

namespace nmfmu {

constexpr int kSpU = 4;   // stored entries in flight per wave and trip: their index / value / panel-row loads are
                          // independent, so kSpU gathers are in flight per wave instead of one

// ---- segments ------------------------------------------------------------------------------------------------------------------
// seg: int32 [n_seg][4] = (owner row, p_begin, p_end, slot) in row order.  slot < 0: the row's only segment; slot >= 0: the
// row is split and this segment's partial row goes to ws slot `slot` (the slots of a row are consecutive, in order).
struct Seg {
  int row, p0, p1, slot;
};

__device__ __forceinline__ Seg load_seg(const int32_t* seg, int sg) {
  // (wave-uniform by construction: one segment per wave)
  return Seg{__builtin_amdgcn_readfirstlane(seg[4 * sg]), __builtin_amdgcn_readfirstlane(seg[4 * sg + 1]),
             __builtin_amdgcn_readfirstlane(seg[4 * sg + 2]), __builtin_amdgcn_readfirstlane(seg[4 * sg + 3])};
}

// a[q] = f[row][lane + 64 q], zero beyond the rank
template <int RL>
__device__ __forceinline__ void load_row(float (&a)[RL], const float* f, int row, int rank, int lane) {
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    a[q] = r < rank ? f[(size_t)row * rank + r] : 0.f;
  }
}

// ---- 64 entries of a segment, one per lane ---------------------------------------------------------------------------------------
// The index is read once per entry (coalesced) and handed to the wave entry by entry with __shfl; what else a kernel keeps
// per entry (value, g, the saved s) it reads at `pe` in the same way.
struct EntryBlock {
  int pe;     // this lane's entry (valid while pe < p1)
  int colv;   // its panel row
  int cnt;    // entries of the block: min(64, p1 - base)
};

__device__ __forceinline__ EntryBlock load_block(const int32_t* idx, int base, int p1, int lane) {
  const int pe = base + lane;
  return EntryBlock{pe, pe < p1 ? idx[pe] : 0, min(64, p1 - base)};
}

// The panel rows of entries j .. j + kSpU - 1 of a block.  An entry past the end of the block (ok[u] false) is not fetched:
// its b is zero whatever the panel holds, so a non-finite panel row 0 cannot reach a row that does not store column 0.
template <int RL>
__device__ __forceinline__ void fetch_group(float (&b)[kSpU][RL], bool (&ok)[kSpU], const EntryBlock& eb, int j,
                                            const float* panel, int rank, int lane) {
#pragma unroll
  for (int u = 0; u < kSpU; ++u) {
    ok[u] = j + u < eb.cnt;
    const int col = ok[u] ? __shfl(eb.colv, (j + u) & 63, 64) : 0;
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      b[u][q] = (ok[u] && r < rank) ? panel[(size_t)col * rank + r] : 0.f;
    }
  }
}

// fn(pe, v, s) once per stored entry of the segment, on the lane that owns the entry: v = vals[pe] and
// s = <a, panel[idx[pe]]> (fixed-order butterfly).  Each lane keeps the dot product of ITS entry of the 64, so whatever fn
// does -- a logarithm, a double sum, the store of s -- runs once per entry instead of once per entry and lane.
template <int RL, class F>
__device__ __forceinline__ void seg_entry_dots(const Seg& sg, const int32_t* idx,
                                               const float* vals, const float (&a)[RL],
                                               const float* panel, int rank, int lane, F&& fn) {
  for (int base = sg.p0; base < sg.p1; base += 64) {
    const EntryBlock eb = load_block(idx, base, sg.p1, lane);
    const float vv = eb.pe < sg.p1 ? vals[eb.pe] : 0.f;
    float sv = 1.f;   // a lane without an entry never hands sv to fn; 1 keeps it finite all the same
    for (int j = 0; j < eb.cnt; j += kSpU) {
      float sdot[kSpU];
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        const bool ok = j + u < eb.cnt;
        const int col = ok ? __shfl(eb.colv, (j + u) & 63, 64) : 0;
        sdot[u] = 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) {
          const int r = lane + 64 * q;
          sdot[u] += (ok && r < rank) ? a[q] * panel[(size_t)col * rank + r] : 0.f;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)     // kSpU fixed-order butterflies, interleaved: kSpU shuffles in flight, not one
#pragma unroll
        for (int u = 0; u < kSpU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
      for (int u = 0; u < kSpU; ++u)
        if (lane == j + u) sv = sdot[u];
    }
    if (eb.pe < sg.p1) fn(eb.pe, vv, sv);
  }
}

// ---- double partials -----------------------------------------------------------------------------------------------------------
// part[blockIdx.x] = the four waves' totals in a fixed order.  `tot` is wave-uniform; every thread of the workgroup calls.
// `red` is the calling kernel's own `__shared__ double red[4]` (a static one in here costs the loss kernels a different
// register allocation).
__device__ __forceinline__ void store_block_total(double tot, double (&red)[4], double* part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the same for per-lane sums: first the lanes of each wave, fixed-order butterfly.  (Not for a `tot` that every lane already
// holds in full: the butterfly would count it 64 times.)
__device__ __forceinline__ void store_lane_totals(double tot, double (&red)[4], double* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  store_block_total(tot, red, part);
}

// *out = (add + the block partials in block order) * mul: one workgroup, strided lanes, tree -- the sum is a pure function
// of n.  (0.0 + x) * 1.0 has the bits of x: every sum here starts from +0.0, so x is never -0.0.  Defined in
// nmfmu_sparse.hip.
__global__ void sp_reduce_kernel(const double* __restrict__ part, int n, double add, double mul, double* __restrict__ out);

// ---- split rows ----------------------------------------------------------------------------------------------------------------
// A split row's segment keeps NP partial rows ("planes": one for the backward, [num | den] for the masked kernels) in its
// slot: ws[(slot * NP + k) * r_pad + r].  Plain stores; every padded rank column is written.
template <int NP, int RL>
__device__ __forceinline__ void store_partial(float* ws, int slot, int k, const float (&acc)[RL], int r_pad, int lane) {
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    if (r < r_pad) ws[(size_t)slot * NP * r_pad + k * r_pad + r] = acc[q];
  }
}

// multi: int32 [n_multi][3] = (owner row, first slot, segments) of the split rows
struct Multi {
  int row, slot0, n;
};

__device__ __forceinline__ Multi load_multi(const int32_t* multi, int m) {
  return Multi{multi[3 * m], multi[3 * m + 1], multi[3 * m + 2]};
}

// acc[k] = rank column r of the row's partials of plane k, added in segment order
template <int NP>
__device__ __forceinline__ void sum_partials(float (&acc)[NP], const float* ws, const Multi& mu, int r,
                                             int r_pad) {
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = ws[(size_t)mu.slot0 * NP * r_pad + k * r_pad + r];
  for (int i = 1; i < mu.n; ++i)
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] += ws[(size_t)(mu.slot0 + i) * NP * r_pad + k * r_pad + r];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// f(std::integral_constant<int, RL>) for the RL of a padded rank: a launch site is a generic lambda that names its kernel
// with decltype(rl)::value
template <class F>
inline void for_rl(int r_pad, F&& f) {
  if (r_pad <= 64) f(std::integral_constant<int, 1>{});
  else if (r_pad == 128) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

// f(std::integral_constant<int, NMFMU_BETA_*>) for a value of nmfmu_beta_kind
template <class F>
inline void for_kind(int kind, F&& f) {
  switch (kind) {
    case NMFMU_BETA_KL: f(std::integral_constant<int, NMFMU_BETA_KL>{}); break;
    case NMFMU_BETA_EUC: f(std::integral_constant<int, NMFMU_BETA_EUC>{}); break;
    case NMFMU_BETA_IS: f(std::integral_constant<int, NMFMU_BETA_IS>{}); break;
    default: f(std::integral_constant<int, NMFMU_BETA_GEN>{}); break;
  }
}

}  // namespace nmfmu
