// Scoring a fitted model without the N x C product (scoring.py).
//
//   score_pairs_kernel   out[p] = <H[rows[p]], W[cols[p]]>: a wave takes 64 pairs, one per lane, and hands them to the wave
//                        kSpU at a time -- the lanes run across the rank (RL slots per lane), fixed-order xor butterfly, every
//                        lane keeps the dot product of ITS pair (the protocol of nmfmu_sparse_common.h's seg_entry_dots, with
//                        both rows changing from pair to pair).
//   topk_partial_kernel  for 64 requested rows and one range of 128-column tiles: S = H_tile W_tile^T by exact-fp32 MFMA
//                        (v_mfma_f32_32x32x2_f32, the staging of reconstruct_kernel: the same k-ordered fmaf chain), the
//                        accumulators go to an LDS score tile, the row's excluded columns inside the tile become -inf, and a
//                        wave per row keeps the row's k best (score, column) in a sorted list in LDS: one ballot of
//                        `score > the list's k-th score` finds the candidates, only those are inserted.
//   topk_merge_kernel    one wave per row: the nsplit partial lists inserted in split order by the same routine.
//
// The order is total -- score descending, equal scores by ascending column -- and a score is a function of its two factor
// rows alone, so the result does not depend on nsplit or on the launch.  No atomics, no fences, plain vector stores.
// A score of -inf (or NaN) is never returned: -inf is what an inadmissible column holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr int kTopRows = 64, kTopCols = 128;   // scoring.TILE_ROWS / TILE_COLS
constexpr int kTopBK = 32, kTopLD = kTopBK + 1;         // rank columns staged per trip; row stride of the staged tiles
constexpr int kTopSLD = kTopCols + 1;                   // row stride of the score tile
constexpr int kTopMaxK = 128, kTopMaxRank = 256;

// ---- pairs -------------------------------------------------------------------------------------------------------------------
template <int RL>
__global__ void __launch_bounds__(256) score_pairs_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                          int64_t n, const float* __restrict__ H, const float* __restrict__ W,
                                                          int rank, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (base >= n) return;
  const int cnt = (int)(n - base < 64 ? n - base : 64);
  const int rowv = lane < cnt ? rows[base + lane] : 0, colv = lane < cnt ? cols[base + lane] : 0;
  float sv = 0.f;
  for (int j = 0; j < cnt; j += kSpU) {
    float sdot[kSpU];
#pragma unroll
    for (int u = 0; u < kSpU; ++u) {
      // a pair past the end reads pair 0's rows (valid addresses) and is dropped below
      const int src = j + u < cnt ? j + u : 0;
      float a[RL], b[RL];
      load_row<RL>(a, H, __shfl(rowv, src, 64), rank, lane);
      load_row<RL>(b, W, __shfl(colv, src, 64), rank, lane);
      sdot[u] = 0.f;
#pragma unroll
      for (int q = 0; q < RL; ++q) sdot[u] += a[q] * b[q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)     // kSpU fixed-order butterflies, interleaved
#pragma unroll
      for (int u = 0; u < kSpU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
    for (int u = 0; u < kSpU; ++u)
      if (lane == j + u) sv = sdot[u];
  }
  if (lane < cnt) out[base + lane] = sv;
}

// ---- the sorted list of a row --------------------------------------------------------------------------------------------------
// Position p of the list is slot p / 64 of lane p % 64; an empty position holds (-inf, -1).
__device__ __forceinline__ bool score_before(float s1, int i1, float s2, int i2) {
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

template <int KL>
struct TopList {
  float s[KL];
  int i[KL];
};

// lane l takes x of lane l - 1, lane 0 takes `in0`: one DPP move (wave_shr:1; a lane without a source lane keeps `old`)
__device__ __forceinline__ int lane_shift_up(int in0, int x) { return __builtin_amdgcn_update_dpp(in0, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float lane_shift_up(float in0, float x) {
  return __int_as_float(lane_shift_up(__float_as_int(in0), __float_as_int(x)));
}

// wave-uniform broadcast of lane b's x (b wave-uniform)
__device__ __forceinline__ int lane_get(int x, int b) { return __builtin_amdgcn_readlane(x, b); }
__device__ __forceinline__ float lane_get(float x, int b) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), b)); }

// lane (k - 1) % 64 of slot (k - 1) / 64, wave-uniform
template <int KL, class T>
__device__ __forceinline__ T list_kth(const T (&x)[KL], int k) {
  T v = x[0];
#pragma unroll
  for (int q = 1; q < KL; ++q)
    if (((k - 1) >> 6) == q) v = x[q];
  return lane_get(v, (k - 1) & 63);
}

// (cs, ci) enters the list when fewer than k entries come before it, that is when it comes before the entry at position
// k - 1.  Every position then keeps its entry if that comes before the candidate, takes the candidate if the entry one
// position up does (position 0: always), and takes that entry otherwise -- a compare, a shift by one lane, a compare.
// ASC: every column of the list is below ci (a scan in ascending column order), so "before" is `score >= cs`.
// Wave-uniform control flow; cs, ci and k are wave-uniform.
template <int KL, bool ASC>
__device__ __forceinline__ void list_insert(TopList<KL>& L, float cs, int ci, int k, int lane) {
  const float ks = list_kth<KL>(L.s, k);
  if (ASC ? !(cs > ks) : !score_before(cs, ci, ks, list_kth<KL>(L.i, k))) return;
  float in_s = __builtin_inff();     // what position 0 sees one position up: an entry before everything
  int in_i = -1;
#pragma unroll
  for (int q = 0; q < KL; ++q) {
    const float ps = lane_shift_up(in_s, L.s[q]);
    const int pi = lane_shift_up(in_i, L.i[q]);
    in_s = lane_get(L.s[q], 63), in_i = lane_get(L.i[q], 63);     // lane 0 of the next slot follows lane 63 of this one
    const bool keep = ASC ? L.s[q] >= cs : score_before(L.s[q], L.i[q], cs, ci);
    const bool here = ASC ? ps >= cs : score_before(ps, pi, cs, ci);
    L.s[q] = keep ? L.s[q] : here ? cs : ps;
    L.i[q] = keep ? L.i[q] : here ? ci : pi;
  }
}

// the candidate lanes of `mask` in ascending order, scores in sc, columns col0 + lane
template <int KL>
__device__ __forceinline__ void list_insert_lanes(TopList<KL>& L, unsigned long long mask, float sc, int col0, int k,
                                                  int lane) {
  while (mask) {
    const int b = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    list_insert<KL, true>(L, lane_get(sc, b), col0 + b, k, lane);
  }
}

// ---- partial lists: 64 rows x one range of column tiles ------------------------------------------------------------------------
// LDS: [score tile 64 x 129 | aliased: H tile 64 x 33, W tile 128 x 33] [list scores 64 x 64 KL] [list columns 64 x 64 KL]
// [row id, exclusion cursor, exclusion end: 3 x 64]
constexpr size_t topk_lds_bytes(int kl) {
  return (size_t)kTopRows * kTopSLD * 4 + (size_t)kTopRows * 64 * kl * 8 + 3 * kTopRows * 4;
}

template <int KL>
__global__ void __launch_bounds__(256) topk_partial_kernel(const float* __restrict__ H, int N,
                                                           const int32_t* __restrict__ row_ids, int n_rows,
                                                           const float* __restrict__ W, int C, int R, int k,
                                                           const int32_t* __restrict__ ex_rowptr,
                                                           const int32_t* __restrict__ ex_colidx, int nsplit,
                                                           float* __restrict__ dst_val, int32_t* __restrict__ dst_idx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = reinterpret_cast<float*>(smem);
  float* sa = sc;                              // the staged tiles live while the MFMA loop runs, the scores after it
  float* sb = sc + kTopRows * kTopLD;
  float* ls = sc + kTopRows * kTopSLD;
  int* li = reinterpret_cast<int*>(ls + kTopRows * 64 * KL);
  int* s_row = li + kTopRows * 64 * KL;
  int* s_cur = s_row + kTopRows;
  int* s_end = s_cur + kTopRows;

  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int rb = blockIdx.x / nsplit, sp = blockIdx.x - rb * nsplit;
  const int n_tiles = (C + kTopCols - 1) / kTopCols;
  const int t0 = (int)((int64_t)sp * n_tiles / nsplit), t1 = (int)((int64_t)(sp + 1) * n_tiles / nsplit);
  const int c_end = min(C, t1 * kTopCols);
  const float ninf = -__builtin_inff();

  // rows of the block, their exclusion ranges (cursor at the split's first column: binary search), empty lists
  if (tid < kTopRows) {
    const int lr = rb * kTopRows + tid;
    int gr = -1, cur = 0, end = 0;
    if (lr < n_rows) {
      gr = row_ids ? row_ids[lr] : lr;
      if (ex_rowptr) {
        int lo = ex_rowptr[gr], hi = ex_rowptr[gr + 1];
        end = hi;
        const int c0 = t0 * kTopCols;
        while (lo < hi) {
          const int mid = lo + ((hi - lo) >> 1);
          if (ex_colidx[mid] < c0) lo = mid + 1;
          else hi = mid;
        }
        cur = lo;
      }
    }
    s_row[tid] = gr, s_cur[tid] = cur, s_end[tid] = end;
  }
  for (int e = tid; e < kTopRows * 64 * KL; e += 256) ls[e] = ninf, li[e] = -1;
  __syncthreads();

  const bool vec = (R & 3) == 0;   // float4 loads need 16-byte aligned rows
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * kTopCols;
    // The next 4 stored columns of each of the wave's 16 rows, one load per wave and tile in flight across the MFMA loop:
    // lane l holds entry l % 4 of row wave + 4 (l / 4).
    const int prow = wave + 4 * (lane >> 2);
    int pre = 0x7fffffff;
    if (ex_rowptr) {
      const int pe = s_cur[prow] + (lane & 3);
      if (pe < s_end[prow]) pre = ex_colidx[pe];
    }
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
    for (int r0 = 0; r0 < R; r0 += kTopBK) {
      // stage H[rows of the block][r0 .. r0+31] (gathered) and W[c0 .. c0+127][r0 .. r0+31], zero fill outside
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        const int idx = (p < 2 ? p : p - 2) * 256 + tid, row = idx >> 3, c4 = (idx & 7) * 4;
        const int r = r0 + c4;
        const int g = p < 2 ? s_row[row] : (c0 + row < C ? c0 + row : -1);
        const float* src = (p < 2 ? H : W) + (size_t)(g < 0 ? 0 : g) * R + r;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (g >= 0 && r < R) {
          if (vec) {
            const float4 x = *reinterpret_cast<const float4*>(src);
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
          } else {
            for (int i = 0; i < 4 && r + i < R; ++i) v[i] = src[i];
          }
        }
        float* dst = (p < 2 ? sa : sb) + row * kTopLD + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = v[i];
      }
      __syncthreads();
      const float* pa = sa + j * kTopLD + hl;
      const float* pb = sb + (wave * 32 + j) * kTopLD + hl;
#pragma unroll
      for (int s2 = 0; s2 < kTopBK; s2 += 2) {
        const float a0 = pa[s2], a1 = pa[32 * kTopLD + s2], b0 = pb[s2];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1], 0, 0, 0);
      }
      __syncthreads();
    }
    // the wave's 64 x 32 scores to the tile (the staged tiles are dead: the barrier above)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        sc[(a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl) * kTopSLD + wave * 32 + j] = acc[a][e];
    __syncthreads();

    // the stored columns of the wave's rows below this tile's end become -inf; the cursors only move forward
    unsigned long long pmask = 0;
    if (ex_rowptr) {
      const bool in = pre < c0 + kTopCols && pre < c_end;
      if (in && pre >= c0) sc[prow * kTopSLD + pre - c0] = ninf;
      pmask = __ballot(in);
      if ((lane & 3) == 0) s_cur[prow] += __popcll((pmask >> lane) & 0xf);
    }

    // a wave per row: rows wave, wave + 4, ...
    for (int ri = 0; ri < kTopRows / 4; ++ri) {
      const int row = wave + 4 * ri;
      if (__builtin_amdgcn_readfirstlane(s_row[row]) < 0) continue;     // (wave-uniform: one row per wave)
      float* srow = sc + row * kTopSLD;
      if (((pmask >> (4 * ri)) & 0xf) == 0xf) {     // all four were inside: the row may store more columns of this tile
        int cur = __builtin_amdgcn_readfirstlane(s_cur[row]);
        const int end = __builtin_amdgcn_readfirstlane(s_end[row]);
        for (;;) {
          const int pe = cur + lane;
          const int col = pe < end ? ex_colidx[pe] : 0x7fffffff;
          const bool in = col < c0 + kTopCols && col < c_end;
          if (in && col >= c0) srow[col - c0] = ninf;
          const int cnt = __popcll(__ballot(in));
          cur += cnt;
          if (cnt < 64) break;
        }
        if (lane == 0) s_cur[row] = cur;
      }
      const float thr = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ls[row * 64 * KL + k - 1])));
      const float x0 = c0 + lane < c_end ? srow[lane] : ninf;
      const float x1 = c0 + 64 + lane < c_end ? srow[64 + lane] : ninf;
      // columns arrive in ascending order: a score equal to the k-th entry's comes behind it
      const unsigned long long m0 = __ballot(x0 > thr), m1 = __ballot(x1 > thr);
      if (m0 | m1) {
        TopList<KL> L;
#pragma unroll
        for (int q = 0; q < KL; ++q) L.s[q] = ls[(row * KL + q) * 64 + lane], L.i[q] = li[(row * KL + q) * 64 + lane];
        list_insert_lanes<KL>(L, m0, x0, c0, k, lane);
        list_insert_lanes<KL>(L, m1, x1, c0 + 64, k, lane);
#pragma unroll
        for (int q = 0; q < KL; ++q) ls[(row * KL + q) * 64 + lane] = L.s[q], li[(row * KL + q) * 64 + lane] = L.i[q];
      }
    }
    __syncthreads();     // the score tile is staged over next
  }

  // the k entries of every (row, split); empty positions are already (-inf, -1)
  for (int row = wave; row < kTopRows; row += 4) {
    const int lr = rb * kTopRows + row;
    if (lr >= n_rows) continue;
    const size_t o = ((size_t)lr * nsplit + sp) * k;
#pragma unroll
    for (int q = 0; q < KL; ++q) {
      const int p = lane + 64 * q;
      if (p < k) dst_val[o + p] = ls[(row * KL + q) * 64 + lane], dst_idx[o + p] = li[(row * KL + q) * 64 + lane];
    }
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------
template <int KL>
__global__ void __launch_bounds__(256) topk_merge_kernel(const float* __restrict__ ws_val, const int32_t* __restrict__ ws_idx,
                                                         int n_rows, int k, int nsplit, float* __restrict__ out_val,
                                                         int32_t* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  TopList<KL> L;
#pragma unroll
  for (int q = 0; q < KL; ++q) L.s[q] = -__builtin_inff(), L.i[q] = -1;
  for (int sp = 0; sp < nsplit; ++sp) {
    const size_t o = ((size_t)row * nsplit + sp) * k;
    for (int base = 0; base < k; base += 64) {
      const int p = base + lane;
      const float v = p < k ? ws_val[o + p] : 0.f;
      const int c = p < k ? ws_idx[o + p] : -1;
      // (padding entries carry column -1)
      for (unsigned long long mask = __ballot(c >= 0); mask;) {
        const int b = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        list_insert<KL, false>(L, lane_get(v, b), lane_get(c, b), k, lane);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KL; ++q) {
    const int p = lane + 64 * q;
    if (p < k) out_val[(size_t)row * k + p] = L.s[q], out_idx[(size_t)row * k + p] = L.i[q];
  }
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_score_pairs(const int32_t* rows, const int32_t* cols, int64_t n, const float* H, int N, const float* W, int C,
                      int rank, float* out, void* stream) {
  if (!rows || !cols || !H || !W || !out || n < 0 || N <= 0 || C <= 0 || rank <= 0) return NMFMU_ERR_ARG;
  if (rank > kTopMaxRank || n > ((int64_t)1 << 38)) return NMFMU_ERR_UNSUPPORTED;
  if (n == 0) return NMFMU_OK;
  const int nblk = (int)((n + 255) / 256);
  for_rl(nmfmu_pad_rank(rank), [&](auto rl) {
    hipLaunchKernelGGL((score_pairs_kernel<decltype(rl)::value>), dim3(nblk), dim3(256), 0, S(stream), rows, cols, n, H, W,
                       rank, out);
  });
  return (int)hipGetLastError();
}

int64_t nmfmu_topk_ws(int n_rows, int k, int nsplit) {
  if (n_rows <= 0 || k < 1 || nsplit <= 1) return 0;
  return (int64_t)n_rows * nsplit * k * 8;     // [n_rows][nsplit][k] floats, then as many int32
}

int nmfmu_topk(const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C, int rank, int k,
               const int32_t* ex_rowptr, const int32_t* ex_colidx, int nsplit, void* ws, float* out_val, int32_t* out_idx,
               void* stream) {
  if (!H || !W || !out_val || !out_idx || N <= 0 || C <= 0 || n_rows <= 0 || rank <= 0 || k < 1 || nsplit < 1)
    return NMFMU_ERR_ARG;
  if (ex_rowptr && !ex_colidx) return NMFMU_ERR_ARG;
  if (nsplit > 1 && !ws) return NMFMU_ERR_ARG;
  if (rank > kTopMaxRank || k > kTopMaxK) return NMFMU_ERR_UNSUPPORTED;
  const int64_t blocks = (int64_t)((n_rows + kTopRows - 1) / kTopRows) * nsplit;
  if (blocks >= ((int64_t)1 << 31)) return NMFMU_ERR_UNSUPPORTED;
  float* pv = nsplit > 1 ? static_cast<float*>(ws) : out_val;
  int32_t* pi = nsplit > 1 ? reinterpret_cast<int32_t*>(pv + (size_t)n_rows * nsplit * k) : out_idx;
  int rc = 0;
  auto go = [&](auto kl) {
    constexpr int KL = decltype(kl)::value;
    constexpr size_t lds = topk_lds_bytes(KL);
    auto kern = topk_partial_kernel<KL>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);     // above 64 KiB
    if (e != hipSuccess) {
      rc = (int)e;
      return;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, S(stream), H, N, row_ids, n_rows, W, C, rank, k,
                       ex_rowptr, ex_colidx, nsplit, pv, pi);
    if (nsplit > 1)
      hipLaunchKernelGGL(topk_merge_kernel<KL>, dim3((n_rows + 3) / 4), dim3(256), 0, S(stream), pv, pi, n_rows, k, nsplit,
                         out_val, out_idx);
  };
  if (k <= 64) go(std::integral_constant<int, 1>{});
  else go(std::integral_constant<int, 2>{});
  return rc ? rc : (int)hipGetLastError();
}

}  // extern "C"
