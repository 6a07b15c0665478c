// Full-ranking evaluation of a fitted model without the n_rows x C score matrix (scoring.py).
//
// For every held-out pair e = (i, c): the score s_ic and the number of admissible columns of row i that come before c in
// topk's total order (score descending, equal scores by ascending column).  The score tile is topk_partial_kernel's
// (nmfmu_score.hip), restated here so that topk's code stays as it is: 64 requested rows x one of nsplit ranges of whole
// 128-column tiles, v_mfma_f32_32x32x2_f32 on operands staged 32 rank columns per trip -- the same k-ordered fmaf chain, so a
// score has topk's bits.  A count needs its thresholds first, hence two passes over the tiles:
//
//   rank_tile_kernel<0>  extract: a forward-only cursor per row over the held-out CSR (binary search at the split's first
//                        column) copies tile[i][c] to out_score[e]; nothing is masked in this pass.  A pair that the exclusion
//                        pattern also stores (binary search in the row's stored columns) gets the flag -1 in out_rank[e], every
//                        other pair 0.
//   rank_tile_kernel<1>  count: the stored columns inside the tile become -inf (topk's exclusion cursor), then a wave per row
//                        counts the tile's scores that come before each of the row's thresholds (s_e, c_e).  The first 64
//                        thresholds of a row and their counts stay in the registers of the row's wave for the whole column
//                        range (lane l: threshold l); further chunks of 64 go through ws with plain loads and stores from the
//                        same lanes.  Two forms of the count, chosen per row:
//                          ballot : per threshold two ballots + one popcount per 64 columns (work ~ thresholds)
//                          scan   : every lane walks the 128 scores of the row in LDS (broadcast reads) against its OWN
//                                   threshold (work ~ 128 whatever the number of thresholds; rows above kRkScanAbove)
//   rank_merge_kernel    a wave per row adds the nsplit partial counts of every pair, keeps -1 on flagged pairs, and writes
//                        out_admissible = C - stored columns of the row.
//
// Counts are integers: the sum over tiles and splits is exact, so a rank does not depend on nsplit, on the form or on the
// launch.  No atomics, no fences, plain vector stores.  -inf marks an inadmissible column as in topk: factors are taken to be
// finite.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr int kRkRows = 64, kRkCols = 128;            // scoring.TILE_ROWS / TILE_COLS
constexpr int kRkBK = 32, kRkLD = kRkBK + 1;          // rank columns staged per trip; row stride of the staged tiles
constexpr int kRkSLD = kRkCols + 1;                   // row stride of the score tile
constexpr int kRkMaxRank = 256;
constexpr int kRkScanAbove = 24;                      // scoring.RANK_SCAN_ABOVE: rows with more held-out pairs use the scan form
constexpr int kRkRowsPerWave = kRkRows / 4;
constexpr int kRkNone = 0x7fffffff;

__device__ __forceinline__ bool rk_before(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }
__device__ __forceinline__ int rk_lane_get(int x, int b) { return __builtin_amdgcn_readlane(x, b); }
__device__ __forceinline__ float rk_lane_get(float x, int b) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), b));
}

// first position in colidx[lo, hi) that holds a column >= c
__device__ __forceinline__ int rk_lower_bound(const int32_t* __restrict__ colidx, int lo, int hi, int c) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (colidx[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The scores of one row of the tile that come before each of up to 64 thresholds; lane l answers for threshold l (sv, cv).
// x0 / x1: the row's scores at columns c0 + lane / c0 + 64 + lane (-inf past the split's end); srow: the same row in LDS,
// ncols of it inside the split.  nthr and scan are wave-uniform.  A lane without a threshold holds (+inf, -1): nothing comes
// before it.
__device__ __forceinline__ int rk_count(float sv, int cv, int nthr, bool scan, float x0, float x1, const float* srow, int c0,
                                        int ncols, int lane) {
  int acc = 0;
  if (scan) {
    for (int c = 0; c < ncols; ++c) acc += rk_before(srow[c], c0 + c, sv, cv) ? 1 : 0;
  } else {
    for (int u = 0; u < nthr; ++u) {
      const float se = rk_lane_get(sv, u);
      const int ce = rk_lane_get(cv, u);
      // column c0 + lane comes before (se, ce) when its score is greater, or equal with c0 + lane < ce: the lanes below
      // ce - c0 are a wave-uniform mask, so the tie rule is two scalar ops on the ballots
      const int d = ce - c0;
      const unsigned long long lt0 = d <= 0 ? 0ull : d >= 64 ? ~0ull : (1ull << d) - 1;
      const unsigned long long lt1 = d <= 64 ? 0ull : d >= 128 ? ~0ull : (1ull << (d - 64)) - 1;
      const int cnt = __popcll(__ballot(x0 > se) | (__ballot(x0 >= se) & lt0)) +
                      __popcll(__ballot(x1 > se) | (__ballot(x1 >= se) & lt1));
      acc = lane == u ? cnt : acc;
    }
  }
  return acc;
}

// LDS: [score tile 64 x 129 | aliased: H tile 64 x 33, W tile 128 x 33] [row id, cursor, cursor end, held-out begin, end: 5 x 64]
// PASS 0: the cursor runs over the held-out CSR; PASS 1: over the exclusion CSR.
template <int PASS>
__global__ void __launch_bounds__(256) rank_tile_kernel(const float* __restrict__ H, const int32_t* __restrict__ row_ids,
                                                        int n_rows, const float* __restrict__ W, int C, int R,
                                                        const int32_t* __restrict__ ho_rowptr,
                                                        const int32_t* __restrict__ ho_colidx,
                                                        const int32_t* __restrict__ ex_rowptr,
                                                        const int32_t* __restrict__ ex_colidx, int nsplit, int scan_above,
                                                        int32_t* __restrict__ ws, float* __restrict__ out_score,
                                                        int32_t* __restrict__ out_rank) {
  __shared__ __attribute__((aligned(16))) float sc[kRkRows * kRkSLD];
  __shared__ int s_row[kRkRows], s_cur[kRkRows], s_end[kRkRows], s_hb[kRkRows], s_he[kRkRows];
  float* sa = sc;                              // the staged tiles live while the MFMA loop runs, the scores after it
  float* sb = sc + kRkRows * kRkLD;

  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int rb = blockIdx.x / nsplit, sp = blockIdx.x - rb * nsplit;
  const int n_tiles = (C + kRkCols - 1) / kRkCols;
  const int t0 = (int)((int64_t)sp * n_tiles / nsplit), t1 = (int)((int64_t)(sp + 1) * n_tiles / nsplit);
  const int c_end = min(C, t1 * kRkCols);
  const float ninf = -__builtin_inff();
  int32_t* __restrict__ ws_sp = ws + (size_t)sp * (size_t)ho_rowptr[n_rows];     // the split's slice [n_pairs] of ws
  const bool use_cursor = PASS == 0 || ex_rowptr != nullptr;
  const int32_t* __restrict__ cur_colidx = PASS == 0 ? ho_colidx : ex_colidx;

  // rows of the block, their held-out ranges, the cursor at the split's first column (binary search)
  if (tid < kRkRows) {
    const int lr = rb * kRkRows + tid;
    int gr = -1, cur = 0, end = 0, hb = 0, he = 0;
    if (lr < n_rows) {
      gr = row_ids ? row_ids[lr] : lr;
      hb = ho_rowptr[lr], he = ho_rowptr[lr + 1];
      if (PASS == 0) {
        end = he;
        cur = rk_lower_bound(ho_colidx, hb, he, t0 * kRkCols);
      } else if (ex_rowptr) {
        end = ex_rowptr[gr + 1];
        cur = rk_lower_bound(ex_colidx, ex_rowptr[gr], end, t0 * kRkCols);
      }
    }
    s_row[tid] = gr, s_cur[tid] = cur, s_end[tid] = end, s_hb[tid] = hb, s_he[tid] = he;
  }
  __syncthreads();

  // PASS 1: the first 64 thresholds of each of the wave's 16 rows and their counts, in registers for the whole column range
  float thr_s[kRkRowsPerWave];
  int thr_c[kRkRowsPerWave], thr_n[kRkRowsPerWave];
  if (PASS == 1) {
#pragma unroll
    for (int ri = 0; ri < kRkRowsPerWave; ++ri) {
      const int row = wave + 4 * ri;
      const int hb = s_hb[row], t = s_he[row] - hb;
      const bool has = lane < t;
      thr_s[ri] = has ? out_score[hb + lane] : __builtin_inff();
      thr_c[ri] = has ? ho_colidx[hb + lane] : -1;
      thr_n[ri] = 0;
    }
  }

  const bool vec = (R & 3) == 0;   // float4 loads need 16-byte aligned rows
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * kRkCols;
    // The next 4 cursor entries of each of the wave's 16 rows, one load per wave and tile in flight across the MFMA loop:
    // lane l holds entry l % 4 of row wave + 4 (l / 4).
    const int prow = wave + 4 * (lane >> 2);
    int pre = kRkNone, ppe = 0;
    if (use_cursor) {
      ppe = s_cur[prow] + (lane & 3);
      if (ppe < s_end[prow]) pre = cur_colidx[ppe];
    }
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
    for (int r0 = 0; r0 < R; r0 += kRkBK) {
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
        float* dst = (p < 2 ? sa : sb) + row * kRkLD + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = v[i];
      }
      __syncthreads();
      const float* pa = sa + j * kRkLD + hl;
      const float* pb = sb + (wave * 32 + j) * kRkLD + hl;
#pragma unroll
      for (int s2 = 0; s2 < kRkBK; s2 += 2) {
        const float a0 = pa[s2], a1 = pa[32 * kRkLD + s2], b0 = pb[s2];
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
        sc[(a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl) * kRkSLD + wave * 32 + j] = acc[a][e];
    __syncthreads();

    // What a cursor entry inside the tile does.  PASS 0: the pair's score leaves the tile, and its flag is set.
    // PASS 1: the stored column becomes -inf.
    auto visit = [&](int row, int pe, int col) {
      if (PASS == 0) {
        out_score[pe] = sc[row * kRkSLD + col - c0];
        int flag = 0;
        if (ex_rowptr) {
          const int gr = s_row[row], end = ex_rowptr[gr + 1];
          const int lo = rk_lower_bound(ex_colidx, ex_rowptr[gr], end, col);
          if (lo < end && ex_colidx[lo] == col) flag = -1;
        }
        out_rank[pe] = flag;
      } else {
        sc[row * kRkSLD + col - c0] = ninf;
      }
    };

    // the prefetched entries below this tile's end; the cursors only move forward
    unsigned long long pmask = 0;
    if (use_cursor) {
      const bool in = pre < c0 + kRkCols && pre < c_end;
      if (in && pre >= c0) visit(prow, ppe, pre);
      pmask = __ballot(in);
      if ((lane & 3) == 0) s_cur[prow] += __popcll((pmask >> lane) & 0xf);
    }

    // a wave per row: rows wave, wave + 4, ...
#pragma unroll
    for (int ri = 0; ri < kRkRowsPerWave; ++ri) {
      const int row = wave + 4 * ri;
      if (__builtin_amdgcn_readfirstlane(s_row[row]) < 0) continue;     // (wave-uniform: one row per wave)
      if (((pmask >> (4 * ri)) & 0xf) == 0xf) {     // all four were inside: the row may have more entries in this tile
        int cur = __builtin_amdgcn_readfirstlane(s_cur[row]);
        const int end = __builtin_amdgcn_readfirstlane(s_end[row]);
        for (;;) {
          const int pe = cur + lane;
          const int col = pe < end ? cur_colidx[pe] : kRkNone;
          const bool in = col < c0 + kRkCols && col < c_end;
          if (in && col >= c0) visit(row, pe, col);
          const int cnt = __popcll(__ballot(in));
          cur += cnt;
          if (cnt < 64) break;
        }
        if (lane == 0) s_cur[row] = cur;
      }
      if (PASS == 1) {
        const int hb = __builtin_amdgcn_readfirstlane(s_hb[row]);
        const int nt = __builtin_amdgcn_readfirstlane(s_he[row]) - hb;
        if (nt <= 0) continue;
        const float* srow = sc + row * kRkSLD;
        const float x0 = c0 + lane < c_end ? srow[lane] : ninf;
        const float x1 = c0 + 64 + lane < c_end ? srow[64 + lane] : ninf;
        const int ncols = min(kRkCols, c_end - c0);
        const bool scan = nt > scan_above;
        thr_n[ri] += rk_count(thr_s[ri], thr_c[ri], min(nt, 64), scan, x0, x1, srow, c0, ncols, lane);
        // thresholds 64 and up: chunks of 64 through ws, the same lane adds to the same word tile after tile
        for (int base = 64; base < nt; base += 64) {
          const int e = hb + base + lane;
          const bool has = base + lane < nt;
          const float sv = has ? out_score[e] : __builtin_inff();
          const int cv = has ? ho_colidx[e] : -1;
          const int add = rk_count(sv, cv, min(nt - base, 64), scan, x0, x1, srow, c0, ncols, lane);
          if (has) {
            int32_t* dst = ws_sp + e;
            *dst = t == t0 ? add : *dst + add;
          }
        }
      }
    }
    __syncthreads();     // the score tile is staged over next
  }

  // the counts of the first 64 thresholds of every (row, split)
  if (PASS == 1) {
#pragma unroll
    for (int ri = 0; ri < kRkRowsPerWave; ++ri) {
      const int row = wave + 4 * ri;
      const int hb = s_hb[row], nt = s_he[row] - hb;
      if (lane < nt) ws_sp[hb + lane] = thr_n[ri];
      if (t0 == t1)     // a split without a tile (nsplit above the number of tiles) still owns its slice
        for (int e = 64 + lane; e < nt; e += 64) ws_sp[hb + e] = 0;
    }
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rank_merge_kernel(const int32_t* __restrict__ row_ids, int n_rows, int C,
                                                         const int32_t* __restrict__ ho_rowptr,
                                                         const int32_t* __restrict__ ex_rowptr, int nsplit,
                                                         const int32_t* __restrict__ ws, int32_t* __restrict__ out_rank,
                                                         int32_t* __restrict__ out_admissible) {
  const int lane = threadIdx.x & 63;
  const int lr = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lr >= n_rows) return;
  const size_t n_pairs = (size_t)ho_rowptr[n_rows];
  const int gr = row_ids ? row_ids[lr] : lr;
  if (lane == 0) out_admissible[lr] = C - (ex_rowptr ? ex_rowptr[gr + 1] - ex_rowptr[gr] : 0);
  const int he = ho_rowptr[lr + 1];
  for (int e = ho_rowptr[lr] + lane; e < he; e += 64) {
    if (out_rank[e] == -1) continue;     // the extract pass's flag: the pair is stored in the exclusion pattern
    int sum = 0;
    for (int sp = 0; sp < nsplit; ++sp) sum += ws[(size_t)sp * n_pairs + e];
    out_rank[e] = sum;
  }
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int64_t nmfmu_rank_ws(int64_t n_pairs, int n_rows, int nsplit) {
  if (n_pairs <= 0 || n_rows <= 0 || nsplit < 1) return 0;
  return n_pairs * nsplit * 4;     // [nsplit][n_pairs] int32 partial counts
}

int nmfmu_rank_pass(int pass, int form, const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C,
                    int rank, const int32_t* ho_rowptr, const int32_t* ho_colidx, const int32_t* ex_rowptr,
                    const int32_t* ex_colidx, int nsplit, void* ws, float* out_score, int32_t* out_rank,
                    int32_t* out_admissible, void* stream) {
  if (!H || !W || !ho_rowptr || !ho_colidx || !ws || !out_score || !out_rank || !out_admissible || N <= 0 || C <= 0 ||
      n_rows <= 0 || rank <= 0 || nsplit < 1 || pass < 0 || pass > 2 || form < 0)
    return NMFMU_ERR_ARG;
  if (ex_rowptr && !ex_colidx) return NMFMU_ERR_ARG;
  if (rank > kRkMaxRank) return NMFMU_ERR_UNSUPPORTED;
  const int64_t blocks = (int64_t)((n_rows + kRkRows - 1) / kRkRows) * nsplit;
  if (blocks >= ((int64_t)1 << 31)) return NMFMU_ERR_UNSUPPORTED;
  int32_t* wsi = static_cast<int32_t*>(ws);
  // rows with more held-out pairs than this scan (form > 2: the threshold itself, for measuring where the forms cross)
  const int scan_above = form == 1 ? kRkNone : form == 2 ? 0 : form > 2 ? form : kRkScanAbove;
  if (pass == 0)
    hipLaunchKernelGGL(rank_tile_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, S(stream), H, row_ids, n_rows, W, C, rank,
                       ho_rowptr, ho_colidx, ex_rowptr, ex_colidx, nsplit, scan_above, wsi, out_score, out_rank);
  else if (pass == 1)
    hipLaunchKernelGGL(rank_tile_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, S(stream), H, row_ids, n_rows, W, C, rank,
                       ho_rowptr, ho_colidx, ex_rowptr, ex_colidx, nsplit, scan_above, wsi, out_score, out_rank);
  else
    hipLaunchKernelGGL(rank_merge_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, S(stream), row_ids, n_rows, C, ho_rowptr,
                       ex_rowptr, nsplit, wsi, out_rank, out_admissible);
  return (int)hipGetLastError();
}

int nmfmu_rank_pairs(const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C, int rank,
                     const int32_t* ho_rowptr, const int32_t* ho_colidx, const int32_t* ex_rowptr, const int32_t* ex_colidx,
                     int nsplit, void* ws, float* out_score, int32_t* out_rank, int32_t* out_admissible, void* stream) {
  for (int pass = 0; pass < 3; ++pass) {
    const int rc = nmfmu_rank_pass(pass, 0, H, N, row_ids, n_rows, W, C, rank, ho_rowptr, ho_colidx, ex_rowptr, ex_colidx,
                                   nsplit, ws, out_score, out_rank, out_admissible, stream);
    if (rc) return rc;
  }
  return NMFMU_OK;
}

}  // extern "C"
