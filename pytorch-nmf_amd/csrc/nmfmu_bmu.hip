// Batched NMF: `batch` independent problems of one shape per launch, V_b (n x c) ~ H_b W_b^T, every problem stopped on its
// own.  The batched, unweighted sibling of nmfmu_wmu.hip, built from the same tile pieces (nmfmu_wmu_tile.h): a workgroup
// (4 waves) owns 128 owner rows x a rank tile of <= 128 x one part of the contraction axis of ONE problem, keeps its owner rows
// in registers, forms Y per 32-step stage by exact-fp32 MFMA over the full padded rank (v_mfma_f32_32x32x2_f32, bitwise a
// k-ordered fmaf chain), turns Y and V into the two seeds of nmf.py:61-74 in LDS (masked_g<KIND>) and accumulates both
// contractions in registers.  V is walked along its rows (H side) or its columns (W side) in place; Y and the seeds never
// reach HBM.  An entry outside the matrix or the part is SELECTED away (its seeds are stored as 0), so nothing the padding
// computes (1 / eps, eps^(beta - 2)) meets a zero panel row in an MFMA.
//
// The problem index is the slow part of grid.x (block = problem * row tiles + row tile; rank tiles on y, parts on z): the
// 65 535 limit of y / z never sees the batch.  A batch whose grid.x would pass 2^31 - 1 is refused (NMFMU_ERR_UNSUPPORTED).
//
// The contraction is cut into parts by the rule of nmfmu_wmu.hip -- a pure function of (rows, contraction, r_pad): the batch
// does not enter, so a problem's bits do not depend on how many others are fitted alongside it.  Every part stores its two
// planes to the slab [problem][part][num | den][rows][r_pad] with plain stores; bmu_finish_kernel adds them in part order and
// stores the planes (terms) or applies nmf.py:78-92 to the owner's fp32 master (step).  No atomics, no fences: a repeated
// call is bitwise identical whatever the workspace held.
//
// Every kernel starts with `if (active && !active[problem]) return;`, uniform for the workgroup and before its first barrier:
// a stopped problem costs one load per workgroup; neither its factors nor its slab nor its loss are touched.  Iteration count
// and stopping live in the host loop and bmu_judge_kernel; no kernel here loops on data.
//
// The weighted entries (nmfmu_bwmu_*) give every problem dense weights M_s (n x c, V's row stride), s = m_index[problem] or
// the problem itself, at Mb + s * mstride (mstride 0: one matrix for all): bwmu_kernel is bmu_kernel with the weighted stage
// of nmfmu_wmu.hip (WmuStage: V and M travel together, both seeds are multiplied by m, an entry with m == 0 is selected
// away), per problem the arithmetic of wmu_kernel in its order -- bitwise nmfmu_wmu_terms / _step on (V_b, M_b).  With
// M == NULL they launch the unweighted kernels above.  `reg` ([batch][2], per-problem (l1, l2)) replaces the scalars of
// the apply for either, in a finish kernel of its own (bmu_finish_reg_kernel): without it every kernel launched is the
// unweighted batch's own.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

// A stage's V (128 x 32) and panel rows (32 x r_pad) on their way from HBM to LDS: 4 x 4 + r_pad / 8 registers per thread,
// loaded one stage ahead.
template <int RP>
struct BmuStage {
  float av[4][4], bv[kWmBK * RP / 256];
};

// av = V at (owner row i0 + i, contraction step c0 + c); zero outside the matrix and the part.  16-byte loads along the
// walk's contiguous axis when `vec`, else scalar loads.
template <int RP, bool TRANS>
__device__ __forceinline__ void bmu_load_v(BmuStage<RP>& st, const float* __restrict__ V, int64_t ld, int rows, int i0, int c0,
                                           int cend, bool vec, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid;
    float* av = st.av[p];
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = 0.f;
    // TRANS: V[c0 + cr][i0 + i4 ..], contiguous along i; else V[i0 + row][c0 + c4 ..], contiguous along c
    const int c = c0 + (TRANS ? idx >> 5 : (idx & 7) * 4), i = i0 + (TRANS ? (idx & 31) * 4 : idx >> 3);
    if (c < cend && i < rows) {
      const size_t off = TRANS ? (size_t)c * ld + i : (size_t)i * ld + c;
      const int left = TRANS ? rows - i : cend - c;      // elements of the quad inside the matrix and the part
      if (vec && left >= 4) {
        const float4 v = *reinterpret_cast<const float4*>(V + off);
        av[0] = v.x, av[1] = v.y, av[2] = v.z, av[3] = v.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < left) av[q] = V[off + q];
      }
    }
  }
}

// sv [i][c], a row stride of 33 floats for either walk
template <int RP, bool TRANS>
__device__ __forceinline__ void bmu_store_v(float* sv, const BmuStage<RP>& st, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int at = TRANS ? ((idx & 31) * 4 + q) * kWmLDA + (idx >> 5) : (idx >> 3) * kWmLDA + (idx & 7) * 4 + q;
      sv[at] = st.av[p][q];
    }
  }
}

__device__ __forceinline__ bool bmu_vec(const float* V, int64_t vstride, int64_t ld) {
  return ((ld | vstride) & 3) == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0;
}

// grid = (problems x row tiles, rank tiles, parts).  on / od + problem * bstride + part * pstride: the part's planes [rows][RP].
template <int RP, bool TRANS, int KIND>
__global__ void __launch_bounds__(256) bmu_kernel(const float* __restrict__ Vb, int64_t vstride, int64_t ld, int rows, int C,
                                                  const float* __restrict__ owner_b, const float* __restrict__ panel_b,
                                                  int rank, float beta, int part_len, int row_tiles,
                                                  const int32_t* __restrict__ active, float* __restrict__ on,
                                                  float* __restrict__ od, int64_t pstride, int64_t bstride) {
  using K = WmuCfg<RP>;
  const int prob = blockIdx.x / row_tiles;
  if (active && !active[prob]) return;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];      // V, then g_neg
  __shared__ __attribute__((aligned(16))) float sg[kWmRows * kWmLDA];      // g_pos
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  const float* V = Vb + (size_t)prob * vstride;
  const float* owner = owner_b + (size_t)prob * rows * rank;
  const float* panel = panel_b + (size_t)prob * C * rank;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave / K::WN, wn = wave % K::WN;
  const int i0 = (blockIdx.x - prob * row_tiles) * kWmRows, r0 = blockIdx.y * K::RT;
  const int cbeg = blockIdx.z * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  f32x16 accn[K::TM][K::TN], accd[K::TM][K::TN];
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) accn[t][b][e] = accd[t][b][e] = 0.f;
  const bool vec = bmu_vec(Vb, vstride, ld);
  BmuStage<RP> st;
  bmu_load_v<RP, TRANS>(st, V, ld, rows, i0, cbeg, cend, vec, tid);
  wmu_load_panel<RP>(st, panel, rank, cbeg, cend, tid);
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    bmu_store_v<RP, TRANS>(sv, st, tid);
    wmu_store_panel<RP>(sb, st, tid);
    __syncthreads();
    if (c0 + kWmBK < cend) {      // the next stage's loads travel behind this stage's MFMAs
      bmu_load_v<RP, TRANS>(st, V, ld, rows, i0, c0 + kWmBK, cend, vec, tid);
      wmu_load_panel<RP>(st, panel, rank, c0 + kWmBK, cend, tid);
    }
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
    // g_neg over V, g_pos beside it: every element belongs to one lane of the wave that owns its row
    const bool col_ok = c0 + j < cend;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wave * 32 + wmu_tile_row(e, hl);
      const int at = row * kWmLDA + j;
      float gn, gp;
      masked_g<KIND>(sv[at], y[e], beta, gn, gp);
      const bool ok = col_ok && i0 + row < rows;
      sv[at] = ok ? gn : 0.f;
      sg[at] = ok ? gp : 0.f;
    }
    __syncthreads();
    const float* pn = sv + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pd = sg + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pb = sb + hl * K::LDB + r0 + wn * K::TN * 32 + j;
#pragma unroll
    for (int s2 = 0; s2 < kWmBK; s2 += 2) {
      float bb[K::TN];
#pragma unroll
      for (int b = 0; b < K::TN; ++b) bb[b] = pb[s2 * K::LDB + b * 32];
#pragma unroll
      for (int t = 0; t < K::TM; ++t) {
        const float gn = pn[t * 32 * kWmLDA + s2], gp = pd[t * 32 * kWmLDA + s2];
#pragma unroll
        for (int b = 0; b < K::TN; ++b) {
          accn[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gn, bb[b], accn[t][b], 0, 0, 0);
          accd[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp, bb[b], accd[t][b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  float* pn = on + (size_t)prob * bstride + (size_t)blockIdx.z * pstride;
  float* pd = od + (size_t)prob * bstride + (size_t)blockIdx.z * pstride;
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b) {
      const int r = r0 + wn * K::TN * 32 + b * 32 + j;      // < RP: the rank tiles cover the padded rank exactly
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + wm * K::TM * 32 + t * 32 + wmu_tile_row(e, hl);
        if (i < rows) {
          pn[(size_t)i * RP + r] = r < rank ? accn[t][b][e] : 0.f;
          pd[(size_t)i * RP + r] = r < rank ? accd[t][b][e] : 0.f;
        }
      }
    }
}

__device__ __forceinline__ bool bwmu_vec(const float* V, int64_t vstride, const float* M, int64_t mstride, int64_t ld) {
  return ((ld | vstride | mstride) & 3) == 0 &&
         ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(M)) & 15) == 0;
}

// the problem's weights: slice m_index[prob] (or prob) of Mb
__device__ __forceinline__ const float* bwmu_weights(const float* Mb, int64_t mstride, const int32_t* m_index, int prob) {
  return Mb + (size_t)(m_index ? m_index[prob] : prob) * mstride;
}

// bmu_kernel's grid and planes, wmu_kernel's stage and seeds: m = 0 outside the matrix and the part, so one selection covers
// the weightless entries and the padding.
template <int RP, bool TRANS, int KIND>
__global__ void __launch_bounds__(256) bwmu_kernel(const float* __restrict__ Vb, int64_t vstride, const float* __restrict__ Mb,
                                                   int64_t mstride, const int32_t* __restrict__ m_index, int64_t ld, int rows,
                                                   int C, const float* __restrict__ owner_b, const float* __restrict__ panel_b,
                                                   int rank, float beta, int part_len, int row_tiles,
                                                   const int32_t* __restrict__ active, float* __restrict__ on,
                                                   float* __restrict__ od, int64_t pstride, int64_t bstride) {
  using K = WmuCfg<RP>;
  const int prob = blockIdx.x / row_tiles;
  if (active && !active[prob]) return;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];      // V, then m g_neg
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];      // M, then m g_pos
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  const float* V = Vb + (size_t)prob * vstride;
  const float* M = bwmu_weights(Mb, mstride, m_index, prob);
  const float* owner = owner_b + (size_t)prob * rows * rank;
  const float* panel = panel_b + (size_t)prob * C * rank;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave / K::WN, wn = wave % K::WN;
  const int i0 = (blockIdx.x - prob * row_tiles) * kWmRows, r0 = blockIdx.y * K::RT;
  const int cbeg = blockIdx.z * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  f32x16 accn[K::TM][K::TN], accd[K::TM][K::TN];
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) accn[t][b][e] = accd[t][b][e] = 0.f;
  const bool vec = bwmu_vec(Vb, vstride, Mb, mstride, ld);
  WmuStage<RP> st;
  wmu_load_vm<RP, TRANS>(st, V, M, ld, rows, i0, cbeg, cend, vec, tid);
  wmu_load_panel<RP>(st, panel, rank, cbeg, cend, tid);
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    wmu_store_vm<RP, TRANS>(sv, sm, st, tid);
    wmu_store_panel<RP>(sb, st, tid);
    __syncthreads();
    if (c0 + kWmBK < cend) {      // the next stage's loads travel behind this stage's MFMAs
      wmu_load_vm<RP, TRANS>(st, V, M, ld, rows, i0, c0 + kWmBK, cend, vec, tid);
      wmu_load_panel<RP>(st, panel, rank, c0 + kWmBK, cend, tid);
    }
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
    // m g_neg over V, m g_pos over M: every element belongs to one lane of the wave that owns its row
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int at = (wave * 32 + wmu_tile_row(e, hl)) * kWmLDA + j;
      const float v = sv[at], m = sm[at];
      float gn, gp;
      masked_g<KIND>(v, y[e], beta, gn, gp);
      const bool w = m > 0.f;
      sv[at] = w ? m * gn : 0.f;
      sm[at] = w ? m * gp : 0.f;
    }
    __syncthreads();
    const float* pn = sv + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pd = sm + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pb = sb + hl * K::LDB + r0 + wn * K::TN * 32 + j;
#pragma unroll
    for (int s2 = 0; s2 < kWmBK; s2 += 2) {
      float bb[K::TN];
#pragma unroll
      for (int b = 0; b < K::TN; ++b) bb[b] = pb[s2 * K::LDB + b * 32];
#pragma unroll
      for (int t = 0; t < K::TM; ++t) {
        const float gn = pn[t * 32 * kWmLDA + s2], gp = pd[t * 32 * kWmLDA + s2];
#pragma unroll
        for (int b = 0; b < K::TN; ++b) {
          accn[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gn, bb[b], accn[t][b], 0, 0, 0);
          accd[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp, bb[b], accd[t][b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  float* pn = on + (size_t)prob * bstride + (size_t)blockIdx.z * pstride;
  float* pd = od + (size_t)prob * bstride + (size_t)blockIdx.z * pstride;
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b) {
      const int r = r0 + wn * K::TN * 32 + b * 32 + j;      // < RP: the rank tiles cover the padded rank exactly
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + wm * K::TM * 32 + t * 32 + wmu_tile_row(e, hl);
        if (i < rows) {
          pn[(size_t)i * RP + r] = r < rank ? accn[t][b][e] : 0.f;
          pd[(size_t)i * RP + r] = r < rank ? accd[t][b][e] : 0.f;
        }
      }
    }
}

// A problem's parts added in part order, then the two planes stored (terms) or nmf.py:78-92 applied in place (step): the body
// of the two finish kernels, blk of fblocks workgroups of problem prob.
__device__ __forceinline__ void bmu_finish_problem(const float* __restrict__ ws_b, int parts, int rows, int rank, int r_pad,
                                                   float* owner_b, float* __restrict__ num_b, float* __restrict__ den_b, int step,
                                                   const MaskedApply& ap, int fblocks, int prob, int blk) {
  const int64_t plane = (int64_t)rows * r_pad;
  const float* ws = ws_b + (size_t)prob * parts * 2 * plane;
  for (int64_t at = (int64_t)blk * 256 + threadIdx.x; at < plane; at += (int64_t)fblocks * 256) {
    float n = ws[at], d = ws[plane + at];
    for (int p = 1; p < parts; ++p) n += ws[(size_t)p * 2 * plane + at], d += ws[(size_t)p * 2 * plane + plane + at];
    if (step) {
      const int r = (int)(at % r_pad);
      float* f = owner_b + (size_t)prob * rows * rank + (size_t)(at / r_pad) * rank + r;
      if (r < rank) *f = masked_apply(*f, n, d, ap);
    } else {
      num_b[(size_t)prob * plane + at] = n, den_b[(size_t)prob * plane + at] = d;
    }
  }
}

// grid.x = problems x fblocks
__global__ void __launch_bounds__(256) bmu_finish_kernel(const float* __restrict__ ws_b, int parts, int rows, int rank,
                                                         int r_pad, float* owner_b, float* __restrict__ num_b,
                                                         float* __restrict__ den_b, int step, MaskedApply ap, int fblocks,
                                                         const int32_t* __restrict__ active) {
  const int prob = blockIdx.x / fblocks, blk = blockIdx.x - prob * fblocks;
  if (active && !active[prob]) return;
  bmu_finish_problem(ws_b, parts, rows, rank, r_pad, owner_b, num_b, den_b, step, ap, fblocks, prob, blk);
}

// the same with the problem's own (l1, l2) from reg [batch][2] in the apply
__global__ void __launch_bounds__(256) bmu_finish_reg_kernel(const float* __restrict__ ws_b, int parts, int rows, int rank,
                                                             int r_pad, float* owner_b, float* __restrict__ num_b,
                                                             float* __restrict__ den_b, int step, MaskedApply ap, int fblocks,
                                                             const int32_t* __restrict__ active,
                                                             const float* __restrict__ reg) {
  const int prob = blockIdx.x / fblocks, blk = blockIdx.x - prob * fblocks;
  if (active && !active[prob]) return;
  ap.l1 = reg[2 * prob], ap.l2 = reg[2 * prob + 1];
  bmu_finish_problem(ws_b, parts, rows, rank, r_pad, owner_b, num_b, den_b, step, ap, fblocks, prob, blk);
}

// part[problem * nblk + tile * nparts + z] = sum over the tile's rows and the part's columns of the term of metrics.beta_div
// that holds y, in double: per lane, per wave (fixed-order butterfly), per workgroup
template <int RP, int KIND>
__global__ void __launch_bounds__(256) bmu_loss_kernel(const float* __restrict__ Vb, int64_t vstride, int64_t ld, int rows,
                                                       int C, const float* __restrict__ owner_b,
                                                       const float* __restrict__ panel_b, int rank, float beta, int part_len,
                                                       int nparts, int nblk, const int32_t* __restrict__ active,
                                                       double* __restrict__ part) {
  using K = WmuCfg<RP>;
  const int prob = blockIdx.x / nblk;
  if (active && !active[prob]) return;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  __shared__ double red[4];
  const float* V = Vb + (size_t)prob * vstride;
  const float* owner = owner_b + (size_t)prob * rows * rank;
  const float* panel = panel_b + (size_t)prob * C * rank;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int blk = blockIdx.x - prob * nblk;
  const int i0 = (blk / nparts) * kWmRows;
  const int cbeg = (blk % nparts) * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  const bool vec = bmu_vec(Vb, vstride, ld);
  double tot = 0.0;
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    BmuStage<RP> st;
    bmu_load_v<RP, false>(st, V, ld, rows, i0, c0, cend, vec, tid);
    wmu_load_panel<RP>(st, panel, rank, c0, cend, tid);
    bmu_store_v<RP, false>(sv, st, tid);
    wmu_store_panel<RP>(sb, st, tid);
    __syncthreads();
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
    const bool col_ok = c0 + j < cend;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wave * 32 + wmu_tile_row(e, hl);
      const double t = masked_loss_term<KIND>(sv[row * kWmLDA + j], y[e], beta);
      tot += (col_ok && i0 + row < rows) ? t : 0.0;
    }
    __syncthreads();
  }
  store_lane_totals(tot, red, part);
}

// bmu_loss_kernel over the weighted entries: every term times m in double; m = 0 outside the matrix and the part
template <int RP, int KIND>
__global__ void __launch_bounds__(256) bwmu_loss_kernel(const float* __restrict__ Vb, int64_t vstride,
                                                        const float* __restrict__ Mb, int64_t mstride,
                                                        const int32_t* __restrict__ m_index, int64_t ld, int rows, int C,
                                                        const float* __restrict__ owner_b, const float* __restrict__ panel_b,
                                                        int rank, float beta, int part_len, int nparts, int nblk,
                                                        const int32_t* __restrict__ active, double* __restrict__ part) {
  using K = WmuCfg<RP>;
  const int prob = blockIdx.x / nblk;
  if (active && !active[prob]) return;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  __shared__ double red[4];
  const float* V = Vb + (size_t)prob * vstride;
  const float* M = bwmu_weights(Mb, mstride, m_index, prob);
  const float* owner = owner_b + (size_t)prob * rows * rank;
  const float* panel = panel_b + (size_t)prob * C * rank;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int blk = blockIdx.x - prob * nblk;
  const int i0 = (blk / nparts) * kWmRows;
  const int cbeg = (blk % nparts) * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  const bool vec = bwmu_vec(Vb, vstride, Mb, mstride, ld);
  double tot = 0.0;
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    WmuStage<RP> st;
    wmu_load_vm<RP, false>(st, V, M, ld, rows, i0, c0, cend, vec, tid);
    wmu_load_panel<RP>(st, panel, rank, c0, cend, tid);
    wmu_store_vm<RP, false>(sv, sm, st, tid);
    wmu_store_panel<RP>(sb, st, tid);
    __syncthreads();
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int at = (wave * 32 + wmu_tile_row(e, hl)) * kWmLDA + j;
      const float m = sm[at];
      const double t = masked_loss_term<KIND>(sv[at], y[e], beta);
      tot += m > 0.f ? (double)m * t : 0.0;
    }
    __syncthreads();
  }
  store_lane_totals(tot, red, part);
}

// out[problem] = (v_term[problem] + the problem's nblk partials) * mul: one workgroup per problem, strided lanes in block
// order, then a tree -- a pure function of nblk
__global__ void __launch_bounds__(256) bmu_reduce_kernel(const double* __restrict__ part, int nblk,
                                                         const double* __restrict__ v_term, double mul,
                                                         const int32_t* __restrict__ active, double* __restrict__ out) {
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (active && !active[prob]) return;
  __shared__ double red[256];
  double s = 0.0;
  for (int i = tid; i < nblk; i += 256) s += part[(size_t)prob * nblk + i];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[prob] = (v_term[prob] + red[0]) * mul;
}

// out[problem] = the sum over the problem's entries of the terms of metrics.beta_div that hold v alone (metrics.py:22, 57,
// 85-96), every term and the sum in double: one workgroup per problem, strided lanes, then a tree -- a pure function of the
// problem's own entries, whatever the batch around it
__global__ void __launch_bounds__(256) bmu_v_term_kernel(const float* __restrict__ Vb, int64_t vstride, int64_t ld, int n, int c,
                                                         double beta, int kind, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float* V = Vb + (size_t)blockIdx.x * vstride;
  const double e = (double)kEps;
  double s = 0.0;
  for (int64_t at = tid; at < (int64_t)n * c; at += 256) {
    const double v = (double)V[(size_t)(at / c) * ld + at % c];
    if (kind == NMFMU_BETA_KL) s += v * log(v + e) - v;
    else if (kind == NMFMU_BETA_IS) s += -log(v + e) - 1.0;
    else s += pow(beta < 0.0 ? v + e : v, beta);
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = kind == NMFMU_BETA_EUC ? 0.0 : red[0];
}

// bmu_v_term_kernel over the weighted entries: m times the term, both in double; an entry with m == 0 is selected away
__global__ void __launch_bounds__(256) bwmu_v_term_kernel(const float* __restrict__ Vb, int64_t vstride,
                                                          const float* __restrict__ Mb, int64_t mstride,
                                                          const int32_t* __restrict__ m_index, int64_t ld, int n, int c,
                                                          double beta, int kind, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float* V = Vb + (size_t)blockIdx.x * vstride;
  const float* M = bwmu_weights(Mb, mstride, m_index, blockIdx.x);
  const double e = (double)kEps;
  double s = 0.0;
  for (int64_t at = tid; at < (int64_t)n * c; at += 256) {
    const size_t off = (size_t)(at / c) * ld + at % c;
    const float m = M[off];
    if (!(m > 0.f)) continue;
    const double v = (double)V[off];
    double t;
    if (kind == NMFMU_BETA_KL) t = v * log(v + e) - v;
    else if (kind == NMFMU_BETA_IS) t = -log(v + e) - 1.0;
    else t = pow(beta < 0.0 ? v + e : v, beta);
    s += (double)m * t;
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = kind == NMFMU_BETA_EUC ? 0.0 : red[0];
}

// One workgroup; one thread per problem (strided over the batch).  nmf.py:402-407 in double on loss = sqrt(2 div) (NaN for
// a negative divergence: no comparison with it holds, so such a problem never stops).
__global__ void __launch_bounds__(256) bmu_judge_kernel(int batch, const double* __restrict__ div,
                                                        const double* __restrict__ loss_init, double* __restrict__ previous,
                                                        double tol, int iteration, int32_t* __restrict__ active,
                                                        int64_t* __restrict__ n_iter, int32_t* __restrict__ n_active) {
  __shared__ int red[256];
  const int tid = threadIdx.x;
  int alive = 0;
  for (int b = tid; b < batch; b += 256) {
    if (!active[b]) continue;
    const double d = 2.0 * div[b];
    const double loss = d >= 0.0 ? sqrt(d) : __longlong_as_double(0x7ff8000000000000ll);
    if ((previous[b] - loss) / loss_init[b] < tol) {
      n_iter[b] = iteration + 1;
      active[b] = 0;
    } else {
      previous[b] = loss;
      ++alive;
    }
  }
  red[tid] = alive;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) *n_active = red[0];
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
constexpr int kFinishBlocks = 4096;      // the finish kernel's workgroups per problem, at most

// NMFMU_OK or the answer the entries give before any device work
int bmu_check(const void* V, int64_t vstride, int64_t ld, int batch, int n, int c, const void* owner, const void* panel,
              int rank, int r_pad, bool has_r_pad) {
  if (!V || !owner || !panel || batch <= 0 || n <= 0 || c <= 0 || ld < c || vstride < 0) return NMFMU_ERR_ARG;
  if (rank <= 0) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (has_r_pad && r_pad != nmfmu_pad_rank(rank)) return NMFMU_ERR_ARG;
  return NMFMU_OK;
}

// the weights' own arguments: a negative stride, or an index without weights to index
int bwmu_check(const void* M, int64_t mstride, const void* m_index) {
  return (mstride < 0 || (m_index && !M)) ? NMFMU_ERR_ARG : NMFMU_OK;
}

int bmu_finish_blocks(int64_t plane) { return (int)std::min<int64_t>((plane + 255) / 256, kFinishBlocks); }

bool bmu_grid_fits(int batch, int64_t blocks_per_problem) { return (int64_t)batch * blocks_per_problem <= INT_MAX; }

// M == nullptr: the unweighted kernel.  reg: per-problem (l1, l2) for the apply, or nullptr.
int bmu_launch(const float* V, int64_t vstride, const float* M, int64_t mstride, const int32_t* m_index, int64_t ld, int batch,
               int n, int c, int side, float* owner, const float* panel, int rank, int r_pad, float beta, int nsplit,
               const int32_t* active, float* ws, float* num, float* den, int step, MaskedApply ap, const float* reg,
               hipStream_t st) {
  const int rows = side ? c : n, contraction = side ? n : c;
  const int parts = wmu_split(rows, contraction, r_pad, nsplit);
  const int part_len = wmu_part_len(contraction, parts);
  const int64_t plane = (int64_t)rows * r_pad;
  const int row_tiles = (rows + kWmRows - 1) / kWmRows, fblocks = bmu_finish_blocks(plane);
  if (!bmu_grid_fits(batch, row_tiles) || !bmu_grid_fits(batch, fblocks)) return NMFMU_ERR_UNSUPPORTED;
  const bool direct = !step && parts == 1;       // one part of terms: the kernel's planes are the result
  float* on = direct ? num : ws;
  float* od = direct ? den : ws + plane;
  const int64_t pstride = 2 * plane, bstride = direct ? plane : (int64_t)parts * 2 * plane;
  const dim3 grid((unsigned)(batch * row_tiles), (r_pad + 127) / 128, parts);
  for_rp(r_pad, [&](auto rp) {
    for_kind(nmfmu_beta_kind(beta), [&](auto k) {
      constexpr int RP = decltype(rp)::value, KIND = decltype(k)::value;
      if (M && side)
        hipLaunchKernelGGL((bwmu_kernel<RP, true, KIND>), grid, dim3(256), 0, st, V, vstride, M, mstride, m_index, ld, rows,
                           contraction, owner, panel, rank, beta, part_len, row_tiles, active, on, od, pstride, bstride);
      else if (M)
        hipLaunchKernelGGL((bwmu_kernel<RP, false, KIND>), grid, dim3(256), 0, st, V, vstride, M, mstride, m_index, ld, rows,
                           contraction, owner, panel, rank, beta, part_len, row_tiles, active, on, od, pstride, bstride);
      else if (side)
        hipLaunchKernelGGL((bmu_kernel<RP, true, KIND>), grid, dim3(256), 0, st, V, vstride, ld, rows, contraction, owner,
                           panel, rank, beta, part_len, row_tiles, active, on, od, pstride, bstride);
      else
        hipLaunchKernelGGL((bmu_kernel<RP, false, KIND>), grid, dim3(256), 0, st, V, vstride, ld, rows, contraction, owner,
                           panel, rank, beta, part_len, row_tiles, active, on, od, pstride, bstride);
    });
  });
  if (!direct && reg)
    hipLaunchKernelGGL(bmu_finish_reg_kernel, dim3((unsigned)(batch * fblocks)), dim3(256), 0, st, ws, parts, rows, rank, r_pad,
                       owner, num, den, step, ap, fblocks, active, reg);
  else if (!direct)
    hipLaunchKernelGGL(bmu_finish_kernel, dim3((unsigned)(batch * fblocks)), dim3(256), 0, st, ws, parts, rows, rank, r_pad,
                       owner, num, den, step, ap, fblocks, active);
  return (int)hipGetLastError();
}

int bmu_loss_split(int n, int c) { return wmu_auto_split((n + kWmRows - 1) / kWmRows, c); }
}  // namespace

extern "C" {

int nmfmu_bmu_nsplit(int rows, int contraction, int r_pad) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0) return NMFMU_ERR_ARG;
  return wmu_split(rows, contraction, r_pad, 0);
}

int64_t nmfmu_bmu_ws(int batch, int rows, int contraction, int r_pad, int nsplit) {
  if (batch <= 0 || rows <= 0 || contraction <= 0 || r_pad <= 0 || nsplit < 0) return 0;
  return (int64_t)batch * wmu_split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad;
}

int nmfmu_bmu_terms(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, int side, const float* owner,
                    const float* panel, int rank, int r_pad, float beta, int nsplit, const int32_t* active, float* ws,
                    float* num, float* den, void* stream) {
  if (!ws || !num || !den || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = bmu_check(V, v_batch_stride, ld, batch, n, c, owner, panel, rank, r_pad, true)) return rc;
  return bmu_launch(V, v_batch_stride, nullptr, 0, nullptr, ld, batch, n, c, side, const_cast<float*>(owner), panel, rank, r_pad,
                    beta, nsplit, active, ws, num, den, 0, MaskedApply{0.f, 0.f, 1.f}, nullptr, S(stream));
}

int nmfmu_bmu_step(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, int side, float* owner,
                   const float* panel, int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit,
                   const int32_t* active, float* ws, void* stream) {
  if (!ws || owner == panel || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = bmu_check(V, v_batch_stride, ld, batch, n, c, owner, panel, rank, r_pad, true)) return rc;
  return bmu_launch(V, v_batch_stride, nullptr, 0, nullptr, ld, batch, n, c, side, owner, panel, rank, r_pad, beta, nsplit,
                    active, ws, nullptr, nullptr, 1, MaskedApply{l1, l2, gamma}, nullptr, S(stream));
}

int nmfmu_bmu_loss_parts(int n, int c) {
  if (n <= 0 || c <= 0) return NMFMU_ERR_ARG;
  return (n + kWmRows - 1) / kWmRows * bmu_loss_split(n, c);
}

int nmfmu_bmu_loss(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, const float* H, const float* W,
                   int rank, float beta, const double* v_term, const int32_t* active, double* part, double* out,
                   void* stream) {
  return nmfmu_bwmu_loss(V, v_batch_stride, nullptr, 0, nullptr, ld, batch, n, c, H, W, rank, beta, v_term, active, part, out,
                         stream);
}

int nmfmu_bwmu_loss(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                    int64_t ld, int batch, int n, int c, const float* H, const float* W, int rank, float beta,
                    const double* v_term, const int32_t* active, double* part, double* out, void* stream) {
  if (!part || !out || !v_term) return NMFMU_ERR_ARG;
  if (const int rc = bwmu_check(M, m_batch_stride, m_index)) return rc;
  if (const int rc = bmu_check(V, v_batch_stride, ld, batch, n, c, H, W, rank, 0, false)) return rc;
  const int nparts = bmu_loss_split(n, c), part_len = wmu_part_len(c, nparts);
  const int nblk = (n + kWmRows - 1) / kWmRows * nparts;
  if (!bmu_grid_fits(batch, nblk)) return NMFMU_ERR_UNSUPPORTED;
  const int kind = nmfmu_beta_kind(beta);
  for_rp(nmfmu_pad_rank(rank), [&](auto rp) {
    for_kind(kind, [&](auto k) {
      constexpr int RP = decltype(rp)::value, KIND = decltype(k)::value;
      const dim3 grid((unsigned)(batch * nblk));
      if (M)
        hipLaunchKernelGGL((bwmu_loss_kernel<RP, KIND>), grid, dim3(256), 0, S(stream), V, v_batch_stride, M, m_batch_stride,
                           m_index, ld, n, c, H, W, rank, beta, part_len, nparts, nblk, active, part);
      else
        hipLaunchKernelGGL((bmu_loss_kernel<RP, KIND>), grid, dim3(256), 0, S(stream), V, v_batch_stride, ld, n, c, H, W, rank,
                           beta, part_len, nparts, nblk, active, part);
    });
  });
  // metrics.py:39 halves the sum of squares; metrics.py:96 divides by beta (beta - 1)
  double mul = 1.0;
  if (kind == NMFMU_BETA_EUC) mul = 0.5;
  if (kind == NMFMU_BETA_GEN) mul = 1.0 / ((double)beta * ((double)beta - 1.0));
  hipLaunchKernelGGL(bmu_reduce_kernel, dim3(batch), dim3(256), 0, S(stream), part, nblk, v_term, mul, active, out);
  return (int)hipGetLastError();
}

int nmfmu_bmu_v_term(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, float beta, double* out,
                     void* stream) {
  if (!V || !out || batch <= 0 || n <= 0 || c <= 0 || ld < c || v_batch_stride < 0) return NMFMU_ERR_ARG;
  hipLaunchKernelGGL(bmu_v_term_kernel, dim3(batch), dim3(256), 0, S(stream), V, v_batch_stride, ld, n, c, (double)beta,
                     nmfmu_beta_kind(beta), out);
  return (int)hipGetLastError();
}

int nmfmu_bwmu_terms(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                     int64_t ld, int batch, int n, int c, int side, const float* owner, const float* panel, int rank, int r_pad,
                     float beta, int nsplit, const int32_t* active, float* ws, float* num, float* den, void* stream) {
  if (!ws || !num || !den || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = bwmu_check(M, m_batch_stride, m_index)) return rc;
  if (const int rc = bmu_check(V, v_batch_stride, ld, batch, n, c, owner, panel, rank, r_pad, true)) return rc;
  return bmu_launch(V, v_batch_stride, M, m_batch_stride, m_index, ld, batch, n, c, side, const_cast<float*>(owner), panel, rank,
                    r_pad, beta, nsplit, active, ws, num, den, 0, MaskedApply{0.f, 0.f, 1.f}, nullptr, S(stream));
}

int nmfmu_bwmu_step(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                    int64_t ld, int batch, int n, int c, int side, float* owner, const float* panel, int rank, int r_pad,
                    float beta, float l1, float l2, const float* reg, float gamma, int nsplit, const int32_t* active, float* ws,
                    void* stream) {
  if (!ws || owner == panel || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = bwmu_check(M, m_batch_stride, m_index)) return rc;
  if (const int rc = bmu_check(V, v_batch_stride, ld, batch, n, c, owner, panel, rank, r_pad, true)) return rc;
  return bmu_launch(V, v_batch_stride, M, m_batch_stride, m_index, ld, batch, n, c, side, owner, panel, rank, r_pad, beta,
                    nsplit, active, ws, nullptr, nullptr, 1, MaskedApply{l1, l2, gamma}, reg, S(stream));
}

int nmfmu_bwmu_v_term(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                      int64_t ld, int batch, int n, int c, float beta, double* out, void* stream) {
  if (const int rc = bwmu_check(M, m_batch_stride, m_index)) return rc;
  if (!M) return nmfmu_bmu_v_term(V, v_batch_stride, ld, batch, n, c, beta, out, stream);
  if (!V || !out || batch <= 0 || n <= 0 || c <= 0 || ld < c || v_batch_stride < 0) return NMFMU_ERR_ARG;
  hipLaunchKernelGGL(bwmu_v_term_kernel, dim3(batch), dim3(256), 0, S(stream), V, v_batch_stride, M, m_batch_stride, m_index,
                     ld, n, c, (double)beta, nmfmu_beta_kind(beta), out);
  return (int)hipGetLastError();
}

int nmfmu_bmu_judge(int batch, const double* div, const double* loss_init, double* previous, double tol, int iteration,
                    int32_t* active, int64_t* n_iter, int32_t* n_active, void* stream) {
  if (batch <= 0 || !div || !loss_init || !previous || !active || !n_iter || !n_active || iteration < 0) return NMFMU_ERR_ARG;
  hipLaunchKernelGGL(bmu_judge_kernel, dim3(1), dim3(256), 0, S(stream), batch, div, loss_init, previous, tol, iteration,
                     active, n_iter, n_active);
  return (int)hipGetLastError();
}

}  // extern "C"
