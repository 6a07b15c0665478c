// Weighted NMF on a dense target: L = sum_ij m_ij d_beta(v_ij | y_ij), y = H W^T, m_ij >= 0 a dense mask or dense weights.
// Both seeds of the multiplicative update (nmf.py:61-74) are multiplied by m:
//
//   num[i][r] = sum_c (m g_neg(v, y))(i, c) panel[c][r]      den[i][r] = sum_c (m g_pos(y))(i, c) panel[c][r]
//
// with (i, c) = (row, column) of V for the H side and (column, row) for the W side: V and M are walked along their rows or
// along their columns IN PLACE, one kernel templated on that, no transposed copy of either.  Where m == 0 the entry is
// SELECTED away (not multiplied): whatever V holds there -- NaN, Inf, a negative value -- reaches neither term nor the loss.
//
// One fused kernel per half-step, exact fp32 (v_mfma_f32_32x32x2_f32, bitwise a k-ordered fmaf chain).  A workgroup (4 waves)
// owns 128 owner rows x a rank tile of <= 128 x one part of the contraction axis.  Its owner rows stay in registers (wave w:
// rows 32 w .. 32 w + 31, one row per lane pair, r_pad / 2 registers).  Per stage of 32 contraction steps:
//   1. V, M (128 x 32 each, [i][c] with a row stride of 33 floats for either walk) and the panel rows (32 x r_pad) go to LDS
//      from registers that were loaded one stage ahead, and the next stage's loads are issued;
//   2. wave w forms Y[32 w ..][32 c] by r_pad / 2 MFMAs over the FULL padded rank (owner registers x panel rows in LDS);
//   3. every lane turns the 16 elements of Y it holds into m g_neg and m g_pos and writes them over V and M in LDS;
//   4. num and den accumulate by MFMA into register tiles (2 x 2 x 2 tiles of 32 x 32 per wave at a rank tile of 128).
// Y and m g never reach HBM.  The contraction is cut into parts (wmu_auto_split: a pure function of the shape); every part
// stores its two planes to a caller-owned slab [part][num | den][rows][r_pad] with plain stores and wmu_finish_kernel adds
// them in part order, then stores the planes (terms) or applies nmf.py:78-92 to the owner's fp32 master (step) -- in a second
// kernel because every part of every row tile reads the owner.  No atomics, no fences: a repeated call is bitwise identical
// whatever the workspace held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

// grid = (row tiles, rank tiles, parts).  on / od + part * pstride: the part's planes [rows][RP].
template <int RP, bool TRANS, int KIND>
__global__ void __launch_bounds__(256) wmu_kernel(const float* __restrict__ V, const float* __restrict__ M, int64_t ld,
                                                  int rows, int C, const float* __restrict__ owner,
                                                  const float* __restrict__ panel, int rank, float beta, int part_len,
                                                  float* __restrict__ on, float* __restrict__ od, int64_t pstride) {
  using K = WmuCfg<RP>;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave / K::WN, wn = wave % K::WN;
  const int i0 = blockIdx.x * kWmRows, r0 = blockIdx.y * K::RT;
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
  // 16-byte loads need 16-byte aligned rows of both operands
  const bool vec = (ld & 3) == 0 && ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(M)) & 15) == 0;
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
  float* pn = on + (size_t)blockIdx.z * pstride;
  float* pd = od + (size_t)blockIdx.z * pstride;
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

// the slab's parts added in part order, then the two planes stored (terms) or nmf.py:78-92 applied in place (step)
__global__ void __launch_bounds__(256) wmu_finish_kernel(const float* __restrict__ ws, int parts, int rows, int rank, int r_pad,
                                                         float* owner, float* __restrict__ num, float* __restrict__ den,
                                                         int step, MaskedApply ap) {
  const int64_t plane = (int64_t)rows * r_pad;
  for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < plane; at += (int64_t)gridDim.x * 256) {
    float n = ws[at], d = ws[plane + at];
    for (int p = 1; p < parts; ++p) n += ws[(size_t)p * 2 * plane + at], d += ws[(size_t)p * 2 * plane + plane + at];
    if (step) {
      const int r = (int)(at % r_pad);
      float* f = owner + (size_t)(at / r_pad) * rank + r;
      if (r < rank) *f = masked_apply(*f, n, d, ap);
    } else {
      num[at] = n, den[at] = d;
    }
  }
}

// part[tile * nparts + z] = sum over the tile's rows and the part's columns of m * (the term of metrics.beta_div that holds
// y), in double: per lane, per wave (fixed-order butterfly), per workgroup
template <int RP, int KIND>
__global__ void __launch_bounds__(256) wmu_loss_kernel(const float* __restrict__ V, const float* __restrict__ M, int64_t ld,
                                                       int rows, int C, const float* __restrict__ owner,
                                                       const float* __restrict__ panel, int rank, float beta, int part_len,
                                                       int nparts, double* __restrict__ part) {
  using K = WmuCfg<RP>;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int i0 = (blockIdx.x / nparts) * kWmRows;
  const int cbeg = (blockIdx.x % nparts) * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  const bool vec = (ld & 3) == 0 && ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(M)) & 15) == 0;
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

}  // namespace nmfmu

using namespace nmfmu;

namespace {
// NMFMU_OK or the answer the entries give before any device work
int wmu_check(const void* V, const void* M, int64_t ld, int n, int c, const void* owner, const void* panel, int rank,
              int r_pad, bool has_r_pad) {
  if (!V || !M || !owner || !panel || n <= 0 || c <= 0 || ld < c) return NMFMU_ERR_ARG;
  if (rank <= 0) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (has_r_pad && r_pad != nmfmu_pad_rank(rank)) return NMFMU_ERR_ARG;
  return NMFMU_OK;
}

int wmu_launch(const float* V, const float* M, int64_t ld, int n, int c, int side, float* owner, const float* panel, int rank,
               int r_pad, float beta, int nsplit, float* ws, float* num, float* den, int step, MaskedApply ap,
               hipStream_t st) {
  const int rows = side ? c : n, contraction = side ? n : c;
  const int parts = wmu_split(rows, contraction, r_pad, nsplit);
  const int part_len = wmu_part_len(contraction, parts);
  const int64_t plane = (int64_t)rows * r_pad;
  const bool direct = !step && parts == 1;       // one part of terms: the kernel's planes are the result
  float* on = direct ? num : ws;
  float* od = direct ? den : ws + plane;
  const dim3 grid((rows + kWmRows - 1) / kWmRows, (r_pad + 127) / 128, parts);
  for_rp(r_pad, [&](auto rp) {
    for_kind(nmfmu_beta_kind(beta), [&](auto k) {
      constexpr int RP = decltype(rp)::value, KIND = decltype(k)::value;
      if (side)
        hipLaunchKernelGGL((wmu_kernel<RP, true, KIND>), grid, dim3(256), 0, st, V, M, ld, rows, contraction, owner, panel,
                           rank, beta, part_len, on, od, 2 * plane);
      else
        hipLaunchKernelGGL((wmu_kernel<RP, false, KIND>), grid, dim3(256), 0, st, V, M, ld, rows, contraction, owner, panel,
                           rank, beta, part_len, on, od, 2 * plane);
    });
  });
  if (!direct) {
    const int fgrid = (int)std::min<int64_t>((plane + 255) / 256, 4096);
    hipLaunchKernelGGL(wmu_finish_kernel, dim3(fgrid), dim3(256), 0, st, ws, parts, rows, rank, r_pad, owner, num, den, step,
                       ap);
  }
  return (int)hipGetLastError();
}

int wmu_loss_split(int n, int c) { return wmu_auto_split((n + kWmRows - 1) / kWmRows, c); }
}  // namespace

extern "C" {

int nmfmu_wmu_nsplit(int rows, int contraction, int r_pad) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0) return NMFMU_ERR_ARG;
  return wmu_split(rows, contraction, r_pad, 0);
}

int64_t nmfmu_wmu_ws(int rows, int contraction, int r_pad, int nsplit) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0 || nsplit < 0) return 0;
  return (int64_t)wmu_split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad;
}

int nmfmu_wmu_terms(const float* V, const float* M, int64_t ld, int n, int c, int side, const float* owner,
                    const float* panel, int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den,
                    void* stream) {
  if (!ws || !num || !den || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = wmu_check(V, M, ld, n, c, owner, panel, rank, r_pad, true)) return rc;
  return wmu_launch(V, M, ld, n, c, side, const_cast<float*>(owner), panel, rank, r_pad, beta, nsplit, ws, num, den, 0,
                    MaskedApply{0.f, 0.f, 1.f}, S(stream));
}

int nmfmu_wmu_step(const float* V, const float* M, int64_t ld, int n, int c, int side, float* owner, const float* panel,
                   int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit, float* ws, void* stream) {
  if (!ws || owner == panel || nsplit < 0 || (side != 0 && side != 1)) return NMFMU_ERR_ARG;
  if (const int rc = wmu_check(V, M, ld, n, c, owner, panel, rank, r_pad, true)) return rc;
  return wmu_launch(V, M, ld, n, c, side, owner, panel, rank, r_pad, beta, nsplit, ws, nullptr, nullptr, 1,
                    MaskedApply{l1, l2, gamma}, S(stream));
}

int nmfmu_wmu_loss_parts(int n, int c) {
  if (n <= 0 || c <= 0) return NMFMU_ERR_ARG;
  return (n + kWmRows - 1) / kWmRows * wmu_loss_split(n, c);
}

int nmfmu_wmu_loss(const float* V, const float* M, int64_t ld, int n, int c, const float* H, const float* W, int rank,
                   float beta, double v_term, double* part, double* out, void* stream) {
  if (!part || !out) return NMFMU_ERR_ARG;
  if (const int rc = wmu_check(V, M, ld, n, c, H, W, rank, 0, false)) return rc;
  const int nparts = wmu_loss_split(n, c), part_len = wmu_part_len(c, nparts);
  const int nblk = (n + kWmRows - 1) / kWmRows * nparts;
  const int kind = nmfmu_beta_kind(beta);
  for_rp(nmfmu_pad_rank(rank), [&](auto rp) {
    for_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((wmu_loss_kernel<decltype(rp)::value, decltype(k)::value>), dim3(nblk), dim3(256), 0, S(stream), V,
                         M, ld, n, c, H, W, rank, beta, part_len, nparts, part);
    });
  });
  // metrics.py:39 halves the sum of squares; metrics.py:96 divides by beta (beta - 1)
  double mul = 1.0;
  if (kind == NMFMU_BETA_EUC) mul = 0.5;
  if (kind == NMFMU_BETA_GEN) mul = 1.0 / ((double)beta * ((double)beta - 1.0));
  hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, nblk, v_term, mul, out);
  return (int)hipGetLastError();
}

}  // extern "C"
