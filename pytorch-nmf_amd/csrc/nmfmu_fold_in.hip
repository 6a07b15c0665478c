// Fold-in: new rows of a target against a FIXED panel W -- every iteration of the H half-step of a row inside one launch
// (NMF.transform).  With W fixed the rows are independent: h = H[row] depends on W and on the row's
// stored entries alone, so a row is iterated to its end by one wave (or one workgroup) that never leaves the kernel:
//
//   s_j = <h, W[j]>                                   j over the stored columns of the row
//   num = sum_j g_neg(v_j, s_j) W[j],  den = sum_j g_pos(s_j) W[j]       (missing: nmfmu_sparse_masked.hip's g per branch)
//   h  *= ((relu(num) + eps) / (den' + l1 + l2 h))^gamma                 (nmf.py:78-92)
//
//   mode missing       : den' = relu(den) + eps
//   mode zero, beta 1  : num = sum_j v_j / (s_j + eps) W[j],  den' = aux[r] = colsum(W), as it is (nmf.py:128-131)
//   mode zero, beta 2  : num = sum_j v_j W[j], formed once;   den' = relu(sum_q h[q] aux[q][r]) + eps, aux = W^T W
//
// The row's entries are cut into blocks of <= B; a block's W rows are staged in LDS (row stride rank | 1: odd, so the lanes
// of pass 1, one per entry, hit different banks).  A range that is a single block is staged ONCE, before the first iteration,
// and every iteration runs from LDS alone; a longer range restages its blocks every iteration, in order.
//
//   pass 1  lanes across the ENTRIES of the block: s_j as an r-ordered fmaf chain against h (LDS, one address for the whole
//           wave), then g_neg / g_pos, to LDS
//   pass 2  lanes across the RANK, RL slots per lane (slot q of a lane is rank column lane + 64 q): num / den as j-ordered
//           fmaf chains that run on across the blocks, so the arithmetic does not depend on B
//
// Both contractions are lane-private chains in a fixed order: no cross-lane butterfly.  Then the apply and the stop test
// max_r |h_k - h_{k-1}| <= tol * max_r h_k (fp32; the two maxima are order-independent).
//
// A row of more than `long_rows` entries (default: the largest block of the rank, what one wave keeps resident) takes the whole
// workgroup, so that a row of up to four blocks is still fetched once: wave w owns the entries [w per, (w + 1) per) of the row,
// per = ceil(count / 4) -- a function of the count alone -- and iterates them in blocks as above; the four [num | den]
// partials go through LDS and are added in wave order by every wave (each keeps its own copy of h: same bits, no broadcast),
// one barrier pair per iteration.  Which path a row takes is a function of its count and long_rows only, and nothing is
// shared between rows: a row's result is bitwise independent of B and of the other rows of the call.  Plain vector stores,
// no atomics, no fences; H is read and written by the row's own wave / workgroup, W and aux are read-only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr int kFoldWaves = 4;
constexpr int kFoldLdsFloats = 16384;      // 64 KiB per workgroup
constexpr int kFoldU = 4;                  // W rows in flight per wave while staging, row by row
constexpr int kFoldV = 8;                  // float4 loads in flight per lane while staging a block as one run

struct FoldArgs {
  const int32_t* rowptr;
  const int32_t* colidx;
  const float* vals;
  const int32_t* order;     // NULL: rows in their own order
  float* H;
  const float* W;
  const float* aux;         // zero mode: colsum(W) [rank] (beta 1) or W^T W [rank][rank] (beta 2)
  int32_t* n_iter;          // NULL, or [n_rows]
  int n_rows, rank, block, long_rows, max_iter, per_wave;
  int vec;                  // rank % 4 == 0 and W 16-byte aligned: a block is staged with float4 loads
  float beta, l1, l2, gamma, tol;
};

// floats of LDS a wave owns: the panel block, g_neg, g_pos and h; a multiple of 4
__host__ __device__ inline int fold_per_wave(int rank, int block, int rl) {
  return (block * ((rank | 1) + 2) + 64 * rl + 3) & ~3;
}

// (g_neg, g_pos) of one stored entry -- masked_g of nmfmu_sparse_masked.hip, operation for operation
template <int KIND>
__device__ __forceinline__ void fold_g(float v, float s, float beta, float& gn, float& gp) {
  if constexpr (KIND == NMFMU_BETA_EUC) {
    gn = v, gp = s;
  } else if constexpr (KIND == NMFMU_BETA_KL) {
    gn = v / (s + kEps), gp = 1.f;
  } else if constexpr (KIND == NMFMU_BETA_IS) {
    const float r = 1.f / (s + kEps);
    gp = r, gn = r * r * v;
  } else {
    const float se = s + kEps;
    const float p2 = exp2f((beta - 2.f) * log2f(se));
    gn = p2 * v, gp = p2 * se;
  }
}

// the W rows of the block's nb entries -> panel[j][r] (stride S); this lane's entry is base + lane.  With rank a multiple of
// 4 (and W 16-byte aligned) the block is one run of nb * rank / 4 float4 loads, kFoldV per lane in flight (a 64-float row is 16 lanes: a trip holds up
// to 32 rows); otherwise row by row, kFoldU rows in flight.
template <int RL>
__device__ __forceinline__ void fold_stage(float* panel, int S, const float* __restrict__ W, int rank, int colv, int nb,
                                           int lane, int vec) {
  if (vec) {
    const int r4 = rank >> 2, tot = nb * r4;
    for (int e0 = 0; e0 < tot; e0 += 64 * kFoldV) {
      float4 v[kFoldV];
      int at[kFoldV];
#pragma unroll
      for (int u = 0; u < kFoldV; ++u) {
        const int e = e0 + 64 * u + lane;
        const bool ok = e < tot;
        const int j = ok ? e / r4 : 0;
        const int c = e - j * r4;
        const int col = __shfl(colv, j & 63, 64);
        at[u] = ok ? j * S + 4 * c : -1;
        v[u] = ok ? *reinterpret_cast<const float4*>(W + (size_t)col * rank + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < kFoldV; ++u)
        if (at[u] >= 0) {
          float* d = panel + at[u];
          d[0] = v[u].x, d[1] = v[u].y, d[2] = v[u].z, d[3] = v[u].w;
        }
    }
    return;
  }
  for (int j = 0; j < nb; j += kFoldU) {
    float b[kFoldU][RL];
#pragma unroll
    for (int u = 0; u < kFoldU; ++u) {
      const bool ok = j + u < nb;
      const int col = ok ? __shfl(colv, (j + u) & 63, 64) : 0;
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        const int r = lane + 64 * q;
        b[u][q] = (ok && r < rank) ? W[(size_t)col * rank + r] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kFoldU; ++u)
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        const int r = lane + 64 * q;
        if (j + u < nb && r < rank) panel[(j + u) * S + r] = b[u][q];
      }
  }
}

// MODE 0: missing; 1: zero (KIND KL or EUC).  WG: the workgroup's four waves share the row.
template <int RL, int KIND, int MODE, bool WG>
__device__ __forceinline__ void fold_row(const FoldArgs& a, int row, float* lw, float* part, int lane, int wave) {
  constexpr bool kConstNum = MODE == 1 && KIND == NMFMU_BETA_EUC;   // num = sum v W[j]: no s, the same every iteration
  constexpr bool kNeedDen = MODE == 0;
  const int rank = a.rank, S = rank | 1, B = a.block;
  float* hs = lw;                          // 16-byte aligned: pass 1 reads it four at a time
  float* gns = hs + 64 * RL;
  float* gps = gns + B;
  float* panel = gps + B;
  const int r0 = __builtin_amdgcn_readfirstlane(a.rowptr[row]);
  const int r1 = __builtin_amdgcn_readfirstlane(a.rowptr[row + 1]);
  int e0 = r0, e1 = r1;
  if constexpr (WG) {
    const int per = (r1 - r0 + kFoldWaves - 1) / kFoldWaves;
    e0 = min(r1, r0 + wave * per);
    e1 = min(r1, e0 + per);
  }
  const bool resident = e1 - e0 <= B;     // a single block: staged once

  float h[RL];
  load_row<RL>(h, a.H, row, rank, lane);
#pragma unroll
  for (int q = 0; q < RL; ++q) hs[lane + 64 * q] = h[q];

  int colv = 0;
  float vv = 0.f;
  auto load_entries = [&](int base, int nb) {
    colv = lane < nb ? a.colidx[base + lane] : 0;
    vv = lane < nb ? a.vals[base + lane] : 0.f;
  };
  // num / den += the block's terms, entries in storage order
  auto pass2 = [&](float (&an)[RL], float (&ad)[RL], int nb) {
#pragma unroll 8      // eight entries' LDS reads in flight; the chains stay j-ordered
    for (int j = 0; j < nb; ++j) {
      const float gn = gns[j];
      const float gp = kNeedDen ? gps[j] : 0.f;
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        const int r = lane + 64 * q;
        const float w = r < rank ? panel[j * S + r] : 0.f;
        an[q] = fmaf(gn, w, an[q]);
        if constexpr (kNeedDen) ad[q] = fmaf(gp, w, ad[q]);
      }
    }
  };
  auto block_terms = [&](float (&an)[RL], float (&ad)[RL], int nb) {
    if (lane < nb) {
      float gn = vv, gp = 0.f;
      if constexpr (!kConstNum) {
        const float* wr = panel + lane * S;
        float s = 0.f;
        int r = 0;
#pragma unroll 4
        for (; r + 3 < rank; r += 4) {       // (the chain is r-ordered either way)
          const float4 hv = *reinterpret_cast<const float4*>(hs + r);
          s = fmaf(hv.x, wr[r], s);
          s = fmaf(hv.y, wr[r + 1], s);
          s = fmaf(hv.z, wr[r + 2], s);
          s = fmaf(hv.w, wr[r + 3], s);
        }
        for (; r < rank; ++r) s = fmaf(hs[r], wr[r], s);
        fold_g<KIND>(vv, s, a.beta, gn, gp);
      }
      gns[lane] = gn;
      if constexpr (kNeedDen) gps[lane] = gp;
    }
    __builtin_amdgcn_wave_barrier();
    pass2(an, ad, nb);
    __builtin_amdgcn_wave_barrier();
  };
  // the wave's range, block by block
  auto range_terms = [&](float (&an)[RL], float (&ad)[RL]) {
#pragma unroll
    for (int q = 0; q < RL; ++q) an[q] = ad[q] = 0.f;
    if (resident) {
      block_terms(an, ad, e1 - e0);
    } else {
      for (int base = e0; base < e1; base += B) {
        const int nb = min(B, e1 - base);
        load_entries(base, nb);
        fold_stage<RL>(panel, S, a.W, rank, colv, nb, lane, a.vec);
        __builtin_amdgcn_wave_barrier();
        block_terms(an, ad, nb);
      }
    }
  };
  // the four waves' partials added in wave order; every wave ends with the same bits
  auto combine = [&](float (&an)[RL], float (&ad)[RL]) {
    if constexpr (WG) {
      float* mine = part + wave * (2 * 64 * RL);
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        mine[lane + 64 * q] = an[q];
        mine[64 * RL + lane + 64 * q] = ad[q];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        an[q] = part[lane + 64 * q];
        ad[q] = part[64 * RL + lane + 64 * q];
      }
      for (int w = 1; w < kFoldWaves; ++w)
#pragma unroll
        for (int q = 0; q < RL; ++q) {
          an[q] += part[w * (2 * 64 * RL) + lane + 64 * q];
          ad[q] += part[w * (2 * 64 * RL) + 64 * RL + lane + 64 * q];
        }
      __syncthreads();
    }
  };

  if (resident && e1 > e0) {
    load_entries(e0, e1 - e0);
    fold_stage<RL>(panel, S, a.W, rank, colv, e1 - e0, lane, a.vec);
  }
  __builtin_amdgcn_wave_barrier();

  float an[RL], ad[RL];
  if constexpr (kConstNum) {
    range_terms(an, ad);
    combine(an, ad);
  }
  int k = 0;
  while (k < a.max_iter) {
    if constexpr (!kConstNum) {
      range_terms(an, ad);
      combine(an, ad);
    }
    float dmax = 0.f, hmax = 0.f;
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      float hn = 0.f;
      if (r < rank) {
        const float f = h[q];
        const float neg = fmaxf(an[q], 0.f) + kEps;             // nmf.py:78
        float pos;
        if constexpr (MODE == 0) {
          pos = fmaxf(ad[q], 0.f) + kEps;                       // nmf.py:83
        } else if constexpr (KIND == NMFMU_BETA_KL) {
          pos = a.aux[r];                                       // nmf.py:128-131: the column sums as they are
        } else {
          float d = 0.f;                                        // h . G[:, r], q-ordered
          for (int t = 0; t < rank; ++t) d = fmaf(hs[t], a.aux[(size_t)t * rank + r], d);
          pos = fmaxf(d, 0.f) + kEps;
        }
        if (a.l1 > 0.f) pos += a.l1;
        if (a.l2 > 0.f) pos += a.l2 * f;
        float mult = neg / pos;
        if (a.gamma != 1.f) mult = powf(mult, a.gamma);
        hn = f * mult;
        dmax = fmaxf(dmax, fabsf(__fsub_rn(hn, f)));    // the rounded h_k minus h_{k-1}: never fused with f * mult
        hmax = fmaxf(hmax, hn);
      }
      h[q] = hn;
    }
    __builtin_amdgcn_wave_barrier();      // the Gram chain above read the old hs
#pragma unroll
    for (int q = 0; q < RL; ++q) hs[lane + 64 * q] = h[q];
    __builtin_amdgcn_wave_barrier();
    ++k;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
      hmax = fmaxf(hmax, __shfl_xor(hmax, o, 64));
    }
    if (a.tol > 0.f && dmax <= a.tol * hmax) break;
  }
  if (!WG || wave == 0) {
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      if (r < rank) a.H[(size_t)row * rank + r] = h[q];
    }
    if (a.n_iter && lane == 0) a.n_iter[row] = k;
  }
}

// A workgroup takes four rows of the order: first its long rows, one after the other with all four waves, then its short
// rows, one per wave.  (Every decision before a barrier is a function of the counts: uniform over the workgroup.)
template <int RL, int KIND, int MODE>
__global__ void __launch_bounds__(256) fold_in_kernel(FoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* lw = lds + wave * a.per_wave;
  float* part = lds + kFoldWaves * a.per_wave;
  int mine = -1;
  for (int i = 0; i < kFoldWaves; ++i) {
    const int at = blockIdx.x * kFoldWaves + i;
    if (at >= a.n_rows) break;
    const int row = a.order ? a.order[at] : at;
    const int cnt = a.rowptr[row + 1] - a.rowptr[row];
    if (cnt > a.long_rows) fold_row<RL, KIND, MODE, true>(a, row, lw, part, lane, wave);
    else if (i == wave) mine = row;
  }
  if (mine >= 0) fold_row<RL, KIND, MODE, false>(a, mine, lw, part, lane, wave);
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
int fold_rl(int rank) {
  const int r_pad = nmfmu_pad_rank(rank);
  return r_pad <= 64 ? 1 : (r_pad == 128 ? 2 : 4);
}

// the largest block the LDS holds: four waves' regions and the long rows' 4 x [num | den] partials
int fold_block_cap(int rank) {
  const int rl = fold_rl(rank);
  const int per = (kFoldLdsFloats - kFoldWaves * 2 * 64 * rl) / kFoldWaves - 64 * rl - 4;
  const int b = per / ((rank | 1) + 2);
  return b < 1 ? 1 : (b > 64 ? 64 : b);
}
}  // namespace

extern "C" {

int nmfmu_fold_in_block(int rank) {
  if (rank <= 0 || rank > 256) return 0;
  return fold_block_cap(rank);
}

int nmfmu_fold_in(const int32_t* rowptr, const int32_t* colidx, const float* vals, int n_rows, float* H, const float* W,
                  int n_cols, int rank, float beta, int mode, const float* aux, float l1, float l2, float gamma,
                  int max_iter, float tol, int32_t* n_iter_rows, const int32_t* order, int block, int long_rows,
                  void* stream) {
  if (!rowptr || !colidx || !vals || !H || !W || H == W) return NMFMU_ERR_ARG;
  if (rank <= 0 || n_rows < 0 || n_cols <= 0 || max_iter < 0 || !(tol >= 0.f) || block < 0 || long_rows < 0)
    return NMFMU_ERR_ARG;
  if (mode != NMFMU_FOLD_MISSING && mode != NMFMU_FOLD_ZERO) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  const int kind = nmfmu_beta_kind(beta);
  if (mode == NMFMU_FOLD_ZERO) {
    if (kind != NMFMU_BETA_KL && kind != NMFMU_BETA_EUC) return NMFMU_ERR_UNSUPPORTED;
    if (!aux) return NMFMU_ERR_ARG;
  }
  if (n_rows == 0 || max_iter == 0) return NMFMU_OK;

  const int rl = fold_rl(rank);
  const int cap = fold_block_cap(rank);
  FoldArgs a;
  a.rowptr = rowptr, a.colidx = colidx, a.vals = vals, a.order = order, a.H = H, a.W = W, a.aux = aux;
  a.n_iter = n_iter_rows;
  a.n_rows = n_rows, a.rank = rank, a.max_iter = max_iter;
  a.block = block == 0 ? cap : (block < cap ? block : cap);
  a.long_rows = long_rows == 0 ? cap : long_rows;      // what one wave keeps resident; a function of the rank alone
  a.per_wave = fold_per_wave(rank, a.block, rl);
  a.beta = beta, a.l1 = l1, a.l2 = l2, a.gamma = gamma, a.tol = tol;
  a.vec = (rank & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
  const size_t lds_bytes = (size_t)(kFoldWaves * a.per_wave + kFoldWaves * 2 * 64 * rl) * sizeof(float);
  if (lds_bytes > (size_t)kFoldLdsFloats * sizeof(float)) return NMFMU_ERR_ARG;   // (fold_block_cap rules it out)
  const dim3 grid((n_rows + kFoldWaves - 1) / kFoldWaves), blk(256);
  for_rl(nmfmu_pad_rank(rank), [&](auto rlc) {
    constexpr int RL = decltype(rlc)::value;
    if (mode == NMFMU_FOLD_MISSING) {
      for_kind(kind, [&](auto k) {
        hipLaunchKernelGGL((fold_in_kernel<RL, decltype(k)::value, 0>), grid, blk, lds_bytes, S(stream), a);
      });
    } else if (kind == NMFMU_BETA_KL) {
      hipLaunchKernelGGL((fold_in_kernel<RL, NMFMU_BETA_KL, 1>), grid, blk, lds_bytes, S(stream), a);
    } else {
      hipLaunchKernelGGL((fold_in_kernel<RL, NMFMU_BETA_EUC, 1>), grid, blk, lds_bytes, S(stream), a);
    }
  });
  return (int)hipGetLastError();
}

}  // extern "C"
