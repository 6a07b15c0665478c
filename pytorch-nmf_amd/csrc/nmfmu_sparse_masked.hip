// Missing-data NMF: a sparse target whose unstored entries are UNKNOWN, not zero.  Both contractions of the multiplicative
// update run over the stored set only, for every beta:
//
//   s_p      = <owner[row], panel[idx[p]]>                       (fixed-order xor butterfly)
//   num[row] = sum_p g_neg(v_p, s_p) * panel[idx[p]]             g_neg / g_pos: output_neg / output_pos of the reference's
//   den[row] = sum_p g_pos(s_p)      * panel[idx[p]]             _double_backward_update (nmf.py:61-74), beta == 1: g_pos = 1
//
// Work is cut into the SEGMENTS of nmfmu_sparse_autograd.hip (seg / multi lists, one wave per run of <= chunk stored entries,
// lanes across the rank, RL rank slots per lane).  Index and value of 64 entries are read once, one per lane, and handed to
// the wave entry by entry; kMaskU entries' panel rows are in flight per trip.  Entries accumulate in storage order.  A whole
// row is finished by the wave that formed its terms: it stores the two planes (terms) or applies nmf.py:78-92 in place to
// the owner's fp32 master (step) -- a row is read by its own wave only, the panel is the other factor.  A split row's
// segments store their partial [num | den] rows to ws[slot][2 r_pad] with plain stores and the finishing kernel adds them in
// segment order before the same epilogue.  No atomics: a repeated call is bitwise identical.
//
// The loss is the reference's metrics.beta_div(s, v, beta) over the two vectors of stored entries (metrics.py:22, 39, 57,
// 85-96): the kernel sums the terms that hold s in double (per lane, per wave, per workgroup, then in block order), the
// terms of v alone come from the host in float64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"

namespace nmfmu {

constexpr int kMaskU = 4;   // stored entries in flight per wave and trip (as sp_partial_kernel)

// (g_neg, g_pos) of one stored entry; s is the plain dot product
template <int KIND>
__device__ __forceinline__ void masked_g(float v, float s, float beta, float& gn, float& gp) {
  if constexpr (KIND == NMFMU_BETA_EUC) {
    gn = v, gp = s;                                   // nmf.py:62-63
  } else if constexpr (KIND == NMFMU_BETA_KL) {
    gn = v / (s + kEps), gp = 1.f;                    // nmf.py:65; the ones seed
  } else if constexpr (KIND == NMFMU_BETA_IS) {
    const float r = 1.f / (s + kEps);                 // nmf.py:68-70
    gp = r, gn = r * r * v;
  } else {
    const float se = s + kEps;                        // nmf.py:72-74
    const float p2 = exp2f((beta - 2.f) * log2f(se));
    gn = p2 * v, gp = p2 * se;
  }
}

struct MaskedApply {
  float l1, l2, gamma;
};

// nmf.py:78-92 on one element
__device__ __forceinline__ float masked_apply(float f, float num, float den, const MaskedApply& ap) {
  const float neg = fmaxf(num, 0.f) + kEps;
  float pos = fmaxf(den, 0.f) + kEps;
  if (ap.l1 > 0.f) pos += ap.l1;
  if (ap.l2 > 0.f) pos += ap.l2 * f;
  float mult = neg / pos;
  if (ap.gamma != 1.f) mult = powf(mult, ap.gamma);
  return f * mult;
}

// the shared epilogue of a finished row: r < r_pad, f = owner[row][r] (step only)
__device__ __forceinline__ void masked_finish(int step, float* owner, float* __restrict__ num, float* __restrict__ den,
                                              int row, int r, int rank, int r_pad, float f, float n, float d,
                                              const MaskedApply& ap) {
  if (step) {
    if (r < rank) owner[(size_t)row * rank + r] = masked_apply(f, n, d, ap);
  } else {
    num[(size_t)row * r_pad + r] = r < rank ? n : 0.f;
    den[(size_t)row * r_pad + r] = r < rank ? d : 0.f;
  }
}

template <int RL, int KIND>
__global__ void __launch_bounds__(256) sp_masked_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ vals,
                                                        float* owner, const float* __restrict__ panel, int rank, float beta,
                                                        float* __restrict__ ws, float* __restrict__ num,
                                                        float* __restrict__ den, int r_pad, int step, MaskedApply ap) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_seg) return;
  // (wave-uniform by construction: one segment per wave)
  const int row = __builtin_amdgcn_readfirstlane(seg[4 * sg]), slot = __builtin_amdgcn_readfirstlane(seg[4 * sg + 3]);
  const int p0 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 1]), p1 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 2]);
  float a[RL], an[RL], ad[RL];      // every kind reads s: EUC through g_pos = s
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    a[q] = r < rank ? owner[(size_t)row * rank + r] : 0.f;
    an[q] = ad[q] = 0.f;
  }
  for (int base = p0; base < p1; base += 64) {
    const int pe = base + lane;
    const int colv = pe < p1 ? idx[pe] : 0;
    const float vv = pe < p1 ? vals[pe] : 0.f;
    const int cnt = min(64, p1 - base);
    for (int j = 0; j < cnt; j += kMaskU) {
      float v[kMaskU], b[kMaskU][RL], sdot[kMaskU];
      bool ok[kMaskU];
#pragma unroll
      for (int u = 0; u < kMaskU; ++u) {
        ok[u] = j + u < cnt;
        const int col = ok[u] ? __shfl(colv, (j + u) & 63, 64) : 0;
        v[u] = __shfl(vv, (j + u) & 63, 64);
#pragma unroll
        for (int q = 0; q < RL; ++q) {
          const int r = lane + 64 * q;
          b[u][q] = (ok[u] && r < rank) ? panel[(size_t)col * rank + r] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kMaskU; ++u) {
        sdot[u] = 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) sdot[u] += a[q] * b[u][q];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)     // kMaskU fixed-order butterflies, interleaved
#pragma unroll
        for (int u = 0; u < kMaskU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
      for (int u = 0; u < kMaskU; ++u) {   // storage order; an entry past the end adds nothing
        float gn, gp;
        masked_g<KIND>(v[u], sdot[u], beta, gn, gp);
        gn = ok[u] ? gn : 0.f, gp = ok[u] ? gp : 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) {
          an[q] += gn * b[u][q];
          ad[q] += gp * b[u][q];
        }
      }
    }
  }
  if (slot >= 0) {
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      if (r < r_pad) {
        ws[(size_t)slot * 2 * r_pad + r] = an[q];
        ws[(size_t)slot * 2 * r_pad + r_pad + r] = ad[q];
      }
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    if (r < r_pad) masked_finish(step, owner, num, den, row, r, rank, r_pad, a[q], an[q], ad[q], ap);
  }
}

// one wave per split row: its partial rows added in segment order, then the epilogue of the kernel above
__global__ void __launch_bounds__(256) sp_masked_finish_kernel(const int32_t* __restrict__ multi, int n_multi,
                                                               const float* __restrict__ ws, float* owner,
                                                               float* __restrict__ num, float* __restrict__ den, int rank,
                                                               int r_pad, int step, MaskedApply ap) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_multi) return;
  const int row = multi[3 * m], slot0 = multi[3 * m + 1], n = multi[3 * m + 2];
  for (int r = lane; r < r_pad; r += 64) {
    float an = ws[(size_t)slot0 * 2 * r_pad + r], ad = ws[(size_t)slot0 * 2 * r_pad + r_pad + r];
    for (int k = 1; k < n; ++k) {
      an += ws[(size_t)(slot0 + k) * 2 * r_pad + r];
      ad += ws[(size_t)(slot0 + k) * 2 * r_pad + r_pad + r];
    }
    const float f = (step && r < rank) ? owner[(size_t)row * rank + r] : 0.f;
    masked_finish(step, owner, num, den, row, r, rank, r_pad, f, an, ad, ap);
  }
}

// the s-dependent term of metrics.beta_div at one stored entry, in double (see nmfmu_sp_masked_loss in include/nmfmu.h)
template <int KIND>
__device__ __forceinline__ double masked_loss_term(float v, float s, float beta) {
  if constexpr (KIND == NMFMU_BETA_EUC) {
    const float d = s - v;                            // metrics.py:39
    return (double)d * (double)d;
  } else if constexpr (KIND == NMFMU_BETA_KL) {
    return (double)s - (double)(v * logf(s + kEps));  // metrics.py:22
  } else if constexpr (KIND == NMFMU_BETA_IS) {
    const float se = s + kEps;                        // metrics.py:56-57
    return (double)((v + kEps) / se) + (double)logf(se);
  } else {
    const float se = s + kEps;                        // metrics.py:85-95
    const float vt = beta < 0.f ? v + kEps : v;
    const float pb1 = exp2f((beta - 1.f) * log2f(se));
    return (double)pb1 * ((double)(beta - 1.f) * (double)se - (double)beta * (double)vt);
  }
}

template <int RL, int KIND>
__global__ void __launch_bounds__(256) sp_masked_loss_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                             const int32_t* __restrict__ colidx,
                                                             const float* __restrict__ vals,
                                                             const float* __restrict__ owner,
                                                             const float* __restrict__ panel, int rank, float beta,
                                                             double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sg = blockIdx.x * 4 + w;
  double tot = 0.0;
  if (sg < n_seg) {
    // (wave-uniform by construction: one segment per wave)
    const int row = __builtin_amdgcn_readfirstlane(seg[4 * sg]);
    const int p0 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 1]), p1 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 2]);
    float a[RL];
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      a[q] = r < rank ? owner[(size_t)row * rank + r] : 0.f;
    }
    // each lane keeps the dot product of ITS entry of the 64: the logarithm and the double sum run once per entry
    for (int base = p0; base < p1; base += 64) {
      const int pe = base + lane;
      const int colv = pe < p1 ? colidx[pe] : 0;
      const float vv = pe < p1 ? vals[pe] : 0.f;
      float sv = 1.f;
      const int cnt = min(64, p1 - base);
      for (int j = 0; j < cnt; j += kMaskU) {
        float sdot[kMaskU];
#pragma unroll
        for (int u = 0; u < kMaskU; ++u) {
          const bool ok = j + u < cnt;
          const int col = ok ? __shfl(colv, (j + u) & 63, 64) : 0;
          sdot[u] = 0.f;
#pragma unroll
          for (int q = 0; q < RL; ++q) {
            const int r = lane + 64 * q;
            sdot[u] += (ok && r < rank) ? a[q] * panel[(size_t)col * rank + r] : 0.f;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
          for (int u = 0; u < kMaskU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
        for (int u = 0; u < kMaskU; ++u)
          if (lane == j + u) sv = sdot[u];
      }
      if (pe < p1) tot += masked_loss_term<KIND>(vv, sv, beta);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);   // the lanes' sums, fixed order
  if (lane == 0) red[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the block partials in block order (one workgroup, strided lanes, tree): *out = (add + sum) * mul
__global__ void __launch_bounds__(256) sp_masked_reduce_kernel(const double* __restrict__ part, int n, double add, double mul,
                                                               double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = (add + red[0]) * mul;
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// NMFMU_OK or the answer the three entries give before any device work
int masked_rank_check(int rank, int r_pad, bool has_r_pad) {
  if (rank <= 0) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (has_r_pad && r_pad != nmfmu_pad_rank(rank)) return NMFMU_ERR_ARG;
  return NMFMU_OK;
}

int masked_launch(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx, const float* vals,
                  float* owner, const float* panel, int rank, float beta, float* ws, float* num, float* den, int r_pad,
                  int step, MaskedApply ap, hipStream_t st) {
  const int kind = nmfmu_beta_kind(beta);
  const int nblk = (n_seg + 3) / 4;
#define L2(RLV, K)                                                                                                       \
  hipLaunchKernelGGL((sp_masked_kernel<RLV, K>), dim3(nblk), dim3(256), 0, st, seg, n_seg, idx, vals, owner, panel, rank, \
                     beta, ws, num, den, r_pad, step, ap);
#define L(RLV)                                                                           \
  switch (kind) {                                                                        \
    case NMFMU_BETA_KL: L2(RLV, NMFMU_BETA_KL) break;                                    \
    case NMFMU_BETA_EUC: L2(RLV, NMFMU_BETA_EUC) break;                                  \
    case NMFMU_BETA_IS: L2(RLV, NMFMU_BETA_IS) break;                                    \
    default: L2(RLV, NMFMU_BETA_GEN) break;                                              \
  }
  if (r_pad <= 64) { L(1) } else if (r_pad == 128) { L(2) } else { L(4) }
#undef L
#undef L2
  if (n_multi > 0)
    hipLaunchKernelGGL(sp_masked_finish_kernel, dim3((n_multi + 3) / 4), dim3(256), 0, st, multi, n_multi, ws, owner, num,
                       den, rank, r_pad, step, ap);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" {

int64_t nmfmu_sp_masked_ws(int n_multi_segments, int r_pad) {
  if (n_multi_segments <= 0 || r_pad <= 0) return 0;
  return (int64_t)n_multi_segments * 2 * r_pad;
}

int nmfmu_sp_masked_terms(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                          const float* vals, const float* owner, const float* panel, int rank, float beta, float* ws,
                          float* num, float* den, int r_pad, void* stream) {
  if (!seg || !idx || !vals || !owner || !panel || !num || !den || n_seg <= 0 || n_multi < 0) return NMFMU_ERR_ARG;
  if (n_multi > 0 && (!multi || !ws)) return NMFMU_ERR_ARG;
  if (const int rc = masked_rank_check(rank, r_pad, true)) return rc;
  return masked_launch(seg, n_seg, multi, n_multi, idx, vals, const_cast<float*>(owner), panel, rank, beta, ws, num, den,
                       r_pad, 0, MaskedApply{0.f, 0.f, 1.f}, S(stream));
}

int nmfmu_sp_masked_step(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                         const float* vals, float* owner, const float* panel, int rank, float beta, float l1, float l2,
                         float gamma, float* ws, int r_pad, void* stream) {
  if (!seg || !idx || !vals || !owner || !panel || owner == panel || n_seg <= 0 || n_multi < 0) return NMFMU_ERR_ARG;
  if (n_multi > 0 && (!multi || !ws)) return NMFMU_ERR_ARG;
  if (const int rc = masked_rank_check(rank, r_pad, true)) return rc;
  return masked_launch(seg, n_seg, multi, n_multi, idx, vals, owner, panel, rank, beta, ws, nullptr, nullptr, r_pad, 1,
                       MaskedApply{l1, l2, gamma}, S(stream));
}

int nmfmu_sp_masked_loss(const int32_t* seg, int n_seg, const int32_t* colidx, const float* vals, const float* owner,
                         const float* panel, int rank, float beta, double v_term, double* part, double* out, void* stream) {
  if (!seg || !colidx || !vals || !owner || !panel || !part || !out || n_seg <= 0) return NMFMU_ERR_ARG;
  if (const int rc = masked_rank_check(rank, 0, false)) return rc;
  const int kind = nmfmu_beta_kind(beta);
  const int nblk = (n_seg + 3) / 4;
  const int r_pad = nmfmu_pad_rank(rank);
#define L2(RLV, K)                                                                                                      \
  hipLaunchKernelGGL((sp_masked_loss_kernel<RLV, K>), dim3(nblk), dim3(256), 0, S(stream), seg, n_seg, colidx, vals,     \
                     owner, panel, rank, beta, part);
#define L(RLV)                                                                           \
  switch (kind) {                                                                        \
    case NMFMU_BETA_KL: L2(RLV, NMFMU_BETA_KL) break;                                    \
    case NMFMU_BETA_EUC: L2(RLV, NMFMU_BETA_EUC) break;                                  \
    case NMFMU_BETA_IS: L2(RLV, NMFMU_BETA_IS) break;                                    \
    default: L2(RLV, NMFMU_BETA_GEN) break;                                              \
  }
  if (r_pad <= 64) { L(1) } else if (r_pad == 128) { L(2) } else { L(4) }
#undef L
#undef L2
  // metrics.py:39 halves the sum of squares; metrics.py:96 divides by beta (beta - 1)
  double mul = 1.0;
  if (kind == NMFMU_BETA_EUC) mul = 0.5;
  if (kind == NMFMU_BETA_GEN) mul = 1.0 / ((double)beta * ((double)beta - 1.0));
  hipLaunchKernelGGL(sp_masked_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, nblk, v_term, mul, out);
  return (int)hipGetLastError();
}

}  // extern "C"
