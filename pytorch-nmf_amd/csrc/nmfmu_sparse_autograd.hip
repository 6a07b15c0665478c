// Autograd on sparse-COO targets: the scalar V_norm + pos - neg of the reference's sparse path (nmf.py:162-181, 617-638)
// and its gradients with respect to both factors, beta in {1, 2}.
//
// The sparse MU kernels (nmfmu_sparse.hip) give one wave a whole owner row: a target whose row lengths are skewed -- a
// few rows with thousands of entries beside a median of tens -- then runs as long as its longest row.  These kernels are
// built on SEGMENTS instead: the host cuts every CSR row (H side, forward) and every CSC column (W side) into runs of at
// most `chunk` stored entries (torchnmf_amd/sparse_autograd.py: plan_segments) and one wave takes one segment.
//
//   seg   : int32 [n_seg][4] = (owner row, p_begin, p_end, slot) in row order.  slot < 0: the row's only segment (an
//           empty row has one empty segment, so every owner row is written by exactly one wave); slot >= 0: the row is
//           split and this segment's partial row goes to ws[slot][r_pad] (slots of a row are consecutive, in order)
//   multi : int32 [n_multi][3] = (owner row, first slot, segments) of the split rows
//
// forward : s[p] = <owner[row], panel[col[p]]> (fixed-order butterfly), the data term v log(s + eps) | v s summed in
//           double per lane (each lane owns every 64th entry of its segment), per wave (fixed-order butterfly), per workgroup
//           and then in block order; s is stored in CSR order on request (beta == 1
//           with a gradient wanted: the backward then holds no dot product and no cross-lane reduction)
// backward: acc[:] = sum over the segment, in storage order, of g * panel[idx[p]][:], g = v / (s + eps) | v.  A whole
//           row stores up * (pos - acc) directly; a split row stores acc with plain stores and the finishing kernel
//           adds the row's partials in segment order before the same epilogue.  No atomics, no fences: a repeated call
//           is bitwise identical.  pos: a broadcast vector [rank] (beta == 1: the panel's column sums) or a plane
//           [rows][r_pad] (beta == 2: owner @ panel^T panel, nmfmu_rowmat's output).
// Every padded rank column of `out` and of the used part of `ws` is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"

namespace nmfmu {

constexpr int kSpU = 4;   // stored entries in flight per wave and trip (as sp_partial_kernel)

template <int RL, bool KL>
__global__ void __launch_bounds__(256) sp_div_forward_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                             const int32_t* __restrict__ colidx,
                                                             const float* __restrict__ vals,
                                                             const float* __restrict__ owner,
                                                             const float* __restrict__ panel, int rank,
                                                             float* __restrict__ s_out, double* __restrict__ part) {
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
    // 64 entries per block: index and value are read once, one entry per lane (coalesced), and handed to the wave entry by
    // entry; each lane keeps the dot product of ITS entry, so the store of s, the logarithm and the double sum run once
    // per entry instead of once per entry and lane
    for (int base = p0; base < p1; base += 64) {
      const int pe = base + lane;
      const int colv = pe < p1 ? colidx[pe] : 0;
      const float vv = pe < p1 ? vals[pe] : 0.f;
      float sv = 1.f;
      const int cnt = min(64, p1 - base);
      for (int j = 0; j < cnt; j += kSpU) {
        float sdot[kSpU];
#pragma unroll
        for (int u = 0; u < kSpU; ++u) {
          const int col = j + u < cnt ? __shfl(colv, (j + u) & 63, 64) : 0;
          sdot[u] = 0.f;
#pragma unroll
          for (int q = 0; q < RL; ++q) {
            const int r = lane + 64 * q;
            sdot[u] += r < rank ? a[q] * panel[(size_t)col * rank + r] : 0.f;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)     // kSpU fixed-order butterflies, interleaved
#pragma unroll
          for (int u = 0; u < kSpU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
        for (int u = 0; u < kSpU; ++u)
          if (lane == j + u) sv = sdot[u];
      }
      if (pe < p1) {
        tot += KL ? (double)(vv * logf(sv + kEps)) : (double)(vv * sv);
        if (s_out) s_out[pe] = sv;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);   // the lanes' sums, fixed order
  if (lane == 0) red[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the block partials in block order (one workgroup, strided lanes, tree): the sum is a pure function of n
__global__ void __launch_bounds__(256) sp_div_reduce_kernel(const double* __restrict__ part, int n,
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
  if (threadIdx.x == 0) *out = red[0];
}

__device__ __forceinline__ float sp_div_pos(const float* __restrict__ pos, bool plane, int row, int r, int rank,
                                            int r_pad) {
  return plane ? pos[(size_t)row * r_pad + r] : (r < rank ? pos[r] : 0.f);
}

template <int RL, bool KL>
__global__ void __launch_bounds__(256) sp_div_backward_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                              const int32_t* __restrict__ idx,
                                                              const float* __restrict__ vals,
                                                              const int32_t* __restrict__ perm,
                                                              const float* __restrict__ s,
                                                              const float* __restrict__ panel, int rank,
                                                              const float* __restrict__ pos, int pos_plane,
                                                              const float* __restrict__ up, float* __restrict__ ws,
                                                              float* __restrict__ out, int r_pad) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_seg) return;
  // (wave-uniform by construction: one segment per wave)
  const int row = __builtin_amdgcn_readfirstlane(seg[4 * sg]), slot = __builtin_amdgcn_readfirstlane(seg[4 * sg + 3]);
  const int p0 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 1]), p1 = __builtin_amdgcn_readfirstlane(seg[4 * sg + 2]);
  float acc[RL];
#pragma unroll
  for (int q = 0; q < RL; ++q) acc[q] = 0.f;
  // 64 entries per block: index, value, perm and the saved s are read once, one entry per lane (coalesced but for s behind
  // perm), g is formed once per entry -- one divide, not 64 -- and (index, g) are handed to the wave entry by entry
  for (int base = p0; base < p1; base += 64) {
    const int pe = base + lane;
    const int colv = pe < p1 ? idx[pe] : 0;
    float gv = pe < p1 ? vals[pe] : 0.f;      // g = 0 contributes nothing (s + eps > 0)
    if constexpr (KL) {
      const float sv = pe < p1 ? s[perm ? perm[pe] : pe] : 1.f;
      gv = gv / (sv + kEps);
    }
    const int cnt = min(64, p1 - base);
    for (int j = 0; j < cnt; j += kSpU) {
      float g[kSpU], b[kSpU][RL];
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        const bool ok = j + u < cnt;
        const int col = ok ? __shfl(colv, (j + u) & 63, 64) : 0;
        g[u] = ok ? __shfl(gv, (j + u) & 63, 64) : 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) {
          const int r = lane + 64 * q;
          b[u][q] = r < rank ? panel[(size_t)col * rank + r] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kSpU; ++u)         // storage order
#pragma unroll
        for (int q = 0; q < RL; ++q) acc[q] += g[u] * b[u][q];
    }
  }
  if (slot >= 0) {
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      if (r < r_pad) ws[(size_t)slot * r_pad + r] = acc[q];
    }
    return;
  }
  const float upv = up[0];
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    if (r < r_pad)
      out[(size_t)row * r_pad + r] = r < rank ? upv * (sp_div_pos(pos, pos_plane != 0, row, r, rank, r_pad) - acc[q]) : 0.f;
  }
}

// one wave per split row: its partial rows added in segment order, then the epilogue of the kernel above
__global__ void __launch_bounds__(256) sp_div_finish_kernel(const int32_t* __restrict__ multi, int n_multi,
                                                            const float* __restrict__ ws, int rank,
                                                            const float* __restrict__ pos, int pos_plane,
                                                            const float* __restrict__ up, float* __restrict__ out,
                                                            int r_pad) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_multi) return;
  const int row = multi[3 * m], slot0 = multi[3 * m + 1], n = multi[3 * m + 2];
  const float upv = up[0];
  for (int r = lane; r < r_pad; r += 64) {
    float acc = ws[(size_t)slot0 * r_pad + r];
    for (int k = 1; k < n; ++k) acc += ws[(size_t)(slot0 + k) * r_pad + r];
    out[(size_t)row * r_pad + r] = r < rank ? upv * (sp_div_pos(pos, pos_plane != 0, row, r, rank, r_pad) - acc) : 0.f;
  }
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
}

extern "C" {

int64_t nmfmu_sp_div_backward_ws(int n_multi_segments, int r_pad) {
  if (n_multi_segments <= 0 || r_pad <= 0) return 0;
  return (int64_t)n_multi_segments * r_pad;
}

int nmfmu_sp_div_forward(const int32_t* seg, int n_seg, const int32_t* colidx, const float* vals, const float* owner,
                         const float* panel, int rank, float beta, float* s_out, double* part, double* out, void* stream) {
  if (!seg || !colidx || !vals || !owner || !panel || !part || !out || n_seg <= 0 || rank <= 0 || rank > 256)
    return NMFMU_ERR_ARG;
  const int kind = nmfmu_beta_kind(beta);
  if (kind != NMFMU_BETA_KL && kind != NMFMU_BETA_EUC) return NMFMU_ERR_UNSUPPORTED;
  const int nblk = (n_seg + 3) / 4;
  const int r_pad = nmfmu_pad_rank(rank);
#define L2(RLV, K)                                                                                                    \
  hipLaunchKernelGGL((sp_div_forward_kernel<RLV, K>), dim3(nblk), dim3(256), 0, S(stream), seg, n_seg, colidx, vals,   \
                     owner, panel, rank, s_out, part);
#define L(RLV) \
  if (kind == NMFMU_BETA_KL) { L2(RLV, true) } else { L2(RLV, false) }
  if (r_pad <= 64) { L(1) } else if (r_pad == 128) { L(2) } else { L(4) }
#undef L
#undef L2
  hipLaunchKernelGGL(sp_div_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, nblk, out);
  return (int)hipGetLastError();
}

int nmfmu_sp_div_backward(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                          const float* vals, const int32_t* perm, const float* s, const float* panel, int rank, float beta,
                          const float* pos, int pos_plane, const float* up, float* ws, float* out, int r_pad,
                          void* stream) {
  if (!seg || !idx || !vals || !panel || !pos || !up || !out || n_seg <= 0 || n_multi < 0 || rank <= 0 || rank > 256)
    return NMFMU_ERR_ARG;
  if (r_pad != nmfmu_pad_rank(rank) || (n_multi > 0 && (!multi || !ws))) return NMFMU_ERR_ARG;
  const int kind = nmfmu_beta_kind(beta);
  if (kind != NMFMU_BETA_KL && kind != NMFMU_BETA_EUC) return NMFMU_ERR_UNSUPPORTED;
  if (kind == NMFMU_BETA_KL && !s) return NMFMU_ERR_ARG;
  const int nblk = (n_seg + 3) / 4;
#define L2(RLV, K)                                                                                                    \
  hipLaunchKernelGGL((sp_div_backward_kernel<RLV, K>), dim3(nblk), dim3(256), 0, S(stream), seg, n_seg, idx, vals,     \
                     perm, s, panel, rank, pos, pos_plane, up, ws, out, r_pad);
#define L(RLV) \
  if (kind == NMFMU_BETA_KL) { L2(RLV, true) } else { L2(RLV, false) }
  if (r_pad <= 64) { L(1) } else if (r_pad == 128) { L(2) } else { L(4) }
#undef L
#undef L2
  if (n_multi > 0)
    hipLaunchKernelGGL(sp_div_finish_kernel, dim3((n_multi + 3) / 4), dim3(256), 0, S(stream), multi, n_multi, ws, rank,
                       pos, pos_plane, up, out, r_pad);
  return (int)hipGetLastError();
}

}  // extern "C"
