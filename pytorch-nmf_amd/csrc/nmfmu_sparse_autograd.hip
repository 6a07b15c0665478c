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
//
// The segment decode, the 64-entry blocks, the entry walk of the forward, the panel-row fetch of the backward, the ws slots
// and the double partials are the shared protocol of nmfmu_sparse_common.h; this file holds what the two divergences do
// with an entry and with a finished row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

template <int RL, bool KL>
__global__ void __launch_bounds__(256) sp_div_forward_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                             const int32_t* __restrict__ colidx,
                                                             const float* __restrict__ vals,
                                                             const float* __restrict__ owner,
                                                             const float* __restrict__ panel, int rank,
                                                             float* __restrict__ s_out, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  double tot = 0.0;
  if (sg < n_seg) {
    const Seg sgm = load_seg(seg, sg);
    float a[RL];
    load_row<RL>(a, owner, sgm.row, rank, lane);
    seg_entry_dots<RL>(sgm, colidx, vals, a, panel, rank, lane, [&](int pe, float v, float sv) {
      tot += KL ? (double)(v * logf(sv + kEps)) : (double)(v * sv);
      if (s_out) s_out[pe] = sv;
    });
  }
  store_lane_totals(tot, red, part);
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
  const Seg sgm = load_seg(seg, sg);
  const int p1 = sgm.p1;
  float acc[RL];
#pragma unroll
  for (int q = 0; q < RL; ++q) acc[q] = 0.f;
  // per block of 64 entries: value, perm and the saved s are read once, one entry per lane like the index (coalesced but
  // for s behind perm), g is formed once per entry -- one divide, not 64 -- and (index, g) are handed to the wave entry by
  // entry
  for (int base = sgm.p0; base < p1; base += 64) {
    const EntryBlock eb = load_block(idx, base, p1, lane);
    float gv = eb.pe < p1 ? vals[eb.pe] : 0.f;      // g = 0 contributes nothing (s + eps > 0)
    if constexpr (KL) {
      const float sv = eb.pe < p1 ? s[perm ? perm[eb.pe] : eb.pe] : 1.f;
      gv = gv / (sv + kEps);
    }
    for (int j = 0; j < eb.cnt; j += kSpU) {
      float g[kSpU], b[kSpU][RL];
      bool ok[kSpU];
      fetch_group<RL>(b, ok, eb, j, panel, rank, lane);
#pragma unroll
      for (int u = 0; u < kSpU; ++u) g[u] = ok[u] ? __shfl(gv, (j + u) & 63, 64) : 0.f;
#pragma unroll
      for (int u = 0; u < kSpU; ++u)         // storage order
#pragma unroll
        for (int q = 0; q < RL; ++q) acc[q] += g[u] * b[u][q];
    }
  }
  if (sgm.slot >= 0) {
    store_partial<1, RL>(ws, sgm.slot, 0, acc, r_pad, lane);
    return;
  }
  const int row = sgm.row;
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
  const Multi mu = load_multi(multi, m);
  const float upv = up[0];
  for (int r = lane; r < r_pad; r += 64) {
    float acc[1];
    sum_partials<1>(acc, ws, mu, r, r_pad);
    out[(size_t)mu.row * r_pad + r] =
        r < rank ? upv * (sp_div_pos(pos, pos_plane != 0, mu.row, r, rank, r_pad) - acc[0]) : 0.f;
  }
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
// f(std::true_type) for beta == 1, f(std::false_type) for beta == 2: the two kinds of sparse_beta_div
template <class F>
void for_kl(int kind, F&& f) {
  if (kind == NMFMU_BETA_KL) f(std::true_type{});
  else f(std::false_type{});
}
}  // namespace

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
  for_rl(nmfmu_pad_rank(rank), [&](auto rl) {
    for_kl(kind, [&](auto kl) {
      hipLaunchKernelGGL((sp_div_forward_kernel<decltype(rl)::value, decltype(kl)::value>), dim3(nblk), dim3(256), 0,
                         S(stream), seg, n_seg, colidx, vals, owner, panel, rank, s_out, part);
    });
  });
  hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, nblk, 0.0, 1.0, out);
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
  for_rl(r_pad, [&](auto rl) {
    for_kl(kind, [&](auto kl) {
      hipLaunchKernelGGL((sp_div_backward_kernel<decltype(rl)::value, decltype(kl)::value>), dim3(nblk), dim3(256), 0,
                         S(stream), seg, n_seg, idx, vals, perm, s, panel, rank, pos, pos_plane, up, ws, out, r_pad);
    });
  });
  if (n_multi > 0)
    hipLaunchKernelGGL(sp_div_finish_kernel, dim3((n_multi + 3) / 4), dim3(256), 0, S(stream), multi, n_multi, ws, rank,
                       pos, pos_plane, up, out, r_pad);
  return (int)hipGetLastError();
}

}  // extern "C"
