// Missing-data NMF: a sparse target whose unstored entries are UNKNOWN, not zero.  Both contractions of the multiplicative
// update run over the stored set only, for every beta:
//
//   s_p      = <owner[row], panel[idx[p]]>                       (fixed-order xor butterfly)
//   num[row] = sum_p g_neg(v_p, s_p) * panel[idx[p]]             g_neg / g_pos: output_neg / output_pos of the reference's
//   den[row] = sum_p g_pos(s_p)      * panel[idx[p]]             _double_backward_update (nmf.py:61-74), beta == 1: g_pos = 1
//
// Work is cut into SEGMENTS (seg / multi lists, one wave per run of <= chunk stored entries, lanes across the rank, RL rank
// slots per lane): the shared protocol of nmfmu_sparse_common.h, which also holds the 64-entry blocks, the panel-row fetch,
// the ws slots and the double partials.  Index and value of 64 entries are read once, one per lane, and handed to
// the wave entry by entry; kSpU entries' panel rows are in flight per trip.  Entries accumulate in storage order.  A whole
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
#include "nmfmu_mu_terms.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

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
  const Seg sgm = load_seg(seg, sg);
  const int row = sgm.row, p1 = sgm.p1;
  float a[RL], an[RL], ad[RL];      // every kind reads s: EUC through g_pos = s
  load_row<RL>(a, owner, row, rank, lane);
#pragma unroll
  for (int q = 0; q < RL; ++q) an[q] = ad[q] = 0.f;
  for (int base = sgm.p0; base < p1; base += 64) {
    const EntryBlock eb = load_block(idx, base, p1, lane);
    const float vv = eb.pe < p1 ? vals[eb.pe] : 0.f;
    for (int j = 0; j < eb.cnt; j += kSpU) {
      float v[kSpU], b[kSpU][RL], sdot[kSpU];
      bool ok[kSpU];
      fetch_group<RL>(b, ok, eb, j, panel, rank, lane);
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        v[u] = __shfl(vv, (j + u) & 63, 64);
        sdot[u] = 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) sdot[u] += a[q] * b[u][q];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)     // kSpU fixed-order butterflies, interleaved
#pragma unroll
        for (int u = 0; u < kSpU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {   // storage order; an entry past the end adds nothing
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
  if (sgm.slot >= 0) {
    store_partial<2, RL>(ws, sgm.slot, 0, an, r_pad, lane);
    store_partial<2, RL>(ws, sgm.slot, 1, ad, r_pad, lane);
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
  const Multi mu = load_multi(multi, m);
  for (int r = lane; r < r_pad; r += 64) {
    float nd[2];      // [num | den]
    sum_partials<2>(nd, ws, mu, r, r_pad);
    const float f = (step && r < rank) ? owner[(size_t)mu.row * rank + r] : 0.f;
    masked_finish(step, owner, num, den, mu.row, r, rank, r_pad, f, nd[0], nd[1], ap);
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
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  double tot = 0.0;
  if (sg < n_seg) {
    const Seg sgm = load_seg(seg, sg);
    float a[RL];
    load_row<RL>(a, owner, sgm.row, rank, lane);
    seg_entry_dots<RL>(sgm, colidx, vals, a, panel, rank, lane,
                       [&](int, float v, float sv) { tot += masked_loss_term<KIND>(v, sv, beta); });
  }
  store_lane_totals(tot, red, part);
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
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
  for_rl(r_pad, [&](auto rl) {
    for_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((sp_masked_kernel<decltype(rl)::value, decltype(k)::value>), dim3(nblk), dim3(256), 0, st, seg,
                         n_seg, idx, vals, owner, panel, rank, beta, ws, num, den, r_pad, step, ap);
    });
  });
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
  for_rl(nmfmu_pad_rank(rank), [&](auto rl) {
    for_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((sp_masked_loss_kernel<decltype(rl)::value, decltype(k)::value>), dim3(nblk), dim3(256), 0,
                         S(stream), seg, n_seg, colidx, vals, owner, panel, rank, beta, part);
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
