// NTF on a sparse 3-way target: the multiplicative update of one mode and the loss over the STORED entries only.  Per mode the
// target is held sorted by (owner index, a, b) -- a, b the other two modes in ascending mode number -- as rowptr-cut
// segments, two int32 index arrays and the values in that order.  For a stored entry p of owner row i:
//
//   kr_p   = fl32(Pa[idx_a[p]][r] * Pb[idx_b[p]][r])          the Khatri-Rao row: registers only, it never exists in memory
//   s_p    = <F[i], kr_p>                                      lane-private chain over the RL slots, then the xor butterfly
//   num[i] = sum_p g_neg(v_p, s_p) * kr_p                      storage order
//   den[i] = sum_p g_pos(s_p) * kr_p                           unstored = 'missing'
//
// Under unstored = 'zero' (beta in {1, 2}) the denominator sums over EVERY entry of the tensor, so it factorises and comes in
// as `pos`: the vector colsum(Pa) o colsum(Pb) (beta 1, plane 0) or the plane F (Gram(Pa) o Gram(Pb)) (beta 2, plane 1); at
// beta 2 g_neg = v and the dot product is not formed at all.
//
// The walk is the protocol of nmfmu_sparse_common.h (a wave per segment, lanes across the rank, 64 entries read once and
// handed round by __shfl, kSpU entries per trip, ws slots for split rows, double partials in a fixed order).  This file's own:
//
//   * two gathers per entry, multiplied on the way in: 2 kSpU independent panel-row loads are in flight per trip;
//   * a SHORT panel factor (the context mode of users x items x context: tens of rows, gathered once per entry) is copied
//     into LDS once per workgroup and that side's gather reads LDS.  Workgroups on that route are persistent: the grid is a
//     small multiple of the CU count and each workgroup takes a fixed contiguous run of segment quads, so the copy is paid
//     a few hundred times and not once per quad.  A segment is still one wave's work from its first entry to its last, and
//     an LDS row holds the bits of the memory row: the result does not depend on the route or on the grid;
//   * no matrix instructions: s_p contracts two gathered rows that no other entry shares, so an MFMA tile would carry one
//     useful row in sixteen.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

// LDS floats per staged panel.  Both panels may be staged: 2 * 7936 * 4 B = 63 488 B per workgroup, with the 32 B of the loss
// kernel's partials below the 64 KiB a launch may ask for without opting in; two workgroups take 127 040 B of the CU's
// 160 KiB (163 840 B), so at least two stay resident -- eight waves per CU to cover the gathers of the unstaged side.
constexpr int kNtfLdsFloats = 7936;
constexpr int kNtfWgPerCu = 2;       // persistent workgroups per CU on the staged route when both panels fill their budget;
constexpr int kNtfWgPerCuMax = 8;    // a smaller copy leaves room for more, up to the 32 waves per CU the unstaged route gets
constexpr int kNtfCuLdsBytes = 160 * 1024;

struct NtfArgs {
  const int32_t* seg;
  const int32_t *idx_a, *idx_b;
  const float* vals;
  float* owner;
  const float *pa, *pb;
  const float* pos;      // 'zero' only
  float *ws, *num, *den;
  double* part;          // loss only: one double per segment quad
  int n_seg, rows_a, rows_b, rank, r_pad, pos_plane, step, quads_per_wg;
  float beta;
  MaskedApply ap;
};

// ---- 64 entries of a segment, one per lane, with both panel indices -------------------------------------------------------------
struct EntryBlock2 {
  int pe, ia, ib, cnt;
};

__device__ __forceinline__ EntryBlock2 load_block2(const int32_t* idx_a, const int32_t* idx_b, int base, int p1, int lane) {
  const int pe = base + lane;
  return EntryBlock2{pe, pe < p1 ? idx_a[pe] : 0, pe < p1 ? idx_b[pe] : 0, min(64, p1 - base)};
}

// The Khatri-Rao rows of entries j .. j + kSpU - 1 of a block: all 2 kSpU RL loads are issued before the first product.  An
// entry past the end of the block fetches nothing and its kr is zero whatever row 0 of a panel holds.
template <int RL>
__device__ __forceinline__ void fetch_kr(float (&kr)[kSpU][RL], bool (&ok)[kSpU], const EntryBlock2& eb, int j,
                                         const float* pa, const float* pb, int rank, int lane) {
  float xa[kSpU][RL], xb[kSpU][RL];
#pragma unroll
  for (int u = 0; u < kSpU; ++u) {
    ok[u] = j + u < eb.cnt;
    const int ca = ok[u] ? __shfl(eb.ia, (j + u) & 63, 64) : 0;
    const int cb = ok[u] ? __shfl(eb.ib, (j + u) & 63, 64) : 0;
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      const bool m = ok[u] && r < rank;
      xa[u][q] = m ? pa[(size_t)ca * rank + r] : 0.f;
      xb[u][q] = m ? pb[(size_t)cb * rank + r] : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < kSpU; ++u)
#pragma unroll
    for (int q = 0; q < RL; ++q) kr[u][q] = xa[u][q] * xb[u][q];
}

// sdot[u] = <a, kr[u]>: the chain over the slots, then kSpU fixed-order butterflies, interleaved
template <int RL>
__device__ __forceinline__ void kr_dots(float (&sdot)[kSpU], const float (&a)[RL], const float (&kr)[kSpU][RL]) {
#pragma unroll
  for (int u = 0; u < kSpU; ++u) {
    sdot[u] = 0.f;
#pragma unroll
    for (int q = 0; q < RL; ++q) sdot[u] += a[q] * kr[u][q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int u = 0; u < kSpU; ++u) sdot[u] += __shfl_xor(sdot[u], o, 64);
}

// ST: bit 0 -- Pa is staged, bit 1 -- Pb is staged.  Every thread of the workgroup calls; returns the two gather sources.
template <int ST>
__device__ __forceinline__ void stage_panels(const NtfArgs& a, float* lds, const float*& pa, const float*& pb) {
  pa = a.pa, pb = a.pb;
  if constexpr (ST != 0) {
    float* lb = lds;
    if constexpr ((ST & 1) != 0) {
      const int n = a.rows_a * a.rank;
      for (int i = threadIdx.x; i < n; i += 256) lds[i] = a.pa[i];
      pa = lds, lb = lds + n;
    }
    if constexpr ((ST & 2) != 0) {
      const int n = a.rows_b * a.rank;
      for (int i = threadIdx.x; i < n; i += 256) lb[i] = a.pb[i];
      pb = lb;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float ntf_pos(const NtfArgs& a, int row, int r) {
  return a.pos_plane ? a.pos[(size_t)row * a.r_pad + r] : (r < a.rank ? a.pos[r] : 0.f);
}

template <int RL, int KIND, bool ZERO, int ST>
__global__ void __launch_bounds__(256) sp_ntf_kernel(NtfArgs a) {
  extern __shared__ float ntf_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float *pa, *pb;
  stage_panels<ST>(a, ntf_lds, pa, pb);
  const int n_quad = (a.n_seg + 3) / 4;
  const int q0 = blockIdx.x * a.quads_per_wg, q1 = min(q0 + a.quads_per_wg, n_quad);
  const int rank = a.rank;
  for (int qd = q0; qd < q1; ++qd) {
    const int sg = qd * 4 + w;
    if (sg >= a.n_seg) break;      // the last quad only; nothing below meets the other waves
    const Seg sgm = load_seg(a.seg, sg);
    const int row = sgm.row, p1 = sgm.p1;
    float f[RL], an[RL], ad[RL];
    load_row<RL>(f, a.owner, row, rank, lane);
#pragma unroll
    for (int q = 0; q < RL; ++q) an[q] = ad[q] = 0.f;
    for (int base = sgm.p0; base < p1; base += 64) {
      const EntryBlock2 eb = load_block2(a.idx_a, a.idx_b, base, p1, lane);
      const float vv = eb.pe < p1 ? a.vals[eb.pe] : 0.f;
      for (int j = 0; j < eb.cnt; j += kSpU) {
        float kr[kSpU][RL], sdot[kSpU];
        bool ok[kSpU];
        fetch_kr<RL>(kr, ok, eb, j, pa, pb, rank, lane);
        if constexpr (!(ZERO && KIND == NMFMU_BETA_EUC)) kr_dots<RL>(sdot, f, kr);
#pragma unroll
        for (int u = 0; u < kSpU; ++u) {   // storage order; an entry past the end adds nothing
          const float v = __shfl(vv, (j + u) & 63, 64);
          float gn, gp = 0.f;
          if constexpr (ZERO && KIND == NMFMU_BETA_EUC) gn = v;
          else masked_g<KIND>(v, sdot[u], a.beta, gn, gp);
          gn = ok[u] ? gn : 0.f, gp = ok[u] ? gp : 0.f;
#pragma unroll
          for (int q = 0; q < RL; ++q) {
            an[q] += gn * kr[u][q];
            if constexpr (!ZERO) ad[q] += gp * kr[u][q];
          }
        }
      }
    }
    if (sgm.slot >= 0) {
      store_partial<ZERO ? 1 : 2, RL>(a.ws, sgm.slot, 0, an, a.r_pad, lane);
      if constexpr (!ZERO) store_partial<2, RL>(a.ws, sgm.slot, 1, ad, a.r_pad, lane);
      continue;
    }
#pragma unroll
    for (int q = 0; q < RL; ++q) {
      const int r = lane + 64 * q;
      if (r < a.r_pad)
        masked_finish(a.step, a.owner, a.num, a.den, row, r, rank, a.r_pad, f[q], an[q], ZERO ? ntf_pos(a, row, r) : ad[q],
                      a.ap);
    }
  }
}

// one wave per split row: its partial rows added in segment order, then the epilogue of the kernel above
template <bool ZERO>
__global__ void __launch_bounds__(256) sp_ntf_finish_kernel(const int32_t* __restrict__ multi, int n_multi, NtfArgs a) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_multi) return;
  const Multi mu = load_multi(multi, m);
  for (int r = lane; r < a.r_pad; r += 64) {
    float nd[ZERO ? 1 : 2];      // [num | den]
    sum_partials<ZERO ? 1 : 2>(nd, a.ws, mu, r, a.r_pad);
    float d;
    if constexpr (ZERO) d = ntf_pos(a, mu.row, r);
    else d = nd[1];
    const float f = (a.step && r < a.rank) ? a.owner[(size_t)mu.row * a.rank + r] : 0.f;
    masked_finish(a.step, a.owner, a.num, a.den, mu.row, r, a.rank, a.r_pad, f, nd[0], d, a.ap);
  }
}

// The loss from mode 0's list.  Each lane keeps the dot product of ITS entry of the 64 (formed exactly as in the step kernel),
// so the logarithm and the double sum run once per entry.  One double per segment quad, whatever workgroup took the quad.
template <int RL, int KIND, bool ZERO, int ST>
__global__ void __launch_bounds__(256) sp_ntf_loss_kernel(NtfArgs a) {
  extern __shared__ float ntf_lds[];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float *pa, *pb;
  stage_panels<ST>(a, ntf_lds, pa, pb);
  const int n_quad = (a.n_seg + 3) / 4;
  const int q0 = blockIdx.x * a.quads_per_wg, q1 = min(q0 + a.quads_per_wg, n_quad);
  for (int qd = q0; qd < q1; ++qd) {
    const int sg = qd * 4 + w;
    double tot = 0.0;
    if (sg < a.n_seg) {
      const Seg sgm = load_seg(a.seg, sg);
      float f[RL];
      load_row<RL>(f, a.owner, sgm.row, a.rank, lane);
      for (int base = sgm.p0; base < sgm.p1; base += 64) {
        const EntryBlock2 eb = load_block2(a.idx_a, a.idx_b, base, sgm.p1, lane);
        const float vv = eb.pe < sgm.p1 ? a.vals[eb.pe] : 0.f;
        float sv = 1.f;   // a lane without an entry never uses sv; 1 keeps it finite all the same
        for (int j = 0; j < eb.cnt; j += kSpU) {
          float kr[kSpU][RL], sdot[kSpU];
          bool ok[kSpU];
          fetch_kr<RL>(kr, ok, eb, j, pa, pb, a.rank, lane);
          kr_dots<RL>(sdot, f, kr);
#pragma unroll
          for (int u = 0; u < kSpU; ++u)
            if (lane == j + u) sv = sdot[u];
        }
        if (eb.pe < sgm.p1) {
          if constexpr (!ZERO) tot += masked_loss_term<KIND>(vv, sv, a.beta);
          else if constexpr (KIND == NMFMU_BETA_KL) tot += (double)(vv * logf(sv + kEps));
          else tot += (double)(vv * sv);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane == 0) red[w] = tot;
    __syncthreads();
    if (threadIdx.x == 0) a.part[qd] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();      // red is the next quad's as well
  }
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
// which panels a launch stages (bit 0: Pa, bit 1: Pb): a pure function of the counts.  The library's own rule (stage 0)
// stages nothing: in every measured case (a 24-row panel at rank 64, 10 M entries) the short panel's rows
// are served from cache and the persistent grid was 10 - 21 % slower than one quad per workgroup, never faster
int ntf_stage_mask(int rows_a, int rows_b, int rank, int stage) {
  if (stage != 2) return 0;
  const int cap = nmfmu_sp_ntf_lds_rows(rank);
  return (rows_a <= cap ? 1 : 0) | (rows_b <= cap ? 2 : 0);
}

// f(std::integral_constant<int, ST>)
template <class F>
void for_st(int st, F&& f) {
  switch (st) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
  }
}

// f(kind, zero) over the six served combinations
template <class F>
void for_kind_zero(int kind, bool zero, F&& f) {
  if (!zero) {
    for_kind(kind, [&](auto k) { f(k, std::false_type{}); });
  } else if (kind == NMFMU_BETA_KL) {
    f(std::integral_constant<int, NMFMU_BETA_KL>{}, std::true_type{});
  } else {
    f(std::integral_constant<int, NMFMU_BETA_EUC>{}, std::true_type{});
  }
}

// grid and LDS bytes of a walk over n_seg segments; unstaged: one quad per workgroup, staged: persistent workgroups
int ntf_grid(NtfArgs& a, int st, unsigned& grid, size_t& lds) {
  const int n_quad = (a.n_seg + 3) / 4;
  lds = ((st & 1 ? (size_t)a.rows_a * a.rank : 0) + (st & 2 ? (size_t)a.rows_b * a.rank : 0)) * sizeof(float);
  a.quads_per_wg = 1;
  if (st != 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return (int)hipErrorInvalidDevice;
    const int fit = (int)(kNtfCuLdsBytes / lds);
    const int cap = (fit < kNtfWgPerCu ? kNtfWgPerCu : fit > kNtfWgPerCuMax ? kNtfWgPerCuMax : fit) * cus;
    a.quads_per_wg = (n_quad + cap - 1) / cap;
  }
  grid = (unsigned)((n_quad + a.quads_per_wg - 1) / a.quads_per_wg);
  return NMFMU_OK;
}

// NMFMU_OK or the answer every entry gives before any device work
int ntf_check(const void* seg, int n_seg, const void* idx_a, const void* idx_b, const void* vals, int nnz, const void* owner,
              const void* pa, int rows_a, const void* pb, int rows_b, int rank, float beta, int zero, int stage) {
  if (!seg || !idx_a || !idx_b || !vals || !owner || !pa || !pb || n_seg <= 0 || nnz < 0 || rows_a <= 0 || rows_b <= 0)
    return NMFMU_ERR_ARG;
  if (rank <= 0 || stage < 0 || stage > 2 || (zero != 0 && zero != 1)) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (zero && beta != 1.f && beta != 2.f) return NMFMU_ERR_UNSUPPORTED;
  return NMFMU_OK;
}

int ntf_launch(NtfArgs a, const int32_t* multi, int n_multi, bool zero, int stage, hipStream_t st) {
  const int mask = ntf_stage_mask(a.rows_a, a.rows_b, a.rank, stage);
  unsigned grid;
  size_t lds;
  if (const int rc = ntf_grid(a, mask, grid, lds)) return rc;
  for_rl(a.r_pad, [&](auto rl) {
    for_kind_zero(nmfmu_beta_kind(a.beta), zero, [&](auto k, auto z) {
      for_st(mask, [&](auto s) {
        hipLaunchKernelGGL((sp_ntf_kernel<decltype(rl)::value, decltype(k)::value, decltype(z)::value, decltype(s)::value>),
                           dim3(grid), dim3(256), lds, st, a);
      });
    });
  });
  if (n_multi > 0) {
    if (zero) hipLaunchKernelGGL(sp_ntf_finish_kernel<true>, dim3((n_multi + 3) / 4), dim3(256), 0, st, multi, n_multi, a);
    else hipLaunchKernelGGL(sp_ntf_finish_kernel<false>, dim3((n_multi + 3) / 4), dim3(256), 0, st, multi, n_multi, a);
  }
  return (int)hipGetLastError();
}

NtfArgs ntf_args(const int32_t* seg, int n_seg, const int32_t* idx_a, const int32_t* idx_b, const float* vals, float* owner,
                 const float* pa, int rows_a, const float* pb, int rows_b, int rank, float beta) {
  NtfArgs a{};
  a.seg = seg, a.n_seg = n_seg, a.idx_a = idx_a, a.idx_b = idx_b, a.vals = vals, a.owner = owner;
  a.pa = pa, a.rows_a = rows_a, a.pb = pb, a.rows_b = rows_b, a.rank = rank, a.beta = beta;
  a.r_pad = nmfmu_pad_rank(rank);
  a.ap = MaskedApply{0.f, 0.f, 1.f};
  return a;
}
}  // namespace

extern "C" {

int nmfmu_sp_ntf_lds_rows(int rank) {
  if (rank <= 0 || rank > 256) return 0;
  return kNtfLdsFloats / rank;
}

int64_t nmfmu_sp_ntf_ws(int n_multi_segments, int r_pad) {
  if (n_multi_segments <= 0 || r_pad <= 0) return 0;
  return (int64_t)n_multi_segments * 2 * r_pad;
}

int nmfmu_sp_ntf_terms(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx_a,
                       const int32_t* idx_b, const float* vals, int nnz, const float* owner, const float* pa, int rows_a,
                       const float* pb, int rows_b, int rank, float beta, int zero, const float* pos, int pos_plane,
                       float* ws, float* num, float* den, int r_pad, int stage, void* stream) {
  if (const int rc = ntf_check(seg, n_seg, idx_a, idx_b, vals, nnz, owner, pa, rows_a, pb, rows_b, rank, beta, zero, stage))
    return rc;
  if (!num || !den || n_multi < 0 || (n_multi > 0 && (!multi || !ws)) || (zero && !pos) || r_pad != nmfmu_pad_rank(rank))
    return NMFMU_ERR_ARG;
  NtfArgs a = ntf_args(seg, n_seg, idx_a, idx_b, vals, const_cast<float*>(owner), pa, rows_a, pb, rows_b, rank, beta);
  a.pos = pos, a.pos_plane = pos_plane, a.ws = ws, a.num = num, a.den = den, a.step = 0;
  return ntf_launch(a, multi, n_multi, zero != 0, stage, S(stream));
}

int nmfmu_sp_ntf_step(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx_a,
                      const int32_t* idx_b, const float* vals, int nnz, float* owner, const float* pa, int rows_a,
                      const float* pb, int rows_b, int rank, float beta, int zero, const float* pos, int pos_plane, float l1,
                      float l2, float gamma, float* ws, int r_pad, int stage, void* stream) {
  if (const int rc = ntf_check(seg, n_seg, idx_a, idx_b, vals, nnz, owner, pa, rows_a, pb, rows_b, rank, beta, zero, stage))
    return rc;
  if (owner == pa || owner == pb || n_multi < 0 || (n_multi > 0 && (!multi || !ws)) || (zero && !pos) ||
      r_pad != nmfmu_pad_rank(rank))
    return NMFMU_ERR_ARG;
  NtfArgs a = ntf_args(seg, n_seg, idx_a, idx_b, vals, owner, pa, rows_a, pb, rows_b, rank, beta);
  a.pos = pos, a.pos_plane = pos_plane, a.ws = ws, a.step = 1, a.ap = MaskedApply{l1, l2, gamma};
  return ntf_launch(a, multi, n_multi, zero != 0, stage, S(stream));
}

int nmfmu_sp_ntf_loss(const int32_t* seg, int n_seg, const int32_t* idx_a, const int32_t* idx_b, const float* vals, int nnz,
                      const float* owner, const float* pa, int rows_a, const float* pb, int rows_b, int rank, float beta,
                      int zero, double v_term, double* part, double* out, int stage, void* stream) {
  if (const int rc = ntf_check(seg, n_seg, idx_a, idx_b, vals, nnz, owner, pa, rows_a, pb, rows_b, rank, beta, zero, stage))
    return rc;
  if (!part || !out) return NMFMU_ERR_ARG;
  NtfArgs a = ntf_args(seg, n_seg, idx_a, idx_b, vals, const_cast<float*>(owner), pa, rows_a, pb, rows_b, rank, beta);
  a.part = part;
  const int kind = nmfmu_beta_kind(beta);
  const int mask = ntf_stage_mask(rows_a, rows_b, rank, stage);
  unsigned grid;
  size_t lds;
  if (const int rc = ntf_grid(a, mask, grid, lds)) return rc;
  for_rl(a.r_pad, [&](auto rl) {
    for_kind_zero(kind, zero != 0, [&](auto k, auto z) {
      for_st(mask, [&](auto s) {
        hipLaunchKernelGGL(
            (sp_ntf_loss_kernel<decltype(rl)::value, decltype(k)::value, decltype(z)::value, decltype(s)::value>),
            dim3(grid), dim3(256), lds, S(stream), a);
      });
    });
  });
  // 'missing': metrics.py:39 halves the sum of squares, metrics.py:96 divides by beta (beta - 1).  'zero': the partials
  // hold the negative part, *out = v_term - neg
  double add = v_term, mul = 1.0;
  if (zero) add = -v_term, mul = -1.0;
  else if (kind == NMFMU_BETA_EUC) mul = 0.5;
  else if (kind == NMFMU_BETA_GEN) mul = 1.0 / ((double)beta * ((double)beta - 1.0));
  hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, (n_seg + 3) / 4, add, mul, out);
  return (int)hipGetLastError();
}

}  // extern "C"
