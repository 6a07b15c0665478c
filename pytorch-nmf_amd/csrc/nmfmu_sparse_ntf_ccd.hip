// CCD on the CP model of a 3-way tensor: cyclic coordinate descent over the rank on the STORED entries of a sparse tensor, with
// a maintained residual (Yu, Hsieh, Si, Dhillon, ICDM 2012; the "CCD-TC" of Karlsson, Kressner, Uschmajew 2016) -- the beta = 2
// half-step of NTF.fit(solver='ccd', unstored='missing'), DESIGN.md section 40.  Owner F (the factor of the mode), panels Pa, Pb
// (the other two factors, fixed).  Every owner row i with stored entries e (panel rows a_e, b_e, value v_e), on its own:
//
//   q_e,k = __fmul_rn(Pa[a_e][k], Pb[b_e][k])                            (ONE rounded fp32 product, never fused into its use)
//   r_e = v_e - s_e,   s_e = sum_k F[i][k] q_e,k                          (k ascending, one fmaf chain from 0)
//   for k = 0 .. R-1:  d = sum_e q_e,k^2,   n = sum_e r_e q_e,k
//                      f' = max(eps, (fma(F[i][k], d, n) - l1) / ((d + l2) + eps))
//                      r_e = fma(-(f' - F[i][k]), q_e,k, r_e) for every e;   F[i][k] = f'
//
// A row without entries is not touched.  This is nmfmu_sparse_ccd.hip's recurrence with the Khatri-Rao value q_e,k where the
// matrix sweep has P[j_e][k], and its protocol is kept to the letter: the hand-out through `order` (longest rows first); one
// wave for a row of at most wg_rows entries, a workgroup of kCcdWgWaves waves above that (a second launch over the same list);
// entry e on lane e mod 64 of wave (e / 64) mod NW, slot e / (64 NW); d and n per-lane fmaf chains in slot order, the xor
// butterfly 32 .. 1, the waves' totals through LDS in wave order; residuals in registers up to limit NW entries, otherwise in
// the row's slice of an nnz-float scratch; the owner row in LDS; plain vector stores, no atomics, no fences.  So a sweep is BIT
// FOR BIT nmfmu_sp_ccd_sweep on the materialised rows: the rows x nnz matrix whose entry e names panel row e of
// P_eff[e][k] = fp32(Pa[a_e][k] Pb[b_e][k]).
//
// What is this kernel's own: q costs two gathers and a product per entry and coordinate and does not depend on the residual,
// so the rank is walked in groups of G coordinates.  G = 4 (rank % 4 == 0, both panels 16-byte aligned): a lane fetches
// Pa[a_e][k .. k+3] and Pb[b_e][k .. k+3] with one 16-byte load each and forms four q per slot; G = 1: 4-byte loads, any rank.
//   register rows   r, a, b for kCcdSlots slots and kCcdSlots x G values of q: one gather pair per slot and group, then the
//                   G coordinates' reduce / update steps run from registers;
//   scratch rows    G + 1 walks over the row's slots per group: walk 0 reduces coordinate 0, walk j updates the residuals
//                   with coordinate j - 1 and in the same visit reduces coordinate j, walk G updates with the last one.  A
//                   walk reads a_e, b_e, the residual and one gather pair per slot; the residual is updated before it enters
//                   the next coordinate's chain, and the chains stay in slot order -- the operations of the two-walk form
//                   (G = 1: reduce, update) in the same order.
// Both forms produce the same floats in the same order: no bit depends on the choice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr float kTcdEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps
constexpr int kTcdSlots = 8;                         // residuals a lane keeps in registers
constexpr int kTcdLimit = 64 * kTcdSlots;            // = nmfmu_sp_ccd_limit()
constexpr int kTcdWgWaves = 16;                      // = nmfmu_sp_ccd_wg_waves()

struct TcdArgs {
  const int32_t* rowptr;
  const int32_t* idx_a;
  const int32_t* idx_b;
  const float* vals;
  const int32_t* order;    // NULL: rows in their own order
  float* owner;
  const float* pa;
  const float* pb;
  float* scratch;          // [nnz]
  int n_rows, rank, limit, wg_rows;
  float l1, l2;
};

// q[g] = q_e,k0+g for g < G: one 16-byte load per panel (G == 4) or one 4-byte load
template <int G>
__device__ __forceinline__ void tcd_q(float (&q)[G], const TcdArgs& a, int ia, int ib, int k0) {
  const float* __restrict__ ra = a.pa + (size_t)ia * a.rank + k0;
  const float* __restrict__ rb = a.pb + (size_t)ib * a.rank + k0;
  if constexpr (G == 4) {
    const float4 x = *reinterpret_cast<const float4*>(ra);
    const float4 y = *reinterpret_cast<const float4*>(rb);
    q[0] = __fmul_rn(x.x, y.x), q[1] = __fmul_rn(x.y, y.y), q[2] = __fmul_rn(x.z, y.z), q[3] = __fmul_rn(x.w, y.w);
  } else {
    q[0] = __fmul_rn(ra[0], rb[0]);
  }
}

// f' of one coordinate from the row's totals; every lane computes the same bits
__device__ __forceinline__ float tcd_minimiser(float f, float d, float n, float l1, float l2) {
  const float num = fmaf(f, d, n) - l1;
  const float den = (d + l2) + kTcdEps;
  return fmaxf(kTcdEps, num / den);   // (a NaN quotient gives eps)
}

// the row's totals from the lanes' chains: butterfly 32 .. 1, then (NW > 1) the waves' totals in wave order; the LDS buffer
// alternates with the coordinate: one barrier per coordinate
template <int NW>
__device__ __forceinline__ void tcd_totals(float& d, float& n, float* red, int k, int lane, int wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // the two butterflies interleaved: two shuffles in flight
    d += __shfl_xor(d, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  if constexpr (NW > 1) {
    float* rd = red + (k & 1) * 2 * NW;
    if (lane == 0) rd[wave] = d, rd[NW + wave] = n;
    __syncthreads();
    d = rd[0], n = rd[NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) d += rd[w], n += rd[NW + w];
  }
}

// the residuals, both index arrays and the group's q of the row in registers: at most kTcdSlots slots per lane
template <int G, int NW>
__device__ __forceinline__ void tcd_row_reg(const TcdArgs& a, int p0, int cnt, float* fs, float* red, int lane, int wave) {
  const int rank = a.rank;
  const int T = (cnt + 64 * NW - 1) / (64 * NW);   // <= kTcdSlots, uniform over the workgroup
  const int first = 64 * wave + lane;              // this lane's entry of slot 0; slot t: first + 64 NW t
  float r[kTcdSlots], q[kTcdSlots][G];
  int ia[kTcdSlots], ib[kTcdSlots];
  bool on[kTcdSlots];
#pragma unroll
  for (int t = 0; t < kTcdSlots; ++t) {
    const int e = first + 64 * NW * t;
    on[t] = e < cnt;
    ia[t] = on[t] ? a.idx_a[p0 + e] : 0;
    ib[t] = on[t] ? a.idx_b[p0 + e] : 0;
    r[t] = 0.f;                                    // s_e first, then r_e
  }
  // s_e: the slots' chains side by side (kTcdSlots gather pairs in flight), each in ascending k
  for (int k0 = 0; k0 < rank; k0 += G) {
#pragma unroll
    for (int t = 0; t < kTcdSlots; ++t) {
      if (t >= T) break;
      if (on[t]) {
        tcd_q<G>(q[t], a, ia[t], ib[t], k0);
#pragma unroll
        for (int g = 0; g < G; ++g) r[t] = fmaf(fs[k0 + g], q[t][g], r[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kTcdSlots; ++t)
    if (on[t]) r[t] = a.vals[p0 + first + 64 * NW * t] - r[t];

  for (int k0 = 0; k0 < rank; k0 += G) {
#pragma unroll
    for (int t = 0; t < kTcdSlots; ++t) {
      if (t >= T) break;
      if (on[t]) tcd_q<G>(q[t], a, ia[t], ib[t], k0);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k = k0 + g;
      const float f = fs[k];
      float d = 0.f, n = 0.f;
#pragma unroll
      for (int t = 0; t < kTcdSlots; ++t) {
        if (t >= T) break;
        if (on[t]) {
          d = fmaf(q[t][g], q[t][g], d);
          n = fmaf(r[t], q[t][g], n);
        }
      }
      tcd_totals<NW>(d, n, red, k, lane, wave);
      const float fn = tcd_minimiser(f, d, n, a.l1, a.l2);
      const float back = -(fn - f);
#pragma unroll
      for (int t = 0; t < kTcdSlots; ++t) {
        if (t >= T) break;
        if (on[t]) r[t] = fmaf(back, q[t][g], r[t]);
      }
      if (lane == 0 && wave == 0) fs[k] = fn;   // (coordinate k is not read again in this sweep)
    }
  }
}

// the residuals in scratch[p0 .. p0 + cnt), every lane its own entries; the indices re-read once per walk
template <int G, int NW>
__device__ __forceinline__ void tcd_row_scratch(const TcdArgs& a, int p0, int cnt, float* fs, float* red, int lane, int wave) {
  const int rank = a.rank;
  const int T = (cnt + 64 * NW - 1) / (64 * NW);
  const int first = 64 * wave + lane;
  const int32_t* __restrict__ xa = a.idx_a + p0;
  const int32_t* __restrict__ xb = a.idx_b + p0;
  float* res = a.scratch + p0;

#pragma unroll 2      // two slots' chains side by side
  for (int t = 0; t < T; ++t) {
    const int e = first + 64 * NW * t;
    if (e < cnt) {
      const int ca = xa[e], cb = xb[e];
      float s = 0.f;
      for (int k0 = 0; k0 < rank; k0 += G) {
        float q[G];
        tcd_q<G>(q, a, ca, cb, k0);
#pragma unroll
        for (int g = 0; g < G; ++g) s = fmaf(fs[k0 + g], q[g], s);
      }
      res[e] = a.vals[p0 + e] - s;
    }
  }

  for (int k0 = 0; k0 < rank; k0 += G) {
    float back = 0.f;
#pragma unroll
    for (int w = 0; w <= G; ++w) {      // walk w: update with coordinate k0 + w - 1 (w > 0), reduce coordinate k0 + w (w < G)
      float d = 0.f, n = 0.f;
#pragma unroll 4      // four slots' loads in flight; the chains stay t-ordered
      for (int t = 0; t < T; ++t) {
        const int e = first + 64 * NW * t;
        if (e < cnt) {
          float q[G];
          tcd_q<G>(q, a, xa[e], xb[e], k0);
          float rv = res[e];
          if (w > 0) {
            rv = fmaf(back, q[w > 0 ? w - 1 : 0], rv);
            res[e] = rv;
          }
          if (w < G) {
            const float p = q[w < G ? w : 0];
            d = fmaf(p, p, d);
            n = fmaf(rv, p, n);
          }
        }
      }
      if (w < G) {
        const int k = k0 + w;
        const float f = fs[k];
        tcd_totals<NW>(d, n, red, k, lane, wave);
        const float fn = tcd_minimiser(f, d, n, a.l1, a.l2);
        back = -(fn - f);
        if (lane == 0 && wave == 0) fs[k] = fn;
      }
    }
  }
}

// NW == 1: the rows of at most wg_rows entries, one wave each; NW > 1: the longer rows, one workgroup each.  Every decision
// before a barrier is a function of the row's count: uniform over the workgroup.  Registers: the one-wave kernel may take what
// eight waves per SIMD leave (64 VGPRs would spill the 8 x 4 q: it is held to 4 waves per SIMD, 128 VGPRs); the workgroup
// kernel's 1024 threads are 4 waves per SIMD by themselves.
template <int G, int NW>
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) sp_ntf_ccd_sweep_kernel(TcdArgs a) {
  __shared__ __attribute__((aligned(16))) float fs[256];          // the owner row
  __shared__ float red[NW > 1 ? 4 * NW : 1];                      // NW > 1: [2][2][NW]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int at = blockIdx.x;
  if (at >= a.n_rows) return;
  const int row = a.order ? a.order[at] : at;
  const int p0 = a.rowptr[row], cnt = a.rowptr[row + 1] - p0;
  if (cnt <= 0) return;           // a row without data stays as it is
  if ((cnt > a.wg_rows) != (NW > 1)) return;   // the other launch's row
  const int rank = a.rank;
  float* frow = a.owner + (size_t)row * rank;
  for (int c = threadIdx.x; c < rank; c += 64 * NW) fs[c] = frow[c];
  __syncthreads();
  if (cnt <= a.limit * NW) tcd_row_reg<G, NW>(a, p0, cnt, fs, red, lane, wave);
  else tcd_row_scratch<G, NW>(a, p0, cnt, fs, red, lane, wave);
  __syncthreads();
  for (int c = threadIdx.x; c < rank; c += 64 * NW) frow[c] = fs[c];
}

template <int G>
static void tcd_launch(const TcdArgs& a, hipStream_t s) {
  // the long rows first: they are the launch's tail
  hipLaunchKernelGGL((sp_ntf_ccd_sweep_kernel<G, kTcdWgWaves>), dim3((unsigned)a.n_rows), dim3(64 * kTcdWgWaves), 0, s, a);
  hipLaunchKernelGGL((sp_ntf_ccd_sweep_kernel<G, 1>), dim3((unsigned)a.n_rows), dim3(64), 0, s, a);
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_sp_ntf_ccd_sweep(const int32_t* rowptr, const int32_t* idx_a, const int32_t* idx_b, const float* vals,
                           const int32_t* order, int n_rows, float* owner, const float* pa, int rows_a, const float* pb,
                           int rows_b, int rank, float l1, float l2, float* scratch, int limit, int wg_rows, int vec,
                           void* stream) {
  if (!rowptr || !idx_a || !idx_b || !vals || !owner || !pa || !pb || !scratch || owner == pa || owner == pb)
    return NMFMU_ERR_ARG;
  if (n_rows <= 0 || rows_a <= 0 || rows_b <= 0 || rank <= 0 || limit < 0 || limit > kTcdLimit || wg_rows < 0 || vec < 0 ||
      vec > 2)
    return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  TcdArgs a;
  a.rowptr = rowptr, a.idx_a = idx_a, a.idx_b = idx_b, a.vals = vals, a.order = order, a.owner = owner, a.pa = pa, a.pb = pb;
  a.scratch = scratch;
  a.n_rows = n_rows, a.rank = rank;
  a.limit = limit == 0 ? kTcdLimit : limit;
  a.wg_rows = wg_rows == 0 ? kTcdLimit : wg_rows;
  a.l1 = l1, a.l2 = l2;
  // four-wide: every panel row starts on a 16-byte boundary
  const bool wide = vec != 1 && rank % 4 == 0 && ((uintptr_t)pa | (uintptr_t)pb) % 16 == 0;
  if (wide) tcd_launch<4>(a, S(stream));
  else tcd_launch<1>(a, S(stream));
  return (int)hipGetLastError();
}

}  // extern "C"
