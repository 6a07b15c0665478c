// PLCA on a sparse-COO target: the E-step of the EM iteration (reference: plca.py:248-253) over the stored entries only.
//
// With G = Vn / (H diag(Z) W^T + eps) every entry where Vn is zero has G = 0 and adds nothing to G W, G^T H or Z.grad, so
// the two numerator planes of an EM iteration are sums over the stored set -- exactly, not as an approximation:
//
//   estep  (H side, CSR list)  s_p = sum_r (H[i][r] Z[r]) W[j][r]      i = the segment's row, j = colidx[p]
//                              g_p = vn_p / (s_p + eps)                -> g_out[p], CSR order
//                              num[i][:] = sum_p g_p W[j][:]           = (G W)[i]
//   gather (W side, CSC list)  num[j][:] = sum_p g[perm[p]] H[i][:]    i = rowidx[p]   = (G^T H)[j]
//
// One reconstruction feeds every update of the iteration (plca.py:252): g is formed once, on the H side, and the W side
// reads it back through perm -- it holds no dot product, no butterfly and no divide.  The E-step's four butterflies of a trip
// are folded into one (see the kernel): same additions, same bits, 7 cross-lane moves instead of 24.
//
// Segments, 64-entry blocks, the panel-row fetch, the ws slots: the shared protocol of nmfmu_sparse_common.h (one wave per
// segment, lanes across the rank, RL rank slots per lane, kSpU gathers in flight, entries in storage order, a split row's
// partial rows through ws slots and a finishing kernel in segment order).  Plain vector stores, no atomics: a repeated call
// is bitwise identical.  The M-step is nmfmu_plca.hip, which reads either plane as a single slab.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

// a finished row: every padded rank column is written
template <int RL>
__device__ __forceinline__ void plca_store_row(float* __restrict__ num, int row, const float (&acc)[RL], int rank,
                                               int r_pad, int lane) {
#pragma unroll
  for (int q = 0; q < RL; ++q) {
    const int r = lane + 64 * q;
    if (r < r_pad) num[(size_t)row * r_pad + r] = r < rank ? acc[q] : 0.f;
  }
}

static_assert(kSpU == 4, "the folded butterfly of sp_plca_estep_kernel reduces four entries at a time");

template <int RL>
__global__ void __launch_bounds__(256) sp_plca_estep_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                            const int32_t* __restrict__ colidx,
                                                            const float* __restrict__ vals_n,
                                                            const float* __restrict__ owner, const float* __restrict__ z,
                                                            const float* __restrict__ panel, int rank,
                                                            float* __restrict__ g_out, float* __restrict__ ws,
                                                            float* __restrict__ num, int r_pad) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_seg) return;
  const Seg sgm = load_seg(seg, sg);
  const int p1 = sgm.p1;
  float a[RL], acc[RL];
  load_row<RL>(a, owner, sgm.row, rank, lane);
#pragma unroll
  for (int q = 0; q < RL; ++q) {       // H[i] * Z once per segment: the reconstruction operand of plca.py:371-373
    const int r = lane + 64 * q;
    a[q] *= r < rank ? z[r] : 0.f;
    acc[q] = 0.f;
  }
  for (int base = sgm.p0; base < p1; base += 64) {
    const EntryBlock eb = load_block(colidx, base, p1, lane);
    const float vv = eb.pe < p1 ? vals_n[eb.pe] : 0.f;
    float gv = 0.f;                    // g of this lane's entry of the 64
    for (int j = 0; j < eb.cnt; j += kSpU) {
      float b[kSpU][RL], sdot[kSpU];
      bool ok[kSpU];
      fetch_group<RL>(b, ok, eb, j, panel, rank, lane);
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        sdot[u] = 0.f;
#pragma unroll
        for (int q = 0; q < RL; ++q) sdot[u] += a[q] * b[u][q];
      }
      // The four fixed-order butterflies, FOLDED: a lane of the standard butterfly ends with all four sums; here the 16 lanes
      // lane >> 4 == u end with the sum of entry u alone, so the first level moves two values per lane instead of four, the
      // second one, and the last four one instead of four: 7 cross-lane moves per group instead of 24.  The lanes of group
      // u perform exactly the additions the standard butterfly performs in them (own partial + the partner's, xor 32, 16, 8,
      // 4, 2, 1): the sum has the same bits.
      const bool h5 = lane & 32, h4 = lane & 16;
      float k0 = h5 ? sdot[2] : sdot[0], k1 = h5 ? sdot[3] : sdot[1];
      k0 += __shfl_xor(h5 ? sdot[0] : sdot[2], 32, 64);
      k1 += __shfl_xor(h5 ? sdot[1] : sdot[3], 32, 64);
      float s = h4 ? k1 : k0;
      s += __shfl_xor(h4 ? k0 : k1, 16, 64);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      // one divide per entry and lane group, not four per lane; g reaches the wave as a scalar
      const int ue = lane >> 4;
      const float vu = __shfl(vv, (j + ue) & 63, 64);
      const float gl = j + ue < eb.cnt ? vu / (s + kEps) : 0.f;     // an entry past the end adds nothing
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {     // storage order
        const float g = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), 16 * u));
        if (lane == j + u) gv = g;
#pragma unroll
        for (int q = 0; q < RL; ++q) acc[q] += g * b[u][q];
      }
    }
    if (eb.pe < p1) g_out[eb.pe] = gv;     // once per stored entry, by the lane that owns it
  }
  if (sgm.slot >= 0) {
    store_partial<1, RL>(ws, sgm.slot, 0, acc, r_pad, lane);
    return;
  }
  plca_store_row<RL>(num, sgm.row, acc, rank, r_pad, lane);
}

template <int RL>
__global__ void __launch_bounds__(256) sp_plca_gather_kernel(const int32_t* __restrict__ seg, int n_seg,
                                                             const int32_t* __restrict__ rowidx,
                                                             const int32_t* __restrict__ perm, const float* __restrict__ g,
                                                             const float* __restrict__ panel, int rank,
                                                             float* __restrict__ ws, float* __restrict__ num, int r_pad) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_seg) return;
  const Seg sgm = load_seg(seg, sg);
  const int p1 = sgm.p1;
  float acc[RL];
#pragma unroll
  for (int q = 0; q < RL; ++q) acc[q] = 0.f;
  for (int base = sgm.p0; base < p1; base += 64) {
    const EntryBlock eb = load_block(rowidx, base, p1, lane);
    const float gv = eb.pe < p1 ? g[perm[eb.pe]] : 0.f;     // the CSR position of CSC entry pe
    for (int j = 0; j < eb.cnt; j += kSpU) {
      float gu[kSpU], b[kSpU][RL];
      bool ok[kSpU];
      fetch_group<RL>(b, ok, eb, j, panel, rank, lane);
#pragma unroll
      for (int u = 0; u < kSpU; ++u) gu[u] = ok[u] ? __shfl(gv, (j + u) & 63, 64) : 0.f;
#pragma unroll
      for (int u = 0; u < kSpU; ++u)       // storage order
#pragma unroll
        for (int q = 0; q < RL; ++q) acc[q] += gu[u] * b[u][q];
    }
  }
  if (sgm.slot >= 0) {
    store_partial<1, RL>(ws, sgm.slot, 0, acc, r_pad, lane);
    return;
  }
  plca_store_row<RL>(num, sgm.row, acc, rank, r_pad, lane);
}

// one wave per split row: its partial rows added in segment order (both sides)
__global__ void __launch_bounds__(256) sp_plca_finish_kernel(const int32_t* __restrict__ multi, int n_multi,
                                                             const float* __restrict__ ws, float* __restrict__ num,
                                                             int rank, int r_pad) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_multi) return;
  const Multi mu = load_multi(multi, m);
  for (int r = lane; r < r_pad; r += 64) {
    float acc[1];
    sum_partials<1>(acc, ws, mu, r, r_pad);
    num[(size_t)mu.row * r_pad + r] = r < rank ? acc[0] : 0.f;
  }
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
// NMFMU_OK or the answer both entries give before any device work
int plca_shape_check(int n_seg, const int32_t* multi, int n_multi, const float* ws, int rank, int r_pad) {
  if (n_seg <= 0 || n_multi < 0 || rank <= 0) return NMFMU_ERR_ARG;
  if (n_multi > 0 && (!multi || !ws)) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (r_pad != nmfmu_pad_rank(rank)) return NMFMU_ERR_ARG;
  return NMFMU_OK;
}

int plca_finish(const int32_t* multi, int n_multi, const float* ws, float* num, int rank, int r_pad, hipStream_t st) {
  if (n_multi > 0)
    hipLaunchKernelGGL(sp_plca_finish_kernel, dim3((n_multi + 3) / 4), dim3(256), 0, st, multi, n_multi, ws, num, rank,
                       r_pad);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" {

int nmfmu_sp_plca_estep(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* colidx,
                        const float* vals_n, const float* owner, const float* z, const float* panel, int rank, float* g_out,
                        float* ws, float* num, int r_pad, void* stream) {
  if (!seg || !colidx || !vals_n || !owner || !z || !panel || !g_out || !num) return NMFMU_ERR_ARG;
  if (const int rc = plca_shape_check(n_seg, multi, n_multi, ws, rank, r_pad)) return rc;
  for_rl(r_pad, [&](auto rl) {
    hipLaunchKernelGGL((sp_plca_estep_kernel<decltype(rl)::value>), dim3((n_seg + 3) / 4), dim3(256), 0, S(stream), seg,
                       n_seg, colidx, vals_n, owner, z, panel, rank, g_out, ws, num, r_pad);
  });
  return plca_finish(multi, n_multi, ws, num, rank, r_pad, S(stream));
}

int nmfmu_sp_plca_gather(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* rowidx,
                         const int32_t* perm, const float* g, const float* panel, int rank, float* ws, float* num, int r_pad,
                         void* stream) {
  if (!seg || !rowidx || !perm || !g || !panel || !num) return NMFMU_ERR_ARG;
  if (const int rc = plca_shape_check(n_seg, multi, n_multi, ws, rank, r_pad)) return rc;
  for_rl(r_pad, [&](auto rl) {
    hipLaunchKernelGGL((sp_plca_gather_kernel<decltype(rl)::value>), dim3((n_seg + 3) / 4), dim3(256), 0, S(stream), seg,
                       n_seg, rowidx, perm, g, panel, rank, ws, num, r_pad);
  });
  return plca_finish(multi, n_multi, ws, num, rank, r_pad, S(stream));
}

}  // extern "C"
