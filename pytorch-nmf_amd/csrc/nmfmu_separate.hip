// Source separation: per-group soft masks of a fitted model (separation.py).
//
//   Y_g    = the reconstruction from the components of group g alone
//   D      = sum_{g < G} Y_g^p in ascending g            (p == 1: the one reconstruction over all components)
//   out_s  = v * (Y_g^p / (D + eps)),  g = the group of output plane s      (v = 1 without a mixture)
//
// Two kernels:
//
// * separate_kernel (nmfmu_separate; dense models, rank columns R' <= 512): the 128 x 128 tile of reconstruct_kernel
//   (nmfmu_aux.hip) -- four waves, each 2 x 2 tiles of v_mfma_f32_32x32x2_f32, the rank staged through LDS 32 columns at a time
//   with row stride 33 floats.  The host has sorted the components by group and padded every group to an even number of
//   columns (the K = 2 of the MFMA), so a group boundary always falls between two MFMA steps and the test for it is wave
//   uniform.  The rank is walked twice: pass 1 forms D in a second accumulator set (p == 1: the accumulators simply run
//   through every boundary), pass 2 forms every y_g again and turns the lane's 64 values into v y^p / (D + eps) at the end of
//   the group.  Y_g and D never reach memory; V is read once per tile, into registers, before pass 1 (its latency hides
//   behind the first walk).  A lane's 32 neighbours hold 32 consecutive columns of one row, so a store instruction writes
//   whole 128-byte lines (256 bytes for complex planes) without a detour through LDS.
//
// * separate_planes_kernel (nmfmu_separate_planes; any model): G fp32 planes already on the device, one thread per element
//   (four with 16-byte accesses when every base and stride allows), D per element in ascending g unless a denominator plane
//   is given.  An input plane and the output plane of the same group may coincide: a thread reads y_g of its elements before
//   it writes that plane's elements and touches no other element.
//
// Both are free of atomics, so a repeated call is bitwise identical, and a plane's bits do not depend on which other planes
// are selected.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"

namespace nmfmu {

constexpr int kSepBK = 32, kSepLD = kSepBK + 1;
constexpr int kSepMaxRank = 256;       // components
constexpr int kSepMaxCols = 512;       // R' <= R + G <= 2 R
constexpr int kSepPow1 = 0, kSepPow2 = 1, kSepPowGen = 2;
constexpr int kSepNoV = 0, kSepRealV = 1, kSepComplexV = 2;

template <int PMODE>
__device__ __forceinline__ float sep_pow(float y, float p) {
  if (PMODE == kSepPow1) return y;
  if (PMODE == kSepPow2) return y * y;
  return exp2f(p * log2f(y));          // y == 0: exp2f(-inf) = 0
}

// d + y^p as every kernel here forms it, so that a denominator accumulated plane by plane (nmfmu_separate_accumulate) has the
// bits of one summed inside a kernel: p == 2 is ONE fused multiply-add, written out so that it does not hang on the
// compiler's contraction choices.
template <int PMODE>
__device__ __forceinline__ float sep_accumulate(float d, float y, float p) {
  if (PMODE == kSepPow1) return d + y;
  if (PMODE == kSepPow2) return __builtin_fmaf(y, y, d);
  return d + exp2f(p * log2f(y));
}

// tables: gstart [G + 1] then slot [G] (the caller's device copy of the host tables nmfmu_separate validated)
template <int PMODE, int VKIND>
__global__ void __launch_bounds__(256) separate_kernel(const float* __restrict__ Hp, int N, const float* __restrict__ Wp,
                                                       int C, int Rp, int vec, const int32_t* __restrict__ tables, int G,
                                                       const float* __restrict__ V, int64_t ldv, float power, float eps,
                                                       float* __restrict__ out, int64_t ld) {
  constexpr int VW = VKIND == kSepComplexV ? 2 : 1;       // floats per element of V and of the output
  __shared__ float sa[128 * kSepLD], sb[128 * kSepLD];
  __shared__ int32_t s_gstart[kSepMaxRank + 1], s_slot[kSepMaxRank];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
  for (int i = tid; i <= G; i += 256) s_gstart[i] = tables[i];
  for (int i = tid; i < G; i += 256) s_slot[i] = tables[G + 1 + i];

  // the mixture of the lane's 64 elements (zero outside the matrix: those elements are never stored)
  float v[2][2][16 * VW];
  if (VKIND != kSepNoV) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int k = k0 + wn * 64 + b * 32 + j;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          const bool in = k < C && row < N;
          const float* vp = V + ((int64_t)row * ldv + k) * VW;
          if (VKIND == kSepComplexV) {
            f32x2 c = {0.f, 0.f};
            if (in) c = *reinterpret_cast<const f32x2*>(vp);
            v[a][b][2 * e] = c[0], v[a][b][2 * e + 1] = c[1];
          } else {
            v[a][b][e] = in ? *vp : 0.f;
          }
        }
      }
  }

  f32x16 acc[2][2], den[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f, den[a][b][e] = 0.f;

  // vec: float4 loads (16-byte aligned bases and rows, decided on the host)
  // one stage = H'[m0 .. m0+127][r0 .. r0+31] and W' likewise (zero fill outside the matrix), four float4 per thread and factor;
  // the next stage's loads are in flight while the MFMAs of the current one run -- except with a complex mixture, whose 128
  // registers of V leave no room for the 32 of a stage in flight (the kernel would spill)
  constexpr bool PREFETCH = VKIND != kSepComplexV;
  float ra[4][4], rb[4][4];
  auto load_stage = [&](int r0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = p * 256 + tid, row = idx >> 3, c4 = (idx & 7) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) ra[p][i] = 0.f, rb[p][i] = 0.f;
      const int r = r0 + c4;
      if (m0 + row < N && r < Rp) {
        const float* ap = Hp + (size_t)(m0 + row) * Rp + r;
        if (vec) {
          const float4 t = *reinterpret_cast<const float4*>(ap);
          ra[p][0] = t.x, ra[p][1] = t.y, ra[p][2] = t.z, ra[p][3] = t.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (r + i < Rp) ra[p][i] = ap[i];
        }
      }
      if (k0 + row < C && r < Rp) {
        const float* bp = Wp + (size_t)(k0 + row) * Rp + r;
        if (vec) {
          const float4 t = *reinterpret_cast<const float4*>(bp);
          rb[p][0] = t.x, rb[p][1] = t.y, rb[p][2] = t.z, rb[p][3] = t.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (r + i < Rp) rb[p][i] = bp[i];
        }
      }
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = p * 256 + tid, row = idx >> 3, c4 = (idx & 7) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) sa[row * kSepLD + c4 + i] = ra[p][i], sb[row * kSepLD + c4 + i] = rb[p][i];
    }
  };
  const float* pa = sa + (wm * 64 + j) * kSepLD + hl;
  const float* pb = sb + (wn * 64 + j) * kSepLD + hl;
  for (int pass = 0; pass < 2; ++pass) {
    // pass 0 at p == 1 closes nothing: the accumulators run through every boundary and end as D
    const bool closing = pass == 1 || PMODE != kSepPow1;
    int g = 0;                      // the first group not yet closed (wave uniform)
    if (PREFETCH) load_stage(0);
    for (int r0 = 0; r0 < Rp; r0 += kSepBK) {
      if (!PREFETCH) load_stage(r0);
      __syncthreads();              // the previous stage is consumed; the tables are visible
      store_stage();
      __syncthreads();
      if (PREFETCH && r0 + kSepBK < Rp) load_stage(r0 + kSepBK);
      const int s_end = min(kSepBK, Rp - r0);
      int s2 = 0;
      while (true) {
        // close every group that ends at column r0 + s2 (several when empty groups sit there; column 0 closes leading empty
        // groups).  g only moves forward, so the position shared by two stages closes nothing twice.
        if (closing) {
          while (g < G && s_gstart[g + 1] <= r0 + s2) {
            const int s = pass == 1 ? s_slot[g] : -1;
            if (pass == 0) {
#pragma unroll
              for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                  for (int e = 0; e < 16; ++e) den[a][b][e] = sep_accumulate<PMODE>(den[a][b][e], acc[a][b][e], power);
            } else if (s >= 0) {
#pragma unroll
              for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                  const int k = k0 + wn * 64 + b * 32 + j;
                  if (k < C) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                      const int row = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
                      if (row < N) {
                        const float m = sep_pow<PMODE>(acc[a][b][e], power) / den[a][b][e];
                        float* op = out + (((int64_t)s * N + row) * ld + k) * VW;
                        if (VKIND == kSepComplexV) {
                          const f32x2 c = {v[a][b][2 * e] * m, v[a][b][2 * e + 1] * m};
                          __builtin_nontemporal_store(c, reinterpret_cast<f32x2*>(op));
                        } else {
                          __builtin_nontemporal_store(VKIND == kSepRealV ? v[a][b][e] * m : m, op);
                        }
                      }
                    }
                  }
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
            ++g;
          }
        }
        if (s2 >= s_end) break;
        // the run of column pairs up to the next boundary or the end of the stage, free of tests
        int lim = s_end;
        if (closing && g < G) lim = min(lim, s_gstart[g + 1] - r0);
        for (; s2 < lim; s2 += 2) {
          const float a0 = pa[s2], a1 = pa[32 * kSepLD + s2];
          const float b0 = pb[s2], b1 = pb[32 * kSepLD + s2];
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
      }
    }
    if (pass == 0) {
      // D + eps, once; p == 1: the accumulators ran through every boundary and hold D
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            den[a][b][e] = (PMODE == kSepPow1 ? acc[a][b][e] : den[a][b][e]) + eps;
            acc[a][b][e] = 0.f;
          }
    }
  }
}

// ---- planes ------------------------------------------------------------------------------------------------------------------
// Y: plane g, element i at Y[g * ystride + i * yelem] (yelem 1, or 2 when the planes sit in the real slots of a complex
// output); Dp: NULL or the denominator plane [n]; out plane s, element i at out[(s * ostride + i) * VW].
template <int PMODE, int VKIND, int VEC>
__global__ void __launch_bounds__(256) separate_planes_kernel(const float* Y, int G, int64_t ystride, int yelem,
                                                              const float* __restrict__ Dp, const float* __restrict__ V,
                                                              int64_t n, float power, float eps,
                                                              const int32_t* __restrict__ slot, float* out, int64_t ostride) {
  constexpr int VW = VKIND == kSepComplexV ? 2 : 1;
  const int64_t nvec = VEC == 4 ? n / 4 : 0;          // whole groups of four elements; the rest is done one by one
  const int64_t items = VEC == 4 ? nvec + (n - 4 * nvec) : n;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const bool four = VEC == 4 && it < nvec;
    const int64_t i0 = VEC == 4 ? (four ? 4 * it : 4 * nvec + (it - nvec)) : it;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (Dp) {
      if (four) {
        const float4 t = *reinterpret_cast<const float4*>(Dp + i0);
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
      } else {
        d[0] = Dp[i0];
      }
    } else {
      for (int g = 0; g < G; ++g) {
        const float* yp = Y + (int64_t)g * ystride + i0 * yelem;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (four && yelem == 1) {
          const float4 t = *reinterpret_cast<const float4*>(yp);
          y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
        } else if (four) {
          const float4 t = *reinterpret_cast<const float4*>(yp), u = *reinterpret_cast<const float4*>(yp + 4);
          y[0] = t.x, y[1] = t.z, y[2] = u.x, y[3] = u.z;
        } else {
          y[0] = yp[0];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = sep_accumulate<PMODE>(d[q], y[q], power);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] += eps;
    float v[4 * VW];
#pragma unroll
    for (int q = 0; q < 4 * VW; ++q) v[q] = 1.f;
    if (VKIND != kSepNoV) {
      const float* vp = V + i0 * VW;
      if (four) {
#pragma unroll
        for (int q = 0; q < VW; ++q) {
          const float4 t = *reinterpret_cast<const float4*>(vp + 4 * q);
          v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
        }
      } else {
        for (int q = 0; q < VW; ++q) v[q] = vp[q];
      }
    }
    for (int g = 0; g < G; ++g) {
      const int s = slot[g];
      if (s < 0) continue;
      const float* yp = Y + (int64_t)g * ystride + i0 * yelem;
      float y[4] = {0.f, 0.f, 0.f, 0.f};
      if (four && yelem == 1) {
        const float4 t = *reinterpret_cast<const float4*>(yp);
        y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
      } else if (four) {
        const float4 t = *reinterpret_cast<const float4*>(yp), u = *reinterpret_cast<const float4*>(yp + 4);
        y[0] = t.x, y[1] = t.z, y[2] = u.x, y[3] = u.z;
      } else {
        y[0] = yp[0];
      }
      float m[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) m[q] = sep_pow<PMODE>(y[q], power) / d[q];
      float* op = out + ((int64_t)s * ostride + i0) * VW;
      if (VKIND == kSepComplexV) {
        if (four) {
          *reinterpret_cast<float4*>(op) = make_float4(v[0] * m[0], v[1] * m[0], v[2] * m[1], v[3] * m[1]);
          *reinterpret_cast<float4*>(op + 4) = make_float4(v[4] * m[2], v[5] * m[2], v[6] * m[3], v[7] * m[3]);
        } else {
          op[0] = v[0] * m[0], op[1] = v[1] * m[0];
        }
      } else if (four) {
        *reinterpret_cast<float4*>(op) = VKIND == kSepRealV ? make_float4(v[0] * m[0], v[1] * m[1], v[2] * m[2], v[3] * m[3])
                                                            : make_float4(m[0], m[1], m[2], m[3]);
      } else {
        op[0] = VKIND == kSepRealV ? v[0] * m[0] : m[0];
      }
    }
  }
}

// D[i] = D[i] + Y[i * yelem]^p, one thread per element
template <int PMODE>
__global__ void __launch_bounds__(256) separate_accumulate_kernel(const float* __restrict__ Y, int yelem, int64_t n, float power,
                                                                  float* __restrict__ D) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    D[i] = sep_accumulate<PMODE>(D[i], Y[i * yelem], power);
}

static int sep_pmode(float power) { return power == 1.f ? kSepPow1 : power == 2.f ? kSepPow2 : kSepPowGen; }

template <int PMODE, int VKIND>
static void launch_separate(dim3 grid, hipStream_t s, const float* Hp, int N, const float* Wp, int C, int Rp, int vec,
                            const int32_t* tables, int G, const float* V, int64_t ldv, float power, float eps, float* out,
                            int64_t ld) {
  hipLaunchKernelGGL((separate_kernel<PMODE, VKIND>), grid, dim3(256), 0, s, Hp, N, Wp, C, Rp, vec, tables, G, V, ldv, power, eps,
                     out, ld);
}

template <int PMODE, int VKIND>
static void launch_planes(int vec, dim3 grid, hipStream_t s, const float* Y, int G, int64_t ystride, int yelem, const float* Dp,
                          const float* V, int64_t n, float power, float eps, const int32_t* slot, float* out, int64_t ostride) {
  if (vec)
    hipLaunchKernelGGL((separate_planes_kernel<PMODE, VKIND, 4>), grid, dim3(256), 0, s, Y, G, ystride, yelem, Dp, V, n, power,
                       eps, slot, out, ostride);
  else
    hipLaunchKernelGGL((separate_planes_kernel<PMODE, VKIND, 1>), grid, dim3(256), 0, s, Y, G, ystride, yelem, Dp, V, n, power,
                       eps, slot, out, ostride);
}

static bool sep_slots_ok(const int32_t* slot, int G, int S) {
  for (int g = 0; g < G; ++g)
    if (slot[g] < -1 || slot[g] >= S) return false;
  return true;
}

static bool sep_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace nmfmu

using namespace nmfmu;

#define SEP_DISPATCH(FN, pm, vk, ...)                                              \
  do {                                                                             \
    if (pm == kSepPow1 && vk == kSepNoV) FN<kSepPow1, kSepNoV>(__VA_ARGS__);       \
    else if (pm == kSepPow1 && vk == kSepRealV) FN<kSepPow1, kSepRealV>(__VA_ARGS__); \
    else if (pm == kSepPow1) FN<kSepPow1, kSepComplexV>(__VA_ARGS__);              \
    else if (pm == kSepPow2 && vk == kSepNoV) FN<kSepPow2, kSepNoV>(__VA_ARGS__);  \
    else if (pm == kSepPow2 && vk == kSepRealV) FN<kSepPow2, kSepRealV>(__VA_ARGS__); \
    else if (pm == kSepPow2) FN<kSepPow2, kSepComplexV>(__VA_ARGS__);              \
    else if (vk == kSepNoV) FN<kSepPowGen, kSepNoV>(__VA_ARGS__);                  \
    else if (vk == kSepRealV) FN<kSepPowGen, kSepRealV>(__VA_ARGS__);              \
    else FN<kSepPowGen, kSepComplexV>(__VA_ARGS__);                                \
  } while (0)

extern "C" {

int nmfmu_separate_max_rank(void) { return kSepMaxRank; }

int64_t nmfmu_separate_tables_bytes(int groups) { return groups < 1 ? 0 : (int64_t)(2 * groups + 1) * 4; }

int nmfmu_separate(const float* Hp, int n, const float* Wp, int c, int cols, const int32_t* gstart, const int32_t* slot,
                   int groups, int planes, void* tables_dev, const float* V, int v_kind, int64_t ldv, float power, float eps,
                   float* out, int64_t ld, void* stream) {
  if (!Hp || !Wp || !gstart || !slot || !tables_dev || !out || n <= 0 || c <= 0 || cols <= 0 || groups <= 0 || planes <= 0)
    return NMFMU_ERR_ARG;
  if (v_kind < kSepNoV || v_kind > kSepComplexV || (v_kind != kSepNoV && (!V || ldv < c)) || ld < c) return NMFMU_ERR_ARG;
  if (!(power > 0.f) || !(eps >= 0.f)) return NMFMU_ERR_ARG;
  if (gstart[0] != 0 || gstart[groups] != cols) return NMFMU_ERR_ARG;
  for (int g = 0; g < groups; ++g)
    if (gstart[g + 1] < gstart[g] || (gstart[g + 1] & 1)) return NMFMU_ERR_ARG;
  if (!sep_slots_ok(slot, groups, planes)) return NMFMU_ERR_ARG;
  if (groups > kSepMaxRank || cols > kSepMaxCols) return NMFMU_ERR_UNSUPPORTED;
  const int64_t gy = ((int64_t)n + 127) / 128;
  if (gy > 65535) return NMFMU_ERR_UNSUPPORTED;
  const uintptr_t elem_align = v_kind == kSepComplexV ? 7 : 3;      // complex elements are read and written as 8-byte pairs
  if ((reinterpret_cast<uintptr_t>(out) & elem_align) || (V && (reinterpret_cast<uintptr_t>(V) & elem_align))) return NMFMU_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int32_t* td = (const int32_t*)tables_dev;
  const int vec = (cols & 3) == 0 && sep_aligned16(Hp) && sep_aligned16(Wp);
  dim3 grid((c + 127) / 128, (unsigned)gy);
  const int pm = sep_pmode(power);
  SEP_DISPATCH(launch_separate, pm, v_kind, grid, s, Hp, n, Wp, c, cols, vec, td, groups, V, ldv, power, eps, out, ld);
  return (int)hipGetLastError();
}

int nmfmu_separate_planes(const float* Y, int groups, int64_t y_stride, int y_elem, const float* D, const float* V, int v_kind,
                          int64_t n, float power, float eps, const int32_t* slot, int planes, void* slot_dev, float* out,
                          int64_t out_stride, void* stream) {
  if (!Y || !slot || !slot_dev || !out || groups <= 0 || planes <= 0 || n <= 0) return NMFMU_ERR_ARG;
  if (y_elem != 1 && y_elem != 2) return NMFMU_ERR_ARG;
  if (y_stride < n * y_elem || out_stride < n) return NMFMU_ERR_ARG;
  if (v_kind < kSepNoV || v_kind > kSepComplexV || (v_kind != kSepNoV && !V)) return NMFMU_ERR_ARG;
  if (!(power > 0.f) || !(eps >= 0.f)) return NMFMU_ERR_ARG;
  if (!sep_slots_ok(slot, groups, planes)) return NMFMU_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int vw = v_kind == kSepComplexV ? 2 : 1;
  const int vec = n >= 4 && sep_aligned16(Y) && sep_aligned16(out) && (!D || sep_aligned16(D)) && (!V || sep_aligned16(V)) &&
                  (y_stride & 3) == 0 && ((out_stride * vw) & 3) == 0;
  const int64_t items = vec ? n / 4 + (n & 3) : n;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 1 << 16));
  const int pm = sep_pmode(power);
  SEP_DISPATCH(launch_planes, pm, v_kind, vec, dim3(grid), s, Y, groups, y_stride, y_elem, D, V, n, power, eps,
               (const int32_t*)slot_dev, out, out_stride);
  return (int)hipGetLastError();
}

int nmfmu_separate_accumulate(const float* Y, int y_elem, int64_t n, float power, float* D, void* stream) {
  if (!Y || !D || n <= 0 || (y_elem != 1 && y_elem != 2) || !(power > 0.f)) return NMFMU_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 16)));
  const int pm = sep_pmode(power);
  if (pm == kSepPow1) hipLaunchKernelGGL(separate_accumulate_kernel<kSepPow1>, grid, dim3(256), 0, s, Y, y_elem, n, power, D);
  else if (pm == kSepPow2) hipLaunchKernelGGL(separate_accumulate_kernel<kSepPow2>, grid, dim3(256), 0, s, Y, y_elem, n, power, D);
  else hipLaunchKernelGGL(separate_accumulate_kernel<kSepPowGen>, grid, dim3(256), 0, s, Y, y_elem, n, power, D);
  return (int)hipGetLastError();
}

}  // extern "C"
