// Batched Hoyer projection (Hoyer 2004, "Non-negative Matrix Factorization with Sparseness Constraints", section 3.3 and its
// appendix): every slice of a factor is moved to the closest non-negative point with a prescribed L1 norm k1 and squared L2
// norm k2.  x is a contiguous fp32 tensor seen as [outer][J][inner]; slice j is every element with index j on the middle
// axis (n = outer * inner elements).  One workgroup of 256 threads owns one slice for its whole loop; the grid is J workgroups
// and nothing crosses workgroups: no atomics, no spin-waits, no host round trip.
//
// Per slice (the reference's behaviour, quirks included -- see include/nmfmu.h):
//   v = s + (k1 - sum s) / n
//   repeat:  m = k1 / (n - zeroed);  w_i = zeroed_i ? v_i : v_i - m
//            alpha = larger root of |v + alpha w|^2 = k2 (discriminant clamped at 0);  v += alpha w
//            no v_i < 0: stop
//            zeroed |= v < 0;  v = relu(v);  v += (k1 - sum v) / (n - zeroed);  v = relu(v)
// Two sweeps over the slice per pass, one block-wide reduction after each:
//   sweep B  applies the pending shift (and relu) and accumulates the three dot products of the pass (the step needs them);
//   sweep A  takes the step, tests for negatives (needs the step), flags and clamps them, and accumulates sum v, the count
//            of negatives and the count zeroed (the next shift and the next m need those).
// Between passes every value is >= 0, so the "zeroed" flag of an element lives in its sign bit: no flag array.  Only the first
// pass holds genuinely negative values, and there no flag is set yet (`first`).
// Every thread touches only the elements e = tid (mod 256) of its slice, in LDS as in global memory, so the sweeps need no
// barrier of their own; the reductions carry their cross-lane partial sums in fp64 (c = v.v - k2 is a cancellation).
//
// Residency, per launch: n <= lds_max_elems keeps the slice in LDS (read from / written to the strided layout directly: adjacent
// workgroups walk the same cache lines at the same time and share them in L2); otherwise the passes stream a slice-major copy
// in `ws`, built and written back by a tiled transpose through LDS (coalesced on both sides for inner == 1).  A tensor that is
// slice-major already (outer == 1 or J == 1) is streamed in place.  The strided layout is touched exactly twice either way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nmfmu.h"
#include "nmfmu_aux.h"
#include "nmfmu_launch.h"

namespace nmfmu {

constexpr int kHoyerThreads = 256;
constexpr int kHoyerRedBytes = 256;                                     // double red[2][4 waves][3], padded to 256 bytes
constexpr int kHoyerLdsSmall = 16 * 1024;                               // several workgroups per CU for short slices
constexpr int kHoyerLdsLarge = 160 * 1024;                              // the whole LDS of a CU
constexpr int kHoyerSmallElems = (kHoyerLdsSmall - kHoyerRedBytes) / 4;
constexpr int kHoyerMaxElems = (kHoyerLdsLarge - kHoyerRedBytes) / 4;   // 40896

struct HoyerArgs {
  float* x;           // [outer][J][inner]
  float* stream;      // slice-major [J][n] (ws, or x itself when it is slice-major already); streamed residency only
  const float* k1;
  const float* k2;
  int* status;
  int64_t inner;
  int J;
  int n;
};

// Sum of three per-thread values over the workgroup; every thread gets the totals.  `red` is double[2][12]; alternating
// the half makes one barrier per call enough (a thread can only reach the second-next call after everyone left this one).
__device__ inline void block_sum3(double& a, double& b, double& c, double* red, int& phase) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  double* r = red + phase * 12;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) r[wave * 3 + 0] = a, r[wave * 3 + 1] = b, r[wave * 3 + 2] = c;
  __syncthreads();
  a = (r[0] + r[3]) + (r[6] + r[9]);
  b = (r[1] + r[4]) + (r[7] + r[10]);
  c = (r[2] + r[5]) + (r[8] + r[11]);
  phase ^= 1;
}

__device__ inline bool sign_of(float f) { return (__float_as_uint(f) >> 31) != 0; }
__device__ inline float with_sign(float f) { return __uint_as_float(__float_as_uint(f) | 0x80000000u); }
__device__ inline float relu_nan(float f) { return f < 0.f ? 0.f : f; }   // NaN stays NaN, as Tensor.relu_ keeps it

// offset of element e of slice j in the [outer][J][inner] layout
__device__ inline int64_t strided_offset(int64_t e, int j, int J, int64_t inner) {
  if (inner == 1) return e * J + j;
  const int64_t o = e / inner;
  return (o * J + j) * inner + (e - o * inner);
}

// RES: 0 = streamed from a.stream, 1 / 2 = slice in LDS (small / large request: two kernels, so that each has its own
// dynamic-LDS attribute and short slices keep several workgroups on a CU)
template <int RES>
__global__ void __launch_bounds__(kHoyerThreads) hoyer_kernel(HoyerArgs a) {
  constexpr bool LDS = RES != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);
  const int j = blockIdx.x, tid = threadIdx.x;
  const int64_t n = a.n;
  float* v = LDS ? reinterpret_cast<float*>(smem + kHoyerRedBytes) : a.stream + (size_t)j * n;
  const double k1 = a.k1[j], k2 = a.k2[j];
  int phase = 0;

  // the only read of the strided layout (LDS residency) + sum s
  double s0 = 0.0, u0 = 0.0, u1 = 0.0;
  for (int64_t e = tid; e < n; e += kHoyerThreads) {
    float r;
    if (LDS) {
      r = a.x[strided_offset(e, j, a.J, a.inner)];
      v[e] = r;
    } else {
      r = v[e];
    }
    s0 += (double)r;
  }
  block_sum3(s0, u0, u1, red, phase);
  float shift = (float)((k1 - s0) / (double)n);
  int64_t zeroed = 0;
  bool first = true;
  int passes = 0, code;
  for (;;) {
    const float m = (float)(k1 / (double)(n - zeroed));
    // sweep B: pending shift (+ relu after the first pass), the three dot products
    double sa = 0.0, sb = 0.0, sc = 0.0;
#pragma unroll 4
    for (int64_t e = tid; e < n; e += kHoyerThreads) {
      const float r = v[e];
      const bool z = !first && sign_of(r);
      const float val = first ? r + shift : relu_nan(fabsf(r) + shift);
      const float w = z ? val : val - m;
      v[e] = z ? with_sign(val) : val;
      sa += (double)w * (double)w;
      sb += (double)w * (double)val;
      sc += (double)val * (double)val;
    }
    block_sum3(sa, sb, sc, red, phase);
    const double qb = 2.0 * sb, qc = sc - k2;
    double disc = qb * qb - 4.0 * sa * qc;
    disc = disc < 0.0 ? 0.0 : disc;
    const float alpha = (float)((-qb + sqrt(disc)) * 0.5 / sa);
    ++passes;
    // sweep A: the step, the negative test, flags and clamp; sum v, negatives, zeroed
    double sv = 0.0, nneg = 0.0, nzero = 0.0;
#pragma unroll 4
    for (int64_t e = tid; e < n; e += kHoyerThreads) {
      const float r = v[e];
      bool z = !first && sign_of(r);
      const float val = first ? r : fabsf(r);
      const float w = z ? val : val - m;
      const float nv = fmaf(alpha, w, val);
      const bool neg = nv < 0.f;
      z |= neg;
      const float c = neg ? 0.f : nv;
      v[e] = z ? with_sign(c) : fabsf(c);   // (fabsf: a -0.0 that was not flagged must not read as a flag in the next pass)
      sv += (double)c;
      nneg += neg ? 1.0 : 0.0;
      nzero += z ? 1.0 : 0.0;
    }
    block_sum3(sv, nneg, nzero, red, phase);
    first = false;
    if (nneg == 0.0) {          // also the exit of a NaN: nothing compares < 0
      code = passes;
      break;
    }
    if (passes >= n) {          // every useful pass zeroes one more coordinate: n passes are the cap
      code = -passes;
      break;
    }
    zeroed = (int64_t)nzero;
    shift = (float)((k1 - sv) / (double)(n - zeroed));
  }
  // the only write of the strided layout (LDS residency) / the flags leave the sign bits
  for (int64_t e = tid; e < n; e += kHoyerThreads) {
    const float r = fabsf(v[e]);
    if (LDS)
      a.x[strided_offset(e, j, a.J, a.inner)] = r;
    else
      v[e] = r;
  }
  if (tid == 0 && a.status) a.status[j] = code;
}

// x [rows][J] <-> ws [J][rows] (inner == 1): 64 x 64 tiles through LDS, both sides coalesced.  grid = (row tiles, J tiles).
template <bool TO_WS>
__global__ void __launch_bounds__(256) hoyer_transpose_kernel(float* __restrict__ x, float* __restrict__ ws, int64_t rows, int J) {
  __shared__ float tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int64_t j0 = (int64_t)blockIdx.y * 64; j0 < J; j0 += (int64_t)gridDim.y * 64) {
  for (int k = ty; k < 64; k += 4) {
    if (TO_WS) {
      const int64_t r = r0 + k;
      const int64_t j = j0 + tx;
      if (r < rows && j < J) tile[k][tx] = x[r * J + j];
    } else {
      const int64_t j = j0 + k;
      const int64_t r = r0 + tx;
      if (r < rows && j < J) tile[tx][k] = ws[j * rows + r];
    }
  }
  __syncthreads();
  for (int k = ty; k < 64; k += 4) {
    if (TO_WS) {
      const int64_t j = j0 + k;
      const int64_t r = r0 + tx;
      if (r < rows && j < J) ws[j * rows + r] = tile[tx][k];
    } else {
      const int64_t r = r0 + k;
      const int64_t j = j0 + tx;
      if (r < rows && j < J) x[r * J + j] = tile[k][tx];
    }
  }
  __syncthreads();
  }
}

// the same for inner > 1: ws[j][o * inner + i] <-> x[o][j][i]; consecutive threads walk ws, whose runs of `inner` elements are
// runs of x too
template <bool TO_WS>
__global__ void __launch_bounds__(256) hoyer_regroup_kernel(float* __restrict__ x, float* __restrict__ ws, int64_t n, int J,
                                                            int64_t inner) {
  const int64_t total = n * J;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx / n);
    const int64_t e = idx - (int64_t)j * n;
    const int64_t off = strided_offset(e, j, J, inner);
    if (TO_WS)
      ws[idx] = x[off];
    else
      x[off] = ws[idx];
  }
}

static int hoyer_regroup(bool to_ws, float* x, float* ws, int64_t outer, int J, int64_t inner, hipStream_t s) {
  if (inner == 1) {
    dim3 grid((unsigned)((outer + 63) / 64), (unsigned)std::min((J + 63) / 64, 65535));
    if (to_ws)
      hipLaunchKernelGGL(hoyer_transpose_kernel<true>, grid, dim3(256), 0, s, x, ws, outer, J);
    else
      hipLaunchKernelGGL(hoyer_transpose_kernel<false>, grid, dim3(256), 0, s, x, ws, outer, J);
  } else {
    const int64_t n = outer * inner;
    const unsigned grid = (unsigned)std::min<int64_t>((n * J + 255) / 256, 1 << 16);
    if (to_ws)
      hipLaunchKernelGGL(hoyer_regroup_kernel<true>, dim3(grid), dim3(256), 0, s, x, ws, n, J, inner);
    else
      hipLaunchKernelGGL(hoyer_regroup_kernel<false>, dim3(grid), dim3(256), 0, s, x, ws, n, J, inner);
  }
  return (int)hipGetLastError();
}

static int hoyer_lds_limit(int lds_max_elems) {
  return lds_max_elems <= 0 ? kHoyerMaxElems : std::min(lds_max_elems, kHoyerMaxElems);
}

static bool hoyer_shape_ok(int64_t outer, int J, int64_t inner, int* err) {
  if (outer < 1 || inner < 1) return *err = NMFMU_ERR_ARG, false;
  if (J < 1 || outer >= ((int64_t)1 << 31) || inner >= ((int64_t)1 << 31) || outer * inner >= ((int64_t)1 << 31))
    return *err = NMFMU_ERR_UNSUPPORTED, false;
  return true;
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int64_t nmfmu_hoyer_project_ws(int64_t outer, int J, int64_t inner, int lds_max_elems) {
  int err = 0;
  if (!hoyer_shape_ok(outer, J, inner, &err)) return err;
  const int64_t n = outer * inner;
  if (n <= hoyer_lds_limit(lds_max_elems) || outer == 1 || J == 1) return 0;
  return (int64_t)J * n * (int64_t)sizeof(float);
}

int nmfmu_hoyer_project(float* x, int64_t outer, int J, int64_t inner, const float* k1, const float* k2, int lds_max_elems,
                        void* ws, int* status, void* stream) {
  int err = 0;
  if (!hoyer_shape_ok(outer, J, inner, &err)) return err;
  if (!x || !k1 || !k2) return NMFMU_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = outer * inner;
  HoyerArgs a{x, nullptr, k1, k2, status, inner, J, (int)n};
  if (n <= hoyer_lds_limit(lds_max_elems)) {
    if (n <= kHoyerSmallElems)
      return launch_with_dynamic_lds<hoyer_kernel<1>, kHoyerThreads, kHoyerLdsSmall>(dim3(J), s, a);
    return launch_with_dynamic_lds<hoyer_kernel<2>, kHoyerThreads, kHoyerLdsLarge>(dim3(J), s, a);
  }
  const bool in_place = outer == 1 || J == 1;
  if (!in_place && !ws) return NMFMU_ERR_ARG;
  a.stream = in_place ? x : static_cast<float*>(ws);
  if (!in_place) {
    int e = hoyer_regroup(true, x, a.stream, outer, J, inner, s);
    if (e) return e;
  }
  hipLaunchKernelGGL(hoyer_kernel<0>, dim3(J), dim3(kHoyerThreads), kHoyerRedBytes, s, a);
  int e = (int)hipGetLastError();
  if (e || in_place) return e;
  return hoyer_regroup(false, x, a.stream, outer, J, inner, s);
}

}  // extern "C"
