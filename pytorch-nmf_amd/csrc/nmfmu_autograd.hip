// Backward of NMF.reconstruct (out = owner panel^T) for torch.autograd:
//   grad_owner[m][r] = sum_k G[m][k] panel[k][r]        contraction over k
//   grad_panel[k][r] = sum_m G[m][k] owner[m][r]        contraction over m, G read TRANSPOSED in place
// Both are out[i][r] = sum_c A(i, c) B[c][r] with B a row-major factor [C][R] and A the incoming gradient G, walked either
// along its rows (A(i, c) = G[i ld + c]) or along its columns (A(i, c) = G[c ld + i]): one kernel, templated on that.
// No transposed copy of G or of a factor exists anywhere.
//
// Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), the grade and the staging idiom of reconstruct_kernel (nmfmu_aux.hip): a
// 128 x 128 output tile per workgroup (4 waves, 64 x 64 = 2 x 2 MFMA tiles each), the contraction staged through LDS 32
// steps at a time with coalesced 16-byte loads.  The output has only rows/128 x rank/128 tiles -- 32 of them for
// grad_owner at 4096 x 65536 rank 128 -- so the contraction is cut into `nsplit` parts (backward_nsplit below: a pure
// function of the shape), one workgroup per (tile, part).  With nsplit > 1 the parts go to a caller-owned slab
// [nsplit][rows][R] and slab_sum_kernel adds them in part order: no floating-point atomics, bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "nmfmu_aux.h"

namespace nmfmu {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBwBK = 32;            // contraction steps per LDS stage; a part is a whole number of stages
constexpr int kBwLDA = kBwBK + 1;    // G walked along rows: sa[i][c], row stride 33 floats (per-lane reads a[i = j][c] conflict free)
constexpr int kBwLDT = 128;          // contraction-major tiles sa[c][i] / sb[c][r]: lanes read consecutive floats
constexpr int kBwTargetWgs = 512;    // two workgroups on each of the 256 CUs
constexpr int kBwMinStages = 4;      // a part is at least 128 contraction steps long ...
constexpr int kBwMaxSplit = 64;      // ... and there are at most 64 of them

int backward_nsplit(int rows, int contraction, int rank) {
  const int64_t tiles = (int64_t)((rows + 127) / 128) * ((rank + 127) / 128);
  const int stages = (contraction + kBwBK - 1) / kBwBK;
  const int64_t want = (kBwTargetWgs + tiles - 1) / tiles;
  const int cap = std::max(1, stages / kBwMinStages);
  const int n = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, cap), kBwMaxSplit));
  const int per = (stages + n - 1) / n;          // stages per part
  return (stages + per - 1) / per;               // no empty part; only the last one may be short
}
int backward_part_len(int contraction, int nsplit) {
  const int stages = (contraction + kBwBK - 1) / kBwBK;
  return (stages + nsplit - 1) / nsplit * kBwBK;
}

// out (+ part * rows * R) [i][r] = sum_{c in part} A(i, c) B[c][r].  grid = (row tiles, rank tiles, parts).
template <bool TRANS>
__global__ void __launch_bounds__(256) reconstruct_backward_kernel(const float* __restrict__ G, int64_t ld, int rows, int C,
                                                                   const float* __restrict__ B, int R, int part_len,
                                                                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sa[TRANS ? kBwBK * kBwLDT : 128 * kBwLDA];
  __shared__ __attribute__((aligned(16))) float sb[kBwBK * kBwLDT];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int i0 = blockIdx.x * 128, r0 = blockIdx.y * 128;
  const int cbeg = blockIdx.z * part_len, cend = min(C, cbeg + part_len);
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  // 16-byte loads need 16-byte aligned rows
  const bool vec_g = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0;
  const bool vec_b = (R & 3) == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0;
  for (int c0 = cbeg; c0 < cend; c0 += kBwBK) {
    // stage A(i0 .. i0+127, c0 .. c0+31) and B[c0 .. c0+31][r0 .. r0+127], zero fill outside the matrices / the part
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = p * 256 + tid;
      float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (TRANS) {
        const int cr = idx >> 5, i4 = (idx & 31) * 4;       // G[c0 + cr][i0 + i4 ..]: contiguous along i
        const int c = c0 + cr, i = i0 + i4;
        if (c < cend && i < rows) {
          const float* gp = G + (size_t)c * ld + i;
          if (vec_g && i + 3 < rows) {
            const float4 v = *reinterpret_cast<const float4*>(gp);
            av[0] = v.x, av[1] = v.y, av[2] = v.z, av[3] = v.w;
          } else {
            for (int q = 0; q < 4 && i + q < rows; ++q) av[q] = gp[q];
          }
        }
        *reinterpret_cast<float4*>(sa + cr * kBwLDT + i4) = make_float4(av[0], av[1], av[2], av[3]);
      } else {
        const int row = idx >> 3, c4 = (idx & 7) * 4;        // G[i0 + row][c0 + c4 ..]: contiguous along c
        const int c = c0 + c4, i = i0 + row;
        if (i < rows && c < cend) {
          const float* gp = G + (size_t)i * ld + c;
          if (vec_g && c + 3 < cend) {
            const float4 v = *reinterpret_cast<const float4*>(gp);
            av[0] = v.x, av[1] = v.y, av[2] = v.z, av[3] = v.w;
          } else {
            for (int q = 0; q < 4 && c + q < cend; ++q) av[q] = gp[q];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) sa[row * kBwLDA + c4 + q] = av[q];
      }
      {
        const int cr = idx >> 5, r4 = (idx & 31) * 4;
        const int c = c0 + cr, r = r0 + r4;
        if (c < cend && r < R) {
          const float* bp = B + (size_t)c * R + r;
          if (vec_b) {                                        // R % 4 == 0 and r % 4 == 0: r + 3 < R
            const float4 v = *reinterpret_cast<const float4*>(bp);
            bv[0] = v.x, bv[1] = v.y, bv[2] = v.z, bv[3] = v.w;
          } else {
            for (int q = 0; q < 4 && r + q < R; ++q) bv[q] = bp[q];
          }
        }
        *reinterpret_cast<float4*>(sb + cr * kBwLDT + r4) = make_float4(bv[0], bv[1], bv[2], bv[3]);
      }
    }
    __syncthreads();
    const float* pa = TRANS ? sa + hl * kBwLDT + wm * 64 + j : sa + (wm * 64 + j) * kBwLDA + hl;
    const float* pb = sb + hl * kBwLDT + wn * 64 + j;
#pragma unroll
    for (int s2 = 0; s2 < kBwBK; s2 += 2) {
      const float a0 = TRANS ? pa[s2 * kBwLDT] : pa[s2];
      const float a1 = TRANS ? pa[s2 * kBwLDT + 32] : pa[32 * kBwLDA + s2];
      const float b0 = pb[s2 * kBwLDT], b1 = pb[s2 * kBwLDT + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  float* o = out + (size_t)blockIdx.z * rows * R;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = r0 + wn * 64 + b * 32 + j;
      if (r < R) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = i0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          if (i < rows) o[(size_t)i * R + r] = acc[a][b][e];
        }
      }
    }
}

// out[i] = ((slab[0][i] + slab[1][i]) + slab[2][i]) + ...   (part order, whatever the grid)
__global__ void __launch_bounds__(256) slab_sum_kernel(const float* __restrict__ slab, int nslab, int64_t plane,
                                                       float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (int64_t)gridDim.x * 256) {
    float acc = slab[i];
    for (int s = 1; s < nslab; ++s) acc += slab[(size_t)s * plane + i];
    out[i] = acc;
  }
}

int launch_slab_sum(const float* slab, int nslab, int64_t plane, float* out, hipStream_t s) {
  const int rgrid = (int)std::min<int64_t>((plane + 255) / 256, 2048);
  hipLaunchKernelGGL(slab_sum_kernel, dim3(rgrid), dim3(256), 0, s, slab, nslab, plane, out);
  return (int)hipGetLastError();
}

// The product kernel of one half alone: its backward_nsplit(rows, C, R) parts go to dst -- [parts][rows][R] partial products,
// i.e. the output itself when there is one part.  The caller sums the parts (backward_half; nmfmu_plca_autograd.hip).
int launch_backward_product(bool trans, const float* G, int64_t ld, int rows, int C, const float* B, int R, float* dst,
                            hipStream_t s) {
  const int nsplit = backward_nsplit(rows, C, R);
  const int part_len = backward_part_len(C, nsplit);
  dim3 grid((rows + 127) / 128, (R + 127) / 128, nsplit);
  if (trans)
    hipLaunchKernelGGL(reconstruct_backward_kernel<true>, grid, dim3(256), 0, s, G, ld, rows, C, B, R, part_len, dst);
  else
    hipLaunchKernelGGL(reconstruct_backward_kernel<false>, grid, dim3(256), 0, s, G, ld, rows, C, B, R, part_len, dst);
  return (int)hipGetLastError();
}

static int backward_half(bool trans, const float* G, int64_t ld, int rows, int C, const float* B, int R, float* out,
                         float* slab, hipStream_t s) {
  const int nsplit = backward_nsplit(rows, C, R);
  int e = launch_backward_product(trans, G, ld, rows, C, B, R, nsplit > 1 ? slab : out, s);
  if (e || nsplit == 1) return e;
  return launch_slab_sum(slab, nsplit, (int64_t)rows * R, out, s);
}

int64_t backward_ws_floats(int m, int k, int rank, bool want_owner, bool want_panel, int* splits) {
  const int so = want_owner ? backward_nsplit(m, k, rank) : 0;
  const int sp = want_panel ? backward_nsplit(k, m, rank) : 0;
  if (splits) splits[0] = so, splits[1] = sp;
  return (so > 1 ? (int64_t)so * m * rank : 0) + (sp > 1 ? (int64_t)sp * k * rank : 0);
}

int launch_reconstruct_backward(const float* G, int64_t ld, int m, int k, const float* owner, const float* panel, int rank,
                                float* grad_owner, float* grad_panel, float* ws, hipStream_t s) {
  float* slab_p = ws;
  if (grad_owner) {
    const int so = backward_nsplit(m, k, rank);
    int e = backward_half(false, G, ld, m, k, panel, rank, grad_owner, ws, s);
    if (e) return e;
    if (so > 1) slab_p = ws + (size_t)so * m * rank;
  }
  if (grad_panel) return backward_half(true, G, ld, k, m, owner, rank, grad_panel, slab_p, s);
  return 0;
}

}  // namespace nmfmu
