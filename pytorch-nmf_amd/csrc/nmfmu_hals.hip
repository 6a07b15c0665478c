// HALS sweep (Cichocki & Phan 2009; the coordinate descent of sklearn's NMF solver 'cd'): one Gauss-Seidel pass over the rank
// of the Frobenius objective, for every row of a factor independently.  With a = X_owner @ panel and gram = panel^T panel,
//   for r = 0 .. rank-1:   s = sum_{j != r} f[row][j] gram[j][r]            (j < r: the values this pass already wrote)
//                          f[row][r] = max(eps, ((a[row][r] - l1) - s) / ((gram[r][r] + l2) + eps))
//
// One lane per row, one wave (= one workgroup) per 64 rows; nothing crosses waves.  The wave's rows live in LDS as
// fs[j][lane] (pitch 65 floats: the transposing load / store of the row-major factor and the sweep's reads are both
// conflict-free).  Row r of the SYMMETRIC gram matrix is wave-uniform: the wave fetches row r + 1 with one coalesced load per
// 64 columns while it sweeps coordinate r and parks it in a two-row LDS buffer, from which the sweep reads it as broadcast
// 16-byte loads (uniform loads straight from memory missed the 16 KB scalar cache at every step: the matrix is 64 KB at rank
// 128).  a is read once, 32 columns at a time, by the lane that owns the row (its private LDS column abuf[k][lane]).
//
// Accumulation scheme (tests/hals_emulation.py derives its error bound from exactly this): term j goes to accumulator
// j mod 4 by fmaf, in increasing j; slot r holds 0 while coordinate r is swept, so its term adds an exact +0;
// s = (acc0 + acc1) + (acc2 + acc3).  A row's bits depend on nothing but that row of f and a, gram, l1, l2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_launch.h"

namespace nmfmu {

constexpr float kHalsEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps = kEps of nmfmu_fused.h
constexpr int kHalsPitch = 65;                        // floats between fs[j][.] and fs[j + 1][.]
constexpr int kHalsAChunk = 32;                       // columns of a staged at a time
constexpr int hals_gram_row(int r_pad) { return r_pad < 64 ? 64 : r_pad; }   // floats of one buffered gram row
constexpr int hals_lds_bytes(int r_pad) { return (r_pad * kHalsPitch + kHalsAChunk * 64 + 2 * hals_gram_row(r_pad)) * 4; }

struct HalsArgs {
  float* f;            // [rows][rank], updated in place
  const float* a;      // [rows][lda]
  const float* gram;   // [rank][rank], symmetric
  int64_t lda;
  int rows, rank;
  float l1, l2;
};

// R_PAD sizes the dynamic LDS request (one kernel per request, so that each carries its own attribute) and the registers of
// the gram-row prefetch
template <int R_PAD>
__global__ void __launch_bounds__(64) hals_sweep_kernel(HalsArgs p) {
  extern __shared__ __attribute__((aligned(16))) float hals_lds[];
  float* fs = hals_lds;
  float* abuf = hals_lds + R_PAD * kHalsPitch;
  float* gbuf = abuf + kHalsAChunk * 64;
  constexpr int GROW = hals_gram_row(R_PAD), GL = GROW / 64;
  const int lane = threadIdx.x;
  const int rank = p.rank;
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  const int nrow = (int)(p.rows - row0 < 64 ? p.rows - row0 : 64);
  const bool valid = lane < nrow;
  const float* __restrict__ gram = p.gram;

  // row-major rows -> fs[c][rr]: a row is read by consecutive lanes; bank of the write = (c + rr) mod 64
  for (int rr = 0; rr < nrow; ++rr) {
    const float* src = p.f + (size_t)(row0 + rr) * rank;
    for (int c = lane; c < rank; c += 64) fs[c * kHalsPitch + rr] = src[c];
  }
  for (int c = lane; c < rank; c += 64) gbuf[c] = gram[c];
  __syncthreads();

  float* fcol = fs + lane;
  const float* arow = p.a + (size_t)(row0 + (valid ? lane : 0)) * p.lda;
  for (int r0 = 0; r0 < rank; r0 += kHalsAChunk) {
#pragma unroll
    for (int k = 0; k < kHalsAChunk; ++k) {
      float v = 0.f;
      if (valid && r0 + k < rank) v = arow[r0 + k];
      abuf[k * 64 + lane] = v;
    }
    const int r1 = r0 + kHalsAChunk < rank ? r0 + kHalsAChunk : rank;
    for (int r = r0; r < r1; ++r) {
      const float* g = gbuf + (r & 1) * GROW;
      float gnext[GL];
      if (r + 1 < rank) {
#pragma unroll
        for (int q = 0; q < GL; ++q) {
          const int c = lane + 64 * q;
          gnext[q] = c < rank ? gram[(size_t)(r + 1) * rank + c] : 0.f;
        }
      }
      fcol[r * kHalsPitch] = 0.f;
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
      int j = 0;
#pragma unroll 4
      for (; j + 4 <= rank; j += 4) {
        const float4 g4 = *reinterpret_cast<const float4*>(g + j);
        acc0 = fmaf(fcol[(j + 0) * kHalsPitch], g4.x, acc0);
        acc1 = fmaf(fcol[(j + 1) * kHalsPitch], g4.y, acc1);
        acc2 = fmaf(fcol[(j + 2) * kHalsPitch], g4.z, acc2);
        acc3 = fmaf(fcol[(j + 3) * kHalsPitch], g4.w, acc3);
      }
      if (j + 0 < rank) acc0 = fmaf(fcol[(j + 0) * kHalsPitch], g[j + 0], acc0);
      if (j + 1 < rank) acc1 = fmaf(fcol[(j + 1) * kHalsPitch], g[j + 1], acc1);
      if (j + 2 < rank) acc2 = fmaf(fcol[(j + 2) * kHalsPitch], g[j + 2], acc2);
      const float s = (acc0 + acc1) + (acc2 + acc3);
      const float num = (abuf[(r - r0) * 64 + lane] - p.l1) - s;
      const float den = (g[r] + p.l2) + kHalsEps;
      fcol[r * kHalsPitch] = fmaxf(kHalsEps, num / den);   // (a NaN quotient gives eps)
      if (r + 1 < rank) {
#pragma unroll
        for (int q = 0; q < GL; ++q) gbuf[((r + 1) & 1) * GROW + lane + 64 * q] = gnext[q];
      }
      __syncthreads();   // row r + 1 is in place for every lane; nobody reads row r any more
    }
  }
  __syncthreads();

  for (int rr = 0; rr < nrow; ++rr) {
    float* dst = p.f + (size_t)(row0 + rr) * rank;
    for (int c = lane; c < rank; c += 64) dst[c] = fs[c * kHalsPitch + rr];
  }
}

template <int R_PAD>
static int launch_hals(const HalsArgs& a, hipStream_t s) {
  return launch_with_dynamic_lds<hals_sweep_kernel<R_PAD>, 64, hals_lds_bytes(R_PAD)>(dim3((unsigned)((a.rows + 63) / 64)), s, a);
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_hals_sweep(float* f, int rows, int rank, const float* a, int64_t lda, const float* gram, float l1, float l2,
                     void* stream) {
  if (!f || !a || !gram || rows <= 0 || rank <= 0 || lda < rank) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const HalsArgs args{f, a, gram, lda, rows, rank, l1, l2};
  if (rank <= 32) return launch_hals<32>(args, s);
  if (rank <= 64) return launch_hals<64>(args, s);
  if (rank <= 128) return launch_hals<128>(args, s);
  return launch_hals<256>(args, s);
}

}  // extern "C"
