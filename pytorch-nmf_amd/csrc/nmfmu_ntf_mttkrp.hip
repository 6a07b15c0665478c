// The dense MTTKRP of a 3-way tensor: num[o][r] = sum_(a,b) V(o, a, b) Pa[a][r] Pb[b][r] of mode n, the numerator of a
// Frobenius (beta = 2) half-step of ntf.NTF -- HALS (solver='hals') needs it and two small Gram matrices, no reconstruction and
// no second contraction.  Modes, owner, the flat a-major contraction axis, (Pa, Pb) and the three address formulas are those of
// nmfmu_ntf.hip's header comment; p[r] = fl32(Pa[a][r] Pb[b][r]) (one rounding), exact fp32 on v_mfma_f32_32x32x2f32.
//
// A kernel of its own, not the fused tile with a stage removed:
//
//   * V NEVER PASSES THROUGH LDS.  A value of V is needed once, as the A operand of one MFMA, so it is loaded from global
//     memory straight into the A layout of the 32 x 32 x 2 instruction: lane l holds owner row l & 31 and contraction step
//     l >> 5 of the pair.  A wave's run is 32 flat steps = 16 MFMA pairs, fetched one stage ahead into 16 registers.
//       OUTER walk (mode 2, owner contiguous): pair m is steps (2 m, 2 m + 1); the 32 lanes of a half make one 128-byte line.
//       INNER walk (modes 0 and 1, contraction contiguous): the order of the 32 steps is free, so lane half hl takes the four
//       quads of steps 8 q + 4 hl .. + 3 and pair m = 4 q + t is steps (8 q + t, 8 q + 4 + t): a quad is one 16-byte load
//       where it lies in one slice, inside the part and 16-byte aligned (decided per quad, as ntf_load_vm does), else four
//       scalar loads each with its own slice; either way its four values feed four MFMAs without a cross-lane move.  The
//       panel operand is read from LDS at the matching rows.
//   * ONLY THE KHATRI-RAO ROWS LIVE IN LDS, sb [step][r_pad], 32 rows per run, formed from Pa and Pb with the slice table of
//     nmfmu_ntf.hip (lane l & 31 divides once per run, everything else is a shuffle and a multiply), fetched one stage ahead
//     and multiplied on their way into LDS.  The B operand reads one row of sb per lane half: no padding of the rows.
//   * A WAVE CARRIES THE WHOLE PADDED RANK: r_pad / 32 accumulators of 32 x 32 (8 at r_pad 256: 128 registers, the unified
//     file of one wave per SIMD holds them), so V is read from HBM once at every rank.
//   * TWO WAVE ARRANGEMENTS, one template.  WIDE: the four waves own 4 x 32 = 128 consecutive owner rows and share each
//     32-step stage of sb.  SHORT: all four waves own the same 32 owner rows, a stage is 128 steps and wave w takes the run
//     [32 w, 32 w + 32) with its own rows of sb; at the end of the part waves 1 .. 3 hand their accumulators to wave 0
//     through LDS and wave 0 adds them in wave order.  Either is correct for any number of rows.
//   * the panel fetch is one stage ahead while it fits 2 x 32 registers per thread (WIDE: every rank; SHORT: r_pad <= 64);
//     SHORT at r_pad 128 / 256 fetches its run 16 / 8 rows at a time inside the stage, as nmfmu_ntf_short.hip does at 256.
//
// The contraction is cut into parts of whole stages; every part stores its plane to the slab [part][rows][r_pad] with plain
// stores and mk_finish_kernel adds them in part order (one part: the kernel's plane is the result).  No atomics, no fences: a
// repeated call is bitwise identical whatever ws and num held.  Rows past the tensor and steps past the part load as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_launch.h"
#include "nmfmu_ntf_host.h"
#include "nmfmu_ntf_mttkrp.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

template <int RP, bool SHORT>
struct MkCfg {
  static constexpr int NT = RP / 32;                          // 32 x 32 accumulators per wave: the whole padded rank
  static constexpr int STAGE = SHORT ? 4 * kWmBK : kWmBK;     // flat steps per stage
  static constexpr int ROWS = SHORT ? 32 : kWmRows;           // owner rows per workgroup
  static constexpr int LT = SHORT ? 64 : 256;                 // threads that load one 32-row run of the panel
  static constexpr int NP = kWmBK * RP / LT < 32 ? kWmBK * RP / LT : 32;      // registers of a chunk, for Pa and for Pb
  static constexpr int PR = NP * LT / RP;                     // panel rows per chunk
  static constexpr bool AHEAD = PR == kWmBK;                  // the run's rows travel one stage ahead in registers
  static constexpr int LDS_BYTES = STAGE * RP * 4;
};

// bv / bw = Pa[a] / Pb[b] of the PR steps from wc + d0 over the full padded rank; zero in the padded columns and past the part.
// lt: the thread's index among the LT threads that load this run.
template <int RP, bool SHORT, int NP>
__device__ __forceinline__ void mk_load_panel(float (&bv)[NP], float (&bw)[NP], const MkArgs& p, int wc, int cend, int atab,
                                              int d0, int lt) {
  using K = MkCfg<RP, SHORT>;
#pragma unroll
  for (int q = 0; q < K::NP; ++q) {
    const int idx = q * K::LT + lt;
    const int d = d0 + idx / RP, r = idx % RP, c = wc + d;
    const int a = __shfl(atab, d, 64), b = c - a * p.nB;
    const bool ok = c < cend && r < p.rank;
    bv[q] = ok ? p.Pa[(size_t)a * p.rank + r] : 0.f;
    bw[q] = ok ? p.Pb[(size_t)b * p.rank + r] : 0.f;
  }
}

// sb [d][r] = fl32(Pa[a][r] Pb[b][r]): the Khatri-Rao rows of the run, formed here and nowhere else
template <int RP, bool SHORT, int NP>
__device__ __forceinline__ void mk_store_panel(float* sb, const float (&bv)[NP], const float (&bw)[NP], int d0, int lt) {
  using K = MkCfg<RP, SHORT>;
#pragma unroll
  for (int q = 0; q < K::NP; ++q) sb[d0 * RP + q * K::LT + lt] = bv[q] * bw[q];
}

// the sb row that lane half hl multiplies in MFMA pair m of the run
template <bool OUTER>
__device__ __forceinline__ constexpr int mk_pair_row(int m, int hl) {
  return OUTER ? 2 * m + hl : 8 * (m >> 2) + 4 * hl + (m & 3);
}

// vv[m] = V at (owner row i, step wc + mk_pair_row(m, hl)): the A operands of the run's 16 MFMA pairs.  Zero outside the
// tensor and the part.
template <bool OUTER>
__device__ __forceinline__ void mk_load_v(float (&vv)[16], const MkArgs& p, int i, int wc, int cend, int atab, bool al, int hl) {
#pragma unroll
  for (int m = 0; m < 16; ++m) vv[m] = 0.f;
  if constexpr (OUTER) {
    // V[c sA + i]: the 32 lanes of a half are contiguous along the owner
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int c = wc + 2 * m + hl;
      if (c < cend && i < p.rows) vv[m] = p.V[(size_t)c * p.sA + i];
    }
  } else {
    // V[i sO + a sA + b ..]: a quad of the lane's row, contiguous along b inside a slice
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = 8 * q + 4 * hl, c = wc + d;
      int a[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = __shfl(atab, d + t, 64);      // by every lane: outside the branches
      if (c < cend && i < p.rows) {
        const int left = cend - c;
        const size_t off = (size_t)i * p.sO + (size_t)a[0] * p.sA + (c - a[0] * p.nB);
        if (left >= 4 && al && a[3] == a[0] && (off & 3) == 0) {
          const float4 v = *reinterpret_cast<const float4*>(p.V + off);
          vv[4 * q] = v.x, vv[4 * q + 1] = v.y, vv[4 * q + 2] = v.z, vv[4 * q + 3] = v.w;
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t < left) vv[4 * q + t] = p.V[(size_t)i * p.sO + (size_t)a[t] * p.sA + (c + t - a[t] * p.nB)];
        }
      }
    }
  }
}

// grid = (row tiles of MkCfg::ROWS, 1, parts), 256 threads, MkCfg::LDS_BYTES of dynamic LDS
template <int RP, bool OUTER, bool SHORT>
__global__ void __launch_bounds__(256) mk_kernel(const MkArgs p) {
  using K = MkCfg<RP, SHORT>;
  extern __shared__ __attribute__((aligned(16))) float mk_lds[];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  float* sb = mk_lds + (SHORT ? wave * kWmBK * RP : 0);      // the rows of the wave's run
  const int lt = SHORT ? lane : tid;
  const int i = blockIdx.x * K::ROWS + (SHORT ? 0 : wave * 32) + j;      // the lane's owner row
  const int cbeg = blockIdx.z * p.part_len, cend = min(p.C, cbeg + p.part_len);
  const int woff = SHORT ? wave * kWmBK : 0;                 // the wave's run inside a stage
  f32x16 acc[K::NT];
#pragma unroll
  for (int b = 0; b < K::NT; ++b)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;
  const bool al = (reinterpret_cast<uintptr_t>(p.V) & 15) == 0;
  float vv[16], vn[16], bv[K::NP], bw[K::NP];
  {
    const int atab = mk_slices(cbeg + woff, cend, p.nB, lane);
    mk_load_v<OUTER>(vv, p, i, cbeg + woff, cend, atab, al, hl);
    if constexpr (K::AHEAD) mk_load_panel<RP, SHORT, K::NP>(bv, bw, p, cbeg + woff, cend, atab, 0, lt);
  }
  for (int c0 = cbeg; c0 < cend; c0 += K::STAGE) {
    const int wc = c0 + woff;      // past the part for the last waves of a SHORT tail: zeros everywhere
    if constexpr (K::AHEAD) {
      mk_store_panel<RP, SHORT, K::NP>(sb, bv, bw, 0, lt);
    } else {
      const int atab = mk_slices(wc, cend, p.nB, lane);
#pragma unroll
      for (int d0 = 0; d0 < kWmBK; d0 += K::PR) {
        mk_load_panel<RP, SHORT, K::NP>(bv, bw, p, wc, cend, atab, d0, lt);
        mk_store_panel<RP, SHORT, K::NP>(sb, bv, bw, d0, lt);
      }
    }
    __syncthreads();
    // the next stage's loads travel behind this stage's MFMAs
    const bool more = c0 + K::STAGE < cend;
    if (more) {
      const int ntab = mk_slices(wc + K::STAGE, cend, p.nB, lane);
      mk_load_v<OUTER>(vn, p, i, wc + K::STAGE, cend, ntab, al, hl);
      if constexpr (K::AHEAD) mk_load_panel<RP, SHORT, K::NP>(bv, bw, p, wc + K::STAGE, cend, ntab, 0, lt);
    }
    if (wc < cend) {      // wave-uniform; the barriers stay outside
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const float* pb = sb + mk_pair_row<OUTER>(m, hl) * RP + j;
#pragma unroll
        for (int b = 0; b < K::NT; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[m], pb[b * 32], acc[b], 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int m = 0; m < 16; ++m) vv[m] = vn[m];
    }
    __syncthreads();
  }
  // SHORT: the part's sum over its waves, in wave order.  A wave's accumulators are as many floats as its rows of sb.
  if constexpr (SHORT) {
    if (wave != 0) {
#pragma unroll
      for (int b = 0; b < K::NT; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) sb[(b * 16 + e) * 64 + lane] = acc[b][e];
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w)
#pragma unroll
      for (int b = 0; b < K::NT; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] += mk_lds[w * kWmBK * RP + (b * 16 + e) * 64 + lane];
  }
  float* out = p.out + (size_t)blockIdx.z * p.pstride;
  const int ibase = blockIdx.x * K::ROWS + (SHORT ? 0 : wave * 32);
#pragma unroll
  for (int b = 0; b < K::NT; ++b) {
    const int r = b * 32 + j;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = ibase + wmu_tile_row(e, hl);
      if (row < p.rows) out[(size_t)row * RP + r] = r < p.rank ? acc[b][e] : 0.f;
    }
  }
}

// The slab's parts added in part order.  There may be hundreds of parts over a small plane: the loads of 8 parts are issued
// together, the adds stay in part order.
__global__ void __launch_bounds__(256) mk_finish_kernel(const float* __restrict__ ws, int parts, int64_t plane,
                                                        float* __restrict__ num) {
  for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < plane; at += (int64_t)gridDim.x * 256) {
    float n = ws[at];
    int p = 1;
    for (; p + 8 <= parts; p += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = ws[(size_t)(p + u) * plane + at];
#pragma unroll
      for (int u = 0; u < 8; ++u) n += t[u];
    }
    for (; p < parts; ++p) n += ws[(size_t)p * plane + at];
    num[at] = n;
  }
}

void mk_finish_launch(const float* ws, int parts, int64_t plane, float* num, hipStream_t st) {
  hipLaunchKernelGGL(mk_finish_kernel, dim3((unsigned)std::min<int64_t>((plane + 255) / 256, kWmFinishBlocks)), dim3(256), 0, st, ws,
                     parts, plane, num);
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int64_t nmfmu_ntf_mttkrp_ws(int rows, int contraction, int r_pad, int nsplit, int tile) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0 || nsplit < 0 || tile < 0 || tile > 1) return 0;
  return (int64_t)mk_split(rows, contraction, r_pad, nsplit, tile) * rows * r_pad;
}

int nmfmu_ntf_mttkrp(const float* V, int I, int J, int K, int mode, const float* pa, const float* pb, int rank, int r_pad,
                     int nsplit, int tile, float* ws, float* num, void* stream) {
  MkPlan pl;
  if (const int rc = mk_plan(V, I, J, K, mode, pa, pb, rank, r_pad, nsplit, tile, ws, num, &pl)) return rc;
  const MkArgs& a = pl.a;
  const dim3 grid = pl.grid;
  int rc = 0;
  for_rp(r_pad, [&](auto rp) {
    constexpr int RP = decltype(rp)::value;
    auto go = [&](auto outer, auto shrt) {
      constexpr bool O = decltype(outer)::value, S = decltype(shrt)::value;
      rc = launch_with_dynamic_lds<mk_kernel<RP, O, S>, 256, MkCfg<RP, S>::LDS_BYTES>(grid, nmfmu::S(stream), a);
    };
    if (pl.outer)
      tile ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
    else
      tile ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
  });
  if (rc) return rc;
  if (pl.parts > 1) mk_finish_launch(ws, pl.parts, a.pstride, num, nmfmu::S(stream));
  return (int)hipGetLastError();
}

}  // extern "C"
