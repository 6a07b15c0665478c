// The dense MTTKRP of nmfmu_ntf_mttkrp.hip in split bf16 (precision='bf16x3'): num[o][r] = sum_(a,b) V(o, a, b) p(a, b)[r] with
// p[r] = fl32(Pa[a][r] Pb[b][r]), every V and every p held as two bf16 planes (hi = bf16(x), lo = bf16(x - hi), RNE) and a
// product formed by three v_mfma_f32_32x32x16_bf16 into an fp32 accumulator: lo hi, hi lo, hi hi in that order (the two small
// terms first); lo lo (at most 2^-18 of the product) is never formed.  Modes, owner, the flat a-major contraction, the slice
// table, the parts of whole stages and the slab [part][rows][r_pad] finished in part order are nmfmu_ntf_mttkrp.hip's
// (nmfmu_ntf_mttkrp.h); the data movement is not:
//
//   * V NEVER PASSES THROUGH LDS and is read once, as fp32.  The A operand of 32 x 32 x 16 gives lane l owner row l & 31 and
//     the eight consecutive steps 8 (l >> 5) .. + 7 of a 16-step run; a wave's 32-step run is two of them, so lane half hl
//     holds steps 16 u + 8 hl .. + 7 (u = 0, 1): 16 fp32 registers, fetched one stage ahead, split in registers into
//     4 + 4 packed registers per 16-step run right before the run's MFMAs.
//       INNER walk (modes 0 and 1): an octet is 32 contiguous bytes of the lane's row -- two 16-byte loads where a quad lies in
//       one slice, inside the part and 16-byte aligned (decided per quad), else scalar loads each with its own slice.
//       OUTER walk (mode 2): eight dword loads; the 32 lanes of a half make one 128-byte line.
//   * THE KHATRI-RAO ROWS LIVE IN LDS TRANSPOSED AND SPLIT: two bf16 planes [r][step] per 32-step run, so a lane's B operand
//     (column r = 32 b + (l & 31), steps 16 u + 8 hl .. + 7) is one 16-byte ds_read per plane.  A row is 64 bytes of steps and
//     the pitch is 80 bytes (20 banks): the 16 lanes a 16-byte LDS access serves together start at banks 20 j mod 64 =
//     {0, 20, 40, 60, 16, 36, 56, 12, 32, 52, 8, 28, 48, 4, 24, 44}, sixteen different multiples of 4, four banks each: all
//     64 banks once, for the reads (lane = row) and for the writes alike (thread = row, see below).  With 64-byte rows lanes j
//     and j + 4 would meet.
//   * A THREAD THAT FILLS THE PLANES OWNS ONE r AND ONE STEP OCTET: sixteen global loads (Pa[a][r], Pb[b][r] of its eight
//     steps, coalesced along r across the threads), eight products, one 16-byte write per plane.
//   * THE PLANES ARE DOUBLE-BUFFERED where the panel travels one stage ahead in registers, so a stage costs one workgroup
//     barrier: stage s writes buffer s & 1 after the barrier of stage s - 1, which every wave reaches only after its reads of
//     stage s - 2.  SHORT at r_pad 128 / 256 fills its planes inside the stage in 2 / 4 chunks (64 registers at a time) from a
//     single buffer with two barriers: two buffers of four waves would not fit the LDS.
//   * A WAVE CARRIES THE WHOLE PADDED RANK in r_pad / 32 accumulators; WIDE and SHORT are nmfmu_ntf_mttkrp.hip's arrangements
//     (four waves on 128 rows sharing a 32-step stage; four waves on the same 32 rows, a quarter of a 128-step stage each with
//     planes of their own, added through LDS in wave order).
//
// Plain stores, no atomics, no fences: a repeated call is bitwise identical whatever ws and num held.  Rows past the tensor and
// steps past the part load as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_launch.h"
#include "nmfmu_ntf_mttkrp.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

constexpr int kMxPitch = 2 * kWmBK + 16;      // bytes of a plane's row: 32 steps of bf16 and one 16-byte piece

template <int RP, bool SHORT>
struct MxCfg {
  static constexpr int NT = RP / 32;                          // 32 x 32 accumulators per wave: the whole padded rank
  static constexpr int STAGE = SHORT ? 4 * kWmBK : kWmBK;     // flat steps per stage
  static constexpr int ROWS = SHORT ? 32 : kWmRows;           // owner rows per workgroup
  static constexpr int LT = SHORT ? 64 : 256;                 // threads that fill the planes of one 32-step run
  static constexpr int PIECES = RP * kWmBK / 8;               // (r, step octet) pieces of a run
  static constexpr int NI = PIECES / LT < 1 ? 1 : PIECES / LT > 4 ? 4 : PIECES / LT;      // pieces of a thread per chunk: 2 x 8 registers each
  static constexpr int CHUNKS = PIECES / (NI * LT) < 1 ? 1 : PIECES / (NI * LT);
  static constexpr bool AHEAD = CHUNKS == 1;                  // the run's pieces travel one stage ahead in registers
  static constexpr int RUN_BYTES = 2 * RP * kMxPitch;         // the hi plane, then the lo plane
  static constexpr int NBUF = AHEAD ? 2 : 1;
  static constexpr int WAVE_BYTES = NBUF * RUN_BYTES;         // SHORT: a wave's planes; at the end its accumulators (RP * 128 bytes)
  static constexpr int LDS_BYTES = (SHORT ? 4 : 1) * WAVE_BYTES;
};

// pv / pw = Pa[a][r] / Pb[b][r] of the eight steps of the thread's pieces of chunk ch; zero in the padded columns, past the part
// and in the pieces past the run (WIDE at r_pad 32: half of the threads).  lt: the thread's index among the LT that fill this run.
template <int RP, bool SHORT, int NI>
__device__ __forceinline__ void mx_load_panel(float (&pv)[NI][8], float (&pw)[NI][8], const MkArgs& p, int wc, int cend, int atab,
                                              int ch, int lt) {
  using K = MxCfg<RP, SHORT>;
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int idx = (ch * NI + q) * K::LT + lt;
    const int r = idx % RP, oct = idx / RP;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = 8 * oct + e, c = wc + d;
      const int a = __shfl(atab, d & 31, 64), b = c - a * p.nB;      // by every lane: outside the branches
      const bool ok = oct < 4 && c < cend && r < p.rank;
      pv[q][e] = ok ? p.Pa[(size_t)a * p.rank + r] : 0.f;
      pw[q][e] = ok ? p.Pb[(size_t)b * p.rank + r] : 0.f;
    }
  }
}

// hi / lo of eight fp32 values as the eight bf16 of one MFMA operand register quad: element e in bits 16 (e & 1) of word e >> 1
__device__ __forceinline__ void mx_split(const float (&x)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    hi[w] = pack_bf16(x[2 * w], x[2 * w + 1]);
    lo[w] = pack_bf16(x[2 * w] - bf16_lo(hi[w]), x[2 * w + 1] - bf16_hi(hi[w]));
  }
}

// planes [r][oct] = split(fl32(Pa[a][r] Pb[b][r])): the Khatri-Rao rows of the run, formed here and nowhere else
template <int RP, bool SHORT, int NI>
__device__ __forceinline__ void mx_store_panel(char* buf, const float (&pv)[NI][8], const float (&pw)[NI][8], int ch, int lt) {
  using K = MxCfg<RP, SHORT>;
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int idx = (ch * NI + q) * K::LT + lt;
    const int r = idx % RP, oct = idx / RP;
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = __fmul_rn(pv[q][e], pw[q][e]);      // one rounding: never contracted into the lo subtraction
    u32x4 hi, lo;
    mx_split(t, hi, lo);
    if (oct < 4) {
      *reinterpret_cast<u32x4*>(buf + r * kMxPitch + oct * 16) = hi;
      *reinterpret_cast<u32x4*>(buf + (RP + r) * kMxPitch + oct * 16) = lo;
    }
  }
}

// vv[8 u + e] = V at (owner row i, step wc + 16 u + 8 hl + e): the A operands of the run's two 16-step MFMA runs.  Zero outside
// the tensor and the part.
template <bool OUTER>
__device__ __forceinline__ void mx_load_v(float (&vv)[16], const MkArgs& p, int i, int wc, int cend, int atab, bool al, int hl) {
#pragma unroll
  for (int m = 0; m < 16; ++m) vv[m] = 0.f;
  if constexpr (OUTER) {
    // V[c sA + i]: the 32 lanes of a half are contiguous along the owner
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int c = wc + 16 * (m >> 3) + 8 * hl + (m & 7);
      if (c < cend && i < p.rows) vv[m] = p.V[(size_t)c * p.sA + i];
    }
  } else {
    // V[i sO + a sA + b ..]: the two quads of an octet of the lane's row, contiguous along b inside a slice
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = 16 * (q >> 1) + 8 * hl + 4 * (q & 1), c = wc + d;
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

// grid = (row tiles of MxCfg::ROWS, 1, parts), 256 threads, MxCfg::LDS_BYTES of dynamic LDS
template <int RP, bool OUTER, bool SHORT>
__global__ void __launch_bounds__(256) mx_kernel(const MkArgs p) {
  using K = MxCfg<RP, SHORT>;
  extern __shared__ __attribute__((aligned(16))) char mx_lds[];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  char* planes = mx_lds + (SHORT ? wave * K::WAVE_BYTES : 0);      // the planes of the wave's run
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
  float vv[16], vn[16], pv[K::NI][8], pw[K::NI][8];
  {
    const int atab = mk_slices(cbeg + woff, cend, p.nB, lane);
    mx_load_v<OUTER>(vv, p, i, cbeg + woff, cend, atab, al, hl);
    if constexpr (K::AHEAD) mx_load_panel<RP, SHORT, K::NI>(pv, pw, p, cbeg + woff, cend, atab, 0, lt);
  }
  int flip = 0;
  for (int c0 = cbeg; c0 < cend; c0 += K::STAGE) {
    const int wc = c0 + woff;      // past the part for the last waves of a SHORT tail: zeros everywhere
    char* buf = planes + (K::NBUF == 2 ? flip * K::RUN_BYTES : 0);
    if constexpr (K::AHEAD) {
      mx_store_panel<RP, SHORT, K::NI>(buf, pv, pw, 0, lt);
    } else {
      const int atab = mk_slices(wc, cend, p.nB, lane);
#pragma unroll
      for (int ch = 0; ch < K::CHUNKS; ++ch) {
        mx_load_panel<RP, SHORT, K::NI>(pv, pw, p, wc, cend, atab, ch, lt);
        mx_store_panel<RP, SHORT, K::NI>(buf, pv, pw, ch, lt);
      }
    }
    __syncthreads();
    // the next stage's loads travel behind this stage's MFMAs
    const bool more = c0 + K::STAGE < cend;
    if (more) {
      const int ntab = mk_slices(wc + K::STAGE, cend, p.nB, lane);
      mx_load_v<OUTER>(vn, p, i, wc + K::STAGE, cend, ntab, al, hl);
      if constexpr (K::AHEAD) mx_load_panel<RP, SHORT, K::NI>(pv, pw, p, wc + K::STAGE, cend, ntab, 0, lt);
    }
    if (wc < cend) {      // wave-uniform; the barriers stay outside
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = vv[8 * u + e];
        u32x4 ah, alo;
        mx_split(x, ah, alo);
        const char* pb = buf + j * kMxPitch + 32 * u + 16 * hl;
#pragma unroll
        for (int b = 0; b < K::NT; ++b) {
          const u32x4 bh = ld16(pb + b * 32 * kMxPitch), bl = ld16(pb + (RP + b * 32) * kMxPitch);
          acc[b] = mfma_bf16(alo, bh, acc[b]);
          acc[b] = mfma_bf16(ah, bl, acc[b]);
          acc[b] = mfma_bf16(ah, bh, acc[b]);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int m = 0; m < 16; ++m) vv[m] = vn[m];
    }
    if constexpr (K::NBUF == 2)
      flip ^= 1;
    else
      __syncthreads();
  }
  // SHORT: the part's sum over its waves, in wave order, through the waves' own planes (read by no other wave before)
  if constexpr (SHORT) {
    float* sw = reinterpret_cast<float*>(planes);
    if (wave != 0) {
#pragma unroll
      for (int b = 0; b < K::NT; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) sw[(b * 16 + e) * 64 + lane] = acc[b][e];
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w)
#pragma unroll
      for (int b = 0; b < K::NT; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] += reinterpret_cast<const float*>(mx_lds + w * K::WAVE_BYTES)[(b * 16 + e) * 64 + lane];
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

}  // namespace nmfmu

using namespace nmfmu;

extern "C" int nmfmu_ntf_mttkrp_x3(const float* V, int I, int J, int K, int mode, const float* pa, const float* pb, int rank,
                                   int r_pad, int nsplit, int tile, float* ws, float* num, void* stream) {
  MkPlan pl;
  if (const int rc = mk_plan(V, I, J, K, mode, pa, pb, rank, r_pad, nsplit, tile, ws, num, &pl)) return rc;
  int rc = 0;
  for_rp(r_pad, [&](auto rp) {
    constexpr int RP = decltype(rp)::value;
    auto go = [&](auto outer, auto shrt) {
      constexpr bool O = decltype(outer)::value, S = decltype(shrt)::value;
      rc = launch_with_dynamic_lds<mx_kernel<RP, O, S>, 256, MxCfg<RP, S>::LDS_BYTES>(pl.grid, nmfmu::S(stream), pl.a);
    };
    if (pl.outer)
      tile ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
    else
      tile ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
  });
  if (rc) return rc;
  if (pl.parts > 1) mk_finish_launch(ws, pl.parts, pl.a.pstride, num, nmfmu::S(stream));
  return (int)hipGetLastError();
}
