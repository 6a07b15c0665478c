// The NTF half-step of nmfmu_ntf.hip on a tile for SHORT owner modes: a workgroup owns 32 owner rows x a rank tile of <= 128 x
// one part of the contraction axis, and its WS waves lie ALONG THE CONTRACTION.  A stage is 32 WS flat steps; wave w takes
// steps [32 w, 32 w + 32) of it.  Every wave holds the same 32 owner rows as its A operand, so with <= 32 rows in the mode no
// wave multiplies padding rows only (the 128-row tile leaves three of its four waves doing that).  Same arithmetic, same
// contracts, same slab and finishing kernel as the wide tile; the stage loop is written out here (nmfmu_wmu_tile.h says why).
//
// Per wave and stage, all in the wave's own LDS (no wave reads another's):
//   * panel: the wave's 32 Khatri-Rao rows sb [c][r] = fl32(Pa[a][r] Pb[b][r]) over the full padded rank.  r_pad <= 128: Pa[a]
//     and Pb[b] are fetched one stage ahead (r_pad / 2 registers each) and multiplied on the way into LDS.  r_pad 256: the
//     registers go to the owner rows and the accumulators, the panel is fetched in the stage, 4 rows at a time.
//   * the slice table: lane l & 31 divides once, a = (c + l) / nB for the wave's own 32 steps -- one table per wave.
//   * V and M go STRAIGHT into the accumulator layout of Y, one stage ahead, never through LDS: lane (j, hl) holds step j and
//     rows (e & 3) + 8 (e >> 2) + 4 hl.  INNER walk (modes 0, 1): 16 scalar loads, the 32 lanes of a row contiguous along b
//     inside a slice (128-byte runs, broken where a slice ends; the lane's own table entry is its slice).  OUTER walk (mode 2):
//     the lane's four rows of a quad are contiguous, one 16-byte load per quad where it lies inside the tensor and K % 4 == 0
//     and the bases are aligned, else scalar loads.  Rows past the mode are never loaded: 4 loads instead of 16 at 8 rows.
//   * Y = owner x panel (wmu_form_y), both seeds in the accumulator layout (masked_g), through sn / sd [i][c] into the A
//     layout, num and den accumulated over the wave's rank tile with v_mfma_f32_32x32x2f32.
// End of a part: waves 1 .. WS-1 hand their accumulators to wave 0 through LDS in wave order (plain stores, barriers), wave 0
// stores the part's planes to the slab [part][num | den][rows][r_pad].  No atomics, no fences.
//
//   r_pad   WS  threads  LDS bytes (WS x (32 (r_pad + 1) + 2 x 32 x 33) x 4)   workgroups / waves per CU by LDS (160 KB)
//     32     4    256     50688                                                 3 / 12
//     64     4    256     67072                                                 2 /  8
//    128     2    128     49920                                                 3 /  6
//    256     1     64     41344                                                 3 /  3
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_launch.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_ntf_host.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

constexpr int kNsRows = 32;                  // owner rows per workgroup
constexpr int kNsTileC0 = 65536;             // the automatic rule: <= 32 rows contracting over at least this many steps

// waves along the contraction (and with them the stage length 32 WS) per padded rank
constexpr int ntf_short_waves(int r_pad) { return r_pad <= 64 ? 4 : r_pad == 128 ? 2 : 1; }

template <int RP>
struct NtfShortCfg {
  static constexpr int WS = ntf_short_waves(RP);
  static constexpr int RT = WmuCfg<RP>::RT;          // rank tile of the two accumulators (grid.y)
  static constexpr int TN = RT / 32;                 // 32 x 32 tiles per wave along the rank
  static constexpr int LDB = WmuCfg<RP>::LDB;
  static constexpr bool AHEAD = RP <= 128;           // the panel rows travel one stage ahead in registers
  static constexpr int PR = AHEAD ? kWmBK : 4;       // panel rows per register chunk
  static constexpr int NP = PR * RP / 64;            // registers of a chunk, for Pa and for Pb
  static constexpr int WAVE_FLOATS = kWmBK * LDB + 2 * kNsRows * kWmLDA;      // sb, sn, sd
  static constexpr int LDS_BYTES = WS * WAVE_FLOATS * 4;
  static_assert(WS == 1 || TN * 2 * 16 * 64 <= WS * WAVE_FLOATS, "the hand-over of a wave's accumulators fits the LDS");
};

// ---- the split: parts of whole stages of `stage` = 32 WS steps ------------------------------------------------------------------
inline int ntf_short_stage(int r_pad) { return kWmBK * ntf_short_waves(r_pad); }
inline int ntf_short_stages(int contraction, int r_pad) {
  const int stage = ntf_short_stage(r_pad);
  return (contraction + stage - 1) / stage;
}
// parts for a wanted split count >= 1: no empty part, only the last one may be short
inline int ntf_short_parts(int contraction, int r_pad, int nsplit) {
  const int stages = ntf_short_stages(contraction, r_pad);
  const int n = std::max(1, std::min(nsplit, stages));
  const int per = (stages + n - 1) / n;
  return (stages + per - 1) / per;
}
inline int ntf_short_part_len(int contraction, int r_pad, int parts) {
  return (ntf_short_stages(contraction, r_pad) + parts - 1) / parts * ntf_short_stage(r_pad);
}
inline int ntf_short_auto_split(int rows, int contraction, int r_pad) {
  const int64_t tiles = (int64_t)((rows + kNsRows - 1) / kNsRows) * ((r_pad + 127) / 128);
  const int64_t want = (kNtfTargetWgs + tiles - 1) / tiles;
  const int cap = std::max(1, ntf_short_stages(contraction, r_pad) / kWmMinStages);
  return ntf_short_parts(contraction, r_pad, (int)std::min<int64_t>(want, cap));
}
inline int ntf_short_split(int rows, int contraction, int r_pad, int nsplit) {
  return nsplit > 0 ? ntf_short_parts(contraction, r_pad, nsplit) : ntf_short_auto_split(rows, contraction, r_pad);
}

struct NtfShortArgs {
  const float *V, *M;
  int64_t sO, sA;
  int rows, nB, C;
  const float *owner, *Pa, *Pb;
  int rank;
  float beta;
  int part_len;
  float *on, *od;      // + part * pstride: the part's planes [rows][RP]
  int64_t pstride;
};

// the slice table of the wave's 32 steps from wc: lane l & 31 holds a = (wc + l) / nB (0 past the part).  Called by every lane.
__device__ __forceinline__ int ntfs_slices(int wc, int cend, int nB, int lane) {
  const int c = wc + (lane & 31);
  return c < cend ? c / nB : 0;
}

// bv / bw = Pa[a] / Pb[b] of the PR steps from wc + d0 over the full padded rank; zero in the padded columns and past the part
template <int RP, int PR>
__device__ __forceinline__ void ntfs_load_panel(float (&bv)[PR * RP / 64], float (&bw)[PR * RP / 64], const NtfShortArgs& p,
                                                int wc, int cend, int atab, int d0, int lane) {
#pragma unroll
  for (int q = 0; q < PR * RP / 64; ++q) {
    const int idx = q * 64 + lane;
    const int d = d0 + idx / RP, r = idx % RP, c = wc + d;
    const int a = __shfl(atab, d, 64), b = c - a * p.nB;
    const bool ok = c < cend && r < p.rank;
    bv[q] = ok ? p.Pa[(size_t)a * p.rank + r] : 0.f;
    bw[q] = ok ? p.Pb[(size_t)b * p.rank + r] : 0.f;
  }
}

// sb [c][r] = fl32(Pa[a][r] Pb[b][r]): the wave's Khatri-Rao rows, formed here and nowhere else
template <int RP, int PR>
__device__ __forceinline__ void ntfs_store_panel(float* sb, const float (&bv)[PR * RP / 64], const float (&bw)[PR * RP / 64],
                                                 int d0, int lane) {
#pragma unroll
  for (int q = 0; q < PR * RP / 64; ++q) {
    const int idx = q * 64 + lane;
    sb[(d0 + idx / RP) * WmuCfg<RP>::LDB + idx % RP] = bv[q] * bw[q];
  }
}

// vv / mm [e] = V / M at (owner row i0 + wmu_tile_row(e, hl), step wc + j): the accumulator layout of Y.  Zero outside the
// tensor and the part (m = 0: selected away); m = 1 inside when M is NULL.  atab: the lane's own entry is the slice of its step.
template <bool OUTER>
__device__ __forceinline__ void ntfs_load_vm(float (&vv)[16], float (&mm)[16], const NtfShortArgs& p, int i0, int wc, int cend,
                                             int atab, bool al, int j, int hl) {
  const bool has_m = p.M != nullptr;
  const int c = wc + j;
#pragma unroll
  for (int e = 0; e < 16; ++e) vv[e] = mm[e] = 0.f;
  if (c >= cend) return;
  if constexpr (OUTER) {
    // V[c sA + i ..]: the four rows of a quad are contiguous
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 8 * q + 4 * hl, left = p.rows - i;
      const size_t off = (size_t)c * p.sA + i;
      if (left >= 4 && al && (p.sA & 3) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(p.V + off);
        vv[4 * q] = v.x, vv[4 * q + 1] = v.y, vv[4 * q + 2] = v.z, vv[4 * q + 3] = v.w;
        if (has_m) {
          const float4 m = *reinterpret_cast<const float4*>(p.M + off);
          mm[4 * q] = m.x, mm[4 * q + 1] = m.y, mm[4 * q + 2] = m.z, mm[4 * q + 3] = m.w;
        } else {
          mm[4 * q] = mm[4 * q + 1] = mm[4 * q + 2] = mm[4 * q + 3] = 1.f;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < left) {
            vv[4 * q + t] = p.V[off + t];
            mm[4 * q + t] = has_m ? p.M[off + t] : 1.f;
          }
      }
    }
  } else {
    // V[i sO + a sA + b]: the 32 lanes of a row are contiguous along b inside a slice
    const size_t at = (size_t)atab * p.sA + (c - atab * p.nB);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + wmu_tile_row(e, hl);
      if (i < p.rows) {
        const size_t off = (size_t)i * p.sO + at;
        vv[e] = p.V[off];
        mm[e] = has_m ? p.M[off] : 1.f;
      }
    }
  }
}

// grid = (32-row tiles, rank tiles, parts), 64 WS threads, NtfShortCfg<RP>::LDS_BYTES of dynamic LDS
// r_pad 32: two waves per SIMD (256 registers each), so that one workgroup's barrier is another's MFMA time; from r_pad 64
// the stage registers need the whole file (one wave per SIMD), and r_pad 256 still spills a few dozen of them
template <int RP, bool OUTER, int KIND>
__global__ void __launch_bounds__(64 * NtfShortCfg<RP>::WS) __attribute__((amdgpu_waves_per_eu(RP <= 32 ? 2 : 1)))
ntf_short_kernel(const NtfShortArgs p) {
  using K = NtfShortCfg<RP>;
  extern __shared__ __attribute__((aligned(16))) float ns_lds[];
  const int lane = threadIdx.x & 63, j = lane & 31, hl = lane >> 5, wave = threadIdx.x >> 6;
  float* sb = ns_lds + wave * K::WAVE_FLOATS;      // the wave's own panel rows and seed tiles
  float* sn = sb + kWmBK * K::LDB;
  float* sd = sn + kNsRows * kWmLDA;
  const int i0 = blockIdx.x * kNsRows, r0 = blockIdx.y * K::RT;
  const int cbeg = blockIdx.z * p.part_len, cend = min(p.C, cbeg + p.part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, p.owner, p.rows, p.rank, i0 + j, hl);
  f32x16 accn[K::TN], accd[K::TN];
#pragma unroll
  for (int b = 0; b < K::TN; ++b)
#pragma unroll
    for (int e = 0; e < 16; ++e) accn[b][e] = accd[b][e] = 0.f;
  const bool al = ((reinterpret_cast<uintptr_t>(p.V) | reinterpret_cast<uintptr_t>(p.M)) & 15) == 0;
  float vv[16], mm[16], bv[K::NP], bw[K::NP];
  {
    const int wc = cbeg + wave * kWmBK;
    const int atab = ntfs_slices(wc, cend, p.nB, lane);
    ntfs_load_vm<OUTER>(vv, mm, p, i0, wc, cend, atab, al, j, hl);
    if constexpr (K::AHEAD) ntfs_load_panel<RP, K::PR>(bv, bw, p, wc, cend, atab, 0, lane);
  }
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK * K::WS) {
    const int wc = c0 + wave * kWmBK;      // the wave's 32 steps of this stage; past the part for the last waves of a tail
    if constexpr (K::AHEAD) {
      ntfs_store_panel<RP, K::PR>(sb, bv, bw, 0, lane);
    } else {
      const int atab = ntfs_slices(wc, cend, p.nB, lane);
#pragma unroll
      for (int d0 = 0; d0 < kWmBK; d0 += K::PR) {
        ntfs_load_panel<RP, K::PR>(bv, bw, p, wc, cend, atab, d0, lane);
        ntfs_store_panel<RP, K::PR>(sb, bv, bw, d0, lane);
      }
    }
    __syncthreads();
    const bool more = c0 + kWmBK * K::WS < cend;
    const int nc = wc + kWmBK * K::WS;
    const int ntab = more ? ntfs_slices(nc, cend, p.nB, lane) : 0;
    // the next stage's panel rows travel behind all of this stage's MFMAs ...
    if constexpr (K::AHEAD)
      if (more) ntfs_load_panel<RP, K::PR>(bv, bw, p, nc, cend, ntab, 0, lane);
    const bool busy = wc < cend;           // wave-uniform; the barriers stay outside
    if (busy) {
      const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
      // m g_neg, m g_pos in the accumulator layout, stored [i][c] for the A operand of the second product
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float gn, gp;
        masked_g<KIND>(vv[e], y[e], p.beta, gn, gp);
        const bool w = mm[e] > 0.f;
        const int at = wmu_tile_row(e, hl) * kWmLDA + j;
        sn[at] = w ? mm[e] * gn : 0.f;
        sd[at] = w ? mm[e] * gp : 0.f;
      }
    }
    // ... its V and M, in the registers the seeds just left, behind the second product
    if (more) ntfs_load_vm<OUTER>(vv, mm, p, i0, nc, cend, ntab, al, j, hl);
    __syncthreads();
    if (busy) {
      const float* pn = sn + j * kWmLDA + hl;
      const float* pd = sd + j * kWmLDA + hl;
      const float* pb = sb + hl * K::LDB + r0 + j;
#pragma unroll
      for (int s2 = 0; s2 < kWmBK; s2 += 2) {
        const float gn = pn[s2], gp = pd[s2];
#pragma unroll
        for (int b = 0; b < K::TN; ++b) {
          const float bb = pb[s2 * K::LDB + b * 32];
          accn[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gn, bb, accn[b], 0, 0, 0);
          accd[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp, bb, accd[b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // the part's sum over its waves, in wave order: wave w hands over, wave 0 adds
  if constexpr (K::WS > 1) {
    for (int w = 1; w < K::WS; ++w) {
      if (wave == w) {
#pragma unroll
        for (int b = 0; b < K::TN; ++b)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            ns_lds[((b * 2 + 0) * 16 + e) * 64 + lane] = accn[b][e];
            ns_lds[((b * 2 + 1) * 16 + e) * 64 + lane] = accd[b][e];
          }
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int b = 0; b < K::TN; ++b)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            accn[b][e] += ns_lds[((b * 2 + 0) * 16 + e) * 64 + lane];
            accd[b][e] += ns_lds[((b * 2 + 1) * 16 + e) * 64 + lane];
          }
      }
      __syncthreads();
    }
  }
  if (wave != 0) return;
  float* pn = p.on + (size_t)blockIdx.z * p.pstride;
  float* pd = p.od + (size_t)blockIdx.z * p.pstride;
#pragma unroll
  for (int b = 0; b < K::TN; ++b) {
    const int r = r0 + b * 32 + j;      // < RP: the rank tiles cover the padded rank exactly
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + wmu_tile_row(e, hl);
      if (i < p.rows) {
        pn[(size_t)i * RP + r] = r < p.rank ? accn[b][e] : 0.f;
        pd[(size_t)i * RP + r] = r < p.rank ? accd[b][e] : 0.f;
      }
    }
  }
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
int ntf_short_launch(const float* V, const float* M, int I, int J, int K, int mode, float* owner, const float* pa,
                     const float* pb, int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den, int step,
                     MaskedApply ap, hipStream_t st) {
  const NtfMode md = ntf_mode(I, J, K, mode);
  const int rows = md.rows, contraction = md.nA * md.nB;
  const int parts = ntf_short_split(rows, contraction, r_pad, nsplit);
  WmuSlab sl = wmu_slab(1, rows, r_pad, parts, step, ws, num, den);
  sl.grid.x = (rows + kNsRows - 1) / kNsRows;
  const NtfShortArgs a{V, M, md.sO, md.sA, rows, md.nB, contraction, owner, pa, pb, rank, beta,
                       ntf_short_part_len(contraction, r_pad, parts), sl.on, sl.od, sl.pstride};
  int rc = 0;
  for_rp(r_pad, [&](auto rp) {
    for_kind(nmfmu_beta_kind(beta), [&](auto k) {
      constexpr int RP = decltype(rp)::value, KIND = decltype(k)::value;
      using C = NtfShortCfg<RP>;
      rc = md.outer ? launch_with_dynamic_lds<ntf_short_kernel<RP, true, KIND>, 64 * C::WS, C::LDS_BYTES>(sl.grid, st, a)
                    : launch_with_dynamic_lds<ntf_short_kernel<RP, false, KIND>, 64 * C::WS, C::LDS_BYTES>(sl.grid, st, a);
    });
  });
  if (rc) return rc;
  if (!sl.direct) ntf_finish_launch(sl.fblocks, ws, parts, rows, rank, r_pad, owner, num, den, step, ap, st);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" {

int nmfmu_ntf_short_nsplit(int rows, int contraction, int r_pad) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0) return NMFMU_ERR_ARG;
  return ntf_short_split(rows, contraction, r_pad, 0);
}

int64_t nmfmu_ntf_short_ws(int rows, int contraction, int r_pad, int nsplit) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0 || nsplit < 0) return 0;
  return (int64_t)ntf_short_split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad;
}

int nmfmu_ntf_short_terms(const float* V, const float* M, int I, int J, int K, int mode, const float* owner, const float* pa,
                          const float* pb, int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den,
                          void* stream) {
  if (!ws || !num || !den || nsplit < 0) return NMFMU_ERR_ARG;
  if (const int rc = ntf_check(V, I, J, K, mode, owner, pa, pb, rank, r_pad, true, nsplit, ntf_short_split)) return rc;
  return ntf_short_launch(V, M, I, J, K, mode, const_cast<float*>(owner), pa, pb, rank, r_pad, beta, nsplit, ws, num, den, 0,
                          MaskedApply{0.f, 0.f, 1.f}, S(stream));
}

int nmfmu_ntf_short_step(const float* V, const float* M, int I, int J, int K, int mode, float* owner, const float* pa,
                         const float* pb, int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit, float* ws,
                         void* stream) {
  if (!ws || owner == pa || owner == pb || nsplit < 0) return NMFMU_ERR_ARG;
  if (const int rc = ntf_check(V, I, J, K, mode, owner, pa, pb, rank, r_pad, true, nsplit, ntf_short_split)) return rc;
  return ntf_short_launch(V, M, I, J, K, mode, owner, pa, pb, rank, r_pad, beta, nsplit, ws, nullptr, nullptr, 1,
                          MaskedApply{l1, l2, gamma}, S(stream));
}

int nmfmu_ntf_tile(int rows, int contraction, int r_pad) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0) return NMFMU_ERR_ARG;
  return rows <= kNsRows && contraction >= kNsTileC0 ? 1 : 0;
}

}  // extern "C"
