// Non-negative CP (PARAFAC) factorisation of a 3-way tensor, V[i][j][k] ~ sum_r A[i][r] B[j][r] C[k][r], by the
// beta-divergence multiplicative update: L = sum m d_beta(v | y), m an optional dense weight tensor of V's shape.  A half-step
// of mode n updates one factor (the owner); its contraction axis is the flat pair (a, b), a-major, over the other two modes and
// its panel row at step (a, b) is the Khatri-Rao row p[r] = fl32(Pa[a][r] Pb[b][r]):
//
//   num[o][r] = sum_(a,b) (m g_neg(v, y))(o, a, b) p[r]      den[o][r] = sum_(a,b) (m g_pos(y))(o, a, b) p[r]      y = <owner[o], p>
//
//   mode 0: owner A, (a, b) = (j, k), (Pa, Pb) = (B, C), V[o][a][b] at o JK + a K + b
//   mode 1: owner B, (a, b) = (i, k), (Pa, Pb) = (A, C), V[a][o][b] at a JK + o K + b
//   mode 2: owner C, (a, b) = (i, j), (Pa, Pb) = (A, B), V[a][b][o] at (a J + b) K + o
//
// The tile is nmfmu_wmu.hip's (nmfmu_wmu_tile.h): a workgroup of 4 waves owns 128 owner rows x a rank tile of <= 128 x one part
// of the contraction axis, the owner rows stay in registers, a stage is 32 FLAT contraction steps whatever slice boundaries
// fall inside it, Y and the seeds never leave the chip.  What is this kernel's own:
//
//   * two walks of the row-major tensor IN PLACE, no unfolded copy.  INNER (modes 0 and 1): the contraction's inner index b is
//     contiguous, the owner row and the slice a are strided by (JK, K) or (K, JK); a quad of 4 steps is one 16-byte load when
//     it lies inside one slice and its address is 16-byte aligned (decided per quad), else 4 scalar loads, each with its own
//     slice.  OUTER (mode 2): the owner is contiguous and the flat step is the row of a [IJ][K] matrix, wmu's TRANS walk.
//   * the slice table.  Lane l & 31 of every wave divides once per stage: a = (c0 + l) / nB.  Every other index of the stage
//     -- the slices of a quad's four steps, (a, b) of a panel row -- is a wave shuffle of that table and one multiply.
//   * the panel stage.  The 32 rows of Pa and of Pb are fetched one stage ahead into registers (2 x r_pad / 8 per thread) and
//     multiplied on their way into LDS: the Khatri-Rao matrix exists 32 rows at a time, in LDS only.
//   * weights at run time: M == NULL is a uniform branch that skips the loads of M and takes m = 1 inside the tensor.
//   * its own split rule (ntf_auto_split): two workgroups per CU however few row tiles there are -- tensors routinely have one
//     mode of 2 .. 64 -- with parts of at least kWmMinStages stages; wmu's cap of 64 parts is not applied.
//
// Every part stores its two planes to a caller-owned slab [part][num | den][rows][r_pad] with plain stores; ntf_finish_kernel
// adds them in part order and stores the planes (terms) or applies nmf.py:78-92 to the owner in place (step).  No atomics,
// no fences: a repeated call is bitwise identical whatever the workspace held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_ntf_host.h"
#include "nmfmu_sparse_common.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

inline int ntf_auto_split(int rows, int contraction, int r_pad) {
  const int64_t tiles = (int64_t)((rows + kWmRows - 1) / kWmRows) * ((r_pad + 127) / 128);
  const int64_t want = (kNtfTargetWgs + tiles - 1) / tiles;
  const int cap = std::max(1, wmu_stages(contraction) / kWmMinStages);
  return wmu_parts(contraction, (int)std::min<int64_t>(want, cap));
}
inline int ntf_split(int rows, int contraction, int r_pad, int nsplit) {
  return nsplit > 0 ? wmu_parts(contraction, nsplit) : ntf_auto_split(rows, contraction, r_pad);
}

// WmuStage's av / mv / bv (bv: the rows of Pa) and the rows of Pb
template <int RP>
struct NtfStage : WmuStage<RP> {
  float bw[kWmBK * RP / 256];
};

// the slice table of the stage at c0: lane l & 31 holds a = (c0 + l) / nB (0 past the part).  Called by every lane.
__device__ __forceinline__ int ntf_slices(int c0, int cend, int nB, int lane) {
  const int c = c0 + (lane & 31);
  return c < cend ? c / nB : 0;
}

// bv / bw = Pa[a] / Pb[b] of step c0 + idx / RP over the full padded rank; zero in the padded columns and past the part
template <int RP>
__device__ __forceinline__ void ntf_load_panel(NtfStage<RP>& st, const float* __restrict__ Pa, const float* __restrict__ Pb,
                                               int rank, int nB, int c0, int cend, int atab, int tid) {
#pragma unroll
  for (int p = 0; p < kWmBK * RP / 256; ++p) {
    const int idx = p * 256 + tid;
    const int d = idx / RP, r = idx % RP, c = c0 + d;
    const int a = __shfl(atab, d, 64), b = c - a * nB;
    const bool ok = c < cend && r < rank;
    st.bv[p] = ok ? Pa[(size_t)a * rank + r] : 0.f;
    st.bw[p] = ok ? Pb[(size_t)b * rank + r] : 0.f;
  }
}

// sb [c][r] = fl32(Pa[a][r] Pb[b][r]): the Khatri-Rao rows of the stage, formed here and nowhere else
template <int RP>
__device__ __forceinline__ void ntf_store_panel(float* sb, const NtfStage<RP>& st, int tid) {
#pragma unroll
  for (int p = 0; p < kWmBK * RP / 256; ++p) {
    const int idx = p * 256 + tid;
    sb[(idx / RP) * WmuCfg<RP>::LDB + idx % RP] = st.bv[p] * st.bw[p];
  }
}

// av / mv = V / M at (owner row i0 + i, step c0 + c); zero outside the tensor and the part (m = 0: selected away); m = 1
// inside when M is NULL.  OUTER: V[(c0 + c) ld + i0 + i ..], contiguous along the owner, 16-byte loads when `al` and ld % 4 == 0.
// else: V[(i0 + i) sO + a sA + b ..], contiguous along b inside a slice, 16-byte loads per quad where they fit.
template <int RP, bool OUTER>
__device__ __forceinline__ void ntf_load_vm(NtfStage<RP>& st, const float* __restrict__ V, const float* __restrict__ M,
                                            int64_t sO, int64_t sA, int rows, int nB, int i0, int c0, int cend, int atab,
                                            bool al, int tid) {
  const bool has_m = M != nullptr;
  int a[4] = {0, 0, 0, 0};
  if constexpr (!OUTER) {
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = __shfl(atab, (tid & 7) * 4 + q, 64);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid;
    float* av = st.av[p];
    float* mv = st.mv[p];
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = mv[q] = 0.f;
    const int c = c0 + (OUTER ? idx >> 5 : (idx & 7) * 4), i = i0 + (OUTER ? (idx & 31) * 4 : idx >> 3);
    if (c < cend && i < rows) {
      const int left = OUTER ? rows - i : cend - c;      // elements of the quad inside the tensor and the part
      const size_t off = OUTER ? (size_t)c * sA + i : (size_t)i * sO + (size_t)a[0] * sA + (c - a[0] * nB);
      const bool quad = left >= 4 && al && (OUTER ? (sA & 3) == 0 : a[3] == a[0] && (off & 3) == 0);
      if (quad) {
        const float4 v = *reinterpret_cast<const float4*>(V + off);
        av[0] = v.x, av[1] = v.y, av[2] = v.z, av[3] = v.w;
        if (has_m) {
          const float4 m = *reinterpret_cast<const float4*>(M + off);
          mv[0] = m.x, mv[1] = m.y, mv[2] = m.z, mv[3] = m.w;
        } else {
          mv[0] = mv[1] = mv[2] = mv[3] = 1.f;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < left) {
            const size_t at = OUTER ? off + q : (size_t)i * sO + (size_t)a[q] * sA + (c + q - a[q] * nB);
            av[q] = V[at];
            mv[q] = has_m ? M[at] : 1.f;
          }
      }
    }
  }
}

// grid = (row tiles, rank tiles, parts).  on / od + part * pstride: the part's planes [rows][RP].
template <int RP, bool OUTER, int KIND>
__global__ void __launch_bounds__(256) ntf_kernel(const float* __restrict__ V, const float* __restrict__ M, int64_t sO,
                                                  int64_t sA, int rows, int nB, int C, const float* __restrict__ owner,
                                                  const float* __restrict__ Pa, const float* __restrict__ Pb, int rank,
                                                  float beta, int part_len, float* __restrict__ on, float* __restrict__ od,
                                                  int64_t pstride) {
  using K = WmuCfg<RP>;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5;
  const int wave = tid >> 6, wm = wave / K::WN, wn = wave % K::WN;
  const int i0 = blockIdx.x * kWmRows, r0 = blockIdx.y * K::RT;
  const int cbeg = blockIdx.z * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  f32x16 accn[K::TM][K::TN], accd[K::TM][K::TN];
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) accn[t][b][e] = accd[t][b][e] = 0.f;
  const bool al = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(M)) & 15) == 0;
  NtfStage<RP> st;
  int atab = ntf_slices(cbeg, cend, nB, lane);
  ntf_load_vm<RP, OUTER>(st, V, M, sO, sA, rows, nB, i0, cbeg, cend, atab, al, tid);
  ntf_load_panel<RP>(st, Pa, Pb, rank, nB, cbeg, cend, atab, tid);
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    wmu_store_vm<RP, OUTER>(sv, sm, st, tid);
    ntf_store_panel<RP>(sb, st, tid);
    __syncthreads();
    if (c0 + kWmBK < cend) {      // the next stage's loads travel behind this stage's MFMAs
      atab = ntf_slices(c0 + kWmBK, cend, nB, lane);
      ntf_load_vm<RP, OUTER>(st, V, M, sO, sA, rows, nB, i0, c0 + kWmBK, cend, atab, al, tid);
      ntf_load_panel<RP>(st, Pa, Pb, rank, nB, c0 + kWmBK, cend, atab, tid);
    }
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
    // m g_neg over V, m g_pos over M: every element belongs to one lane of the wave that owns its row
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int at = (wave * 32 + wmu_tile_row(e, hl)) * kWmLDA + j;
      const float v = sv[at], m = sm[at];
      float gn, gp;
      masked_g<KIND>(v, y[e], beta, gn, gp);
      const bool w = m > 0.f;
      sv[at] = w ? m * gn : 0.f;
      sm[at] = w ? m * gp : 0.f;
    }
    __syncthreads();
    const float* pn = sv + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pd = sm + (wm * K::TM * 32 + j) * kWmLDA + hl;
    const float* pb = sb + hl * K::LDB + r0 + wn * K::TN * 32 + j;
#pragma unroll
    for (int s2 = 0; s2 < kWmBK; s2 += 2) {
      float bb[K::TN];
#pragma unroll
      for (int b = 0; b < K::TN; ++b) bb[b] = pb[s2 * K::LDB + b * 32];
#pragma unroll
      for (int t = 0; t < K::TM; ++t) {
        const float gn = pn[t * 32 * kWmLDA + s2], gp = pd[t * 32 * kWmLDA + s2];
#pragma unroll
        for (int b = 0; b < K::TN; ++b) {
          accn[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gn, bb[b], accn[t][b], 0, 0, 0);
          accd[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp, bb[b], accd[t][b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  float* pn = on + (size_t)blockIdx.z * pstride;
  float* pd = od + (size_t)blockIdx.z * pstride;
#pragma unroll
  for (int t = 0; t < K::TM; ++t)
#pragma unroll
    for (int b = 0; b < K::TN; ++b) {
      const int r = r0 + wn * K::TN * 32 + b * 32 + j;      // < RP: the rank tiles cover the padded rank exactly
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + wm * K::TM * 32 + t * 32 + wmu_tile_row(e, hl);
        if (i < rows) {
          pn[(size_t)i * RP + r] = r < rank ? accn[t][b][e] : 0.f;
          pd[(size_t)i * RP + r] = r < rank ? accd[t][b][e] : 0.f;
        }
      }
    }
}

// The slab's parts added in part order, then the two planes stored (terms) or nmf.py:78-92 applied in place (step).  There
// may be hundreds of parts over a plane of a few hundred elements: the loads of 8 parts are issued together, the adds stay
// in part order.
__global__ void __launch_bounds__(256) ntf_finish_kernel(const float* __restrict__ ws, int parts, int rows, int rank, int r_pad,
                                                         float* owner, float* __restrict__ num, float* __restrict__ den,
                                                         int step, MaskedApply ap) {
  const int64_t plane = (int64_t)rows * r_pad;
  for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < plane; at += (int64_t)gridDim.x * 256) {
    float n = ws[at], d = ws[plane + at];
    int p = 1;
    for (; p + 8 <= parts; p += 8) {
      float tn[8], td[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) tn[u] = ws[(size_t)(p + u) * 2 * plane + at], td[u] = ws[(size_t)(p + u) * 2 * plane + plane + at];
#pragma unroll
      for (int u = 0; u < 8; ++u) n += tn[u], d += td[u];
    }
    for (; p < parts; ++p) n += ws[(size_t)p * 2 * plane + at], d += ws[(size_t)p * 2 * plane + plane + at];
    if (step) {
      const int r = (int)(at % r_pad);
      float* f = owner + (size_t)(at / r_pad) * rank + r;
      if (r < rank) *f = masked_apply(*f, n, d, ap);
    } else {
      num[at] = n, den[at] = d;
    }
  }
}

// part[tile * nparts + z] = sum over the tile's rows of A and the part's (j, k) of m * (the term of metrics.beta_div that
// holds y), in double: per lane, per wave (fixed-order butterfly), per workgroup.  The mode-0 walk.
template <int RP, int KIND>
__global__ void __launch_bounds__(256) ntf_loss_kernel(const float* __restrict__ V, const float* __restrict__ M, int64_t sO,
                                                       int64_t sA, int rows, int nB, int C, const float* __restrict__ owner,
                                                       const float* __restrict__ Pa, const float* __restrict__ Pb, int rank,
                                                       float beta, int part_len, int nparts, double* __restrict__ part) {
  using K = WmuCfg<RP>;
  __shared__ __attribute__((aligned(16))) float sv[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sm[kWmRows * kWmLDA];
  __shared__ __attribute__((aligned(16))) float sb[kWmBK * K::LDB];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int i0 = (blockIdx.x / nparts) * kWmRows;
  const int cbeg = (blockIdx.x % nparts) * part_len, cend = min(C, cbeg + part_len);
  float a[RP / 2];
  wmu_load_owner<RP>(a, owner, rows, rank, i0 + wave * 32 + j, hl);
  const bool al = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(M)) & 15) == 0;
  double tot = 0.0;
  for (int c0 = cbeg; c0 < cend; c0 += kWmBK) {
    NtfStage<RP> st;
    const int atab = ntf_slices(c0, cend, nB, lane);
    ntf_load_vm<RP, false>(st, V, M, sO, sA, rows, nB, i0, c0, cend, atab, al, tid);
    ntf_load_panel<RP>(st, Pa, Pb, rank, nB, c0, cend, atab, tid);
    wmu_store_vm<RP, false>(sv, sm, st, tid);
    ntf_store_panel<RP>(sb, st, tid);
    __syncthreads();
    const f32x16 y = wmu_form_y<RP>(a, sb, j, hl);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int at = (wave * 32 + wmu_tile_row(e, hl)) * kWmLDA + j;
      const float m = sm[at];
      const double t = masked_loss_term<KIND>(sv[at], y[e], beta);
      tot += m > 0.f ? (double)m * t : 0.0;
    }
    __syncthreads();
  }
  store_lane_totals(tot, red, part);
}

void ntf_finish_launch(int fblocks, const float* ws, int parts, int rows, int rank, int r_pad, float* owner, float* num,
                       float* den, int step, MaskedApply ap, hipStream_t st) {
  hipLaunchKernelGGL(ntf_finish_kernel, dim3(fblocks), dim3(256), 0, st, ws, parts, rows, rank, r_pad, owner, num, den, step, ap);
}

}  // namespace nmfmu

using namespace nmfmu;

namespace {
int ntf_launch(const float* V, const float* M, int I, int J, int K, int mode, float* owner, const float* pa, const float* pb,
               int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den, int step, MaskedApply ap,
               hipStream_t st) {
  const NtfMode md = ntf_mode(I, J, K, mode);
  const int rows = md.rows, contraction = md.nA * md.nB;
  const int parts = ntf_split(rows, contraction, r_pad, nsplit);
  const int part_len = wmu_part_len(contraction, parts);
  const WmuSlab sl = wmu_slab(1, rows, r_pad, parts, step, ws, num, den);
  for_rp(r_pad, [&](auto rp) {
    for_kind(nmfmu_beta_kind(beta), [&](auto k) {
      constexpr int RP = decltype(rp)::value, KIND = decltype(k)::value;
      if (md.outer)
        hipLaunchKernelGGL((ntf_kernel<RP, true, KIND>), sl.grid, dim3(256), 0, st, V, M, md.sO, md.sA, rows, md.nB, contraction,
                           owner, pa, pb, rank, beta, part_len, sl.on, sl.od, sl.pstride);
      else
        hipLaunchKernelGGL((ntf_kernel<RP, false, KIND>), sl.grid, dim3(256), 0, st, V, M, md.sO, md.sA, rows, md.nB, contraction,
                           owner, pa, pb, rank, beta, part_len, sl.on, sl.od, sl.pstride);
    });
  });
  if (!sl.direct) ntf_finish_launch(sl.fblocks, ws, parts, rows, rank, r_pad, owner, num, den, step, ap, st);
  return (int)hipGetLastError();
}

int ntf_loss_split(int I, int64_t JK) { return ntf_auto_split(I, (int)JK, 128); }
}  // namespace

extern "C" {

int nmfmu_ntf_nsplit(int rows, int contraction, int r_pad) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0) return NMFMU_ERR_ARG;
  return ntf_split(rows, contraction, r_pad, 0);
}

int64_t nmfmu_ntf_ws(int rows, int contraction, int r_pad, int nsplit) {
  if (rows <= 0 || contraction <= 0 || r_pad <= 0 || nsplit < 0) return 0;
  return (int64_t)ntf_split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad;
}

int nmfmu_ntf_terms(const float* V, const float* M, int I, int J, int K, int mode, const float* owner, const float* pa,
                    const float* pb, int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den,
                    void* stream) {
  if (!ws || !num || !den || nsplit < 0) return NMFMU_ERR_ARG;
  if (const int rc = ntf_check(V, I, J, K, mode, owner, pa, pb, rank, r_pad, true, nsplit, ntf_split)) return rc;
  return ntf_launch(V, M, I, J, K, mode, const_cast<float*>(owner), pa, pb, rank, r_pad, beta, nsplit, ws, num, den, 0,
                    MaskedApply{0.f, 0.f, 1.f}, S(stream));
}

int nmfmu_ntf_step(const float* V, const float* M, int I, int J, int K, int mode, float* owner, const float* pa, const float* pb,
                   int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit, float* ws, void* stream) {
  if (!ws || owner == pa || owner == pb || nsplit < 0) return NMFMU_ERR_ARG;
  if (const int rc = ntf_check(V, I, J, K, mode, owner, pa, pb, rank, r_pad, true, nsplit, ntf_split)) return rc;
  return ntf_launch(V, M, I, J, K, mode, owner, pa, pb, rank, r_pad, beta, nsplit, ws, nullptr, nullptr, 1,
                    MaskedApply{l1, l2, gamma}, S(stream));
}

int nmfmu_ntf_loss_parts(int I, int J, int K) {
  if (I <= 0 || J <= 0 || K <= 0) return NMFMU_ERR_ARG;
  if ((int64_t)J * K > kNtfMaxContraction) return NMFMU_ERR_UNSUPPORTED;
  return (I + kWmRows - 1) / kWmRows * ntf_loss_split(I, (int64_t)J * K);
}

int nmfmu_ntf_loss(const float* V, const float* M, int I, int J, int K, const float* A, const float* B, const float* C, int rank,
                   float beta, double v_term, double* part, double* out, void* stream) {
  if (!part || !out || !A) return NMFMU_ERR_ARG;
  if (const int rc = ntf_check(V, I, J, K, 0, A, B, C, rank, 0, false, 0, ntf_split)) return rc;
  const int JK = J * K;
  const int nparts = ntf_loss_split(I, JK), part_len = wmu_part_len(JK, nparts);
  const int nblk = (I + kWmRows - 1) / kWmRows * nparts;
  const int kind = nmfmu_beta_kind(beta);
  for_rp(nmfmu_pad_rank(rank), [&](auto rp) {
    for_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((ntf_loss_kernel<decltype(rp)::value, decltype(k)::value>), dim3(nblk), dim3(256), 0, S(stream), V, M,
                         (int64_t)JK, (int64_t)K, I, K, JK, A, B, C, rank, beta, part_len, nparts, part);
    });
  });
  hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, S(stream), part, nblk, v_term, beta_loss_mul(kind, beta),
                     out);
  return (int)hipGetLastError();
}

}  // extern "C"
