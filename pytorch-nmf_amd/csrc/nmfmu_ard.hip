// ARD-NMF (Tan & Fevotte, TPAMI 2013): the MU apply stage with a PER-COMPONENT penalty that changes every iteration, and the
// relevance update that produces it.  The expensive half of an iteration is nmfmu_mu_partial, unchanged; these two kernels are
// HBM / latency bound like their siblings in nmfmu_aux.hip.  Deterministic: fixed-order reductions, no atomics but the fp16
// clamp bit of the status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_aux.h"
#include "nmfmu_pp.h"

namespace nmfmu {

// ------------------------------------------------------------------------------------------------------------
// ard_apply: apply_kernel (nmfmu_aux.hip) without its trainer / pack-only modes and with pen[r] in place of the scalars l1 / l2:
//   neg = relu(sum num slabs) + eps;  pos = kl_den[r] (beta == 1) or relu(sum den slabs) + eps
//   L2 ? pos += pen[r] * f : pos += pen[r];   f *= (neg / pos)^gamma
// A pen entry of 0 leaves the bits of the unpenalised update (x + 0.f and fma(0.f, f, x) are x).  Slab summation order, stripe
// and thread choice, image emission and column sums are COPIES of apply_kernel's -- keep the two in step (tests/test_gpu_ard.py
// compares them bit for bit).  New: the prior's norm of every component over the stripe, f(x) = sum x ('l1': the column sum
// itself, not formed twice) or 1/2 sum x^2 ('l2': from the LDS tile, to norm_part).
// ------------------------------------------------------------------------------------------------------------
template <int ROWS, int R_PAD>
constexpr int ard_threads() { return ROWS * (R_PAD / 4) >= 512 ? 512 : 256; }   // = apply_threads

template <int R_PAD, bool X3, bool L2, int ROWS, int NT>
__global__ void __launch_bounds__(NT) ard_apply_kernel(ApplyArgs a, const float* __restrict__ pen, float* __restrict__ norm_part) {
  constexpr int LDT = R_PAD + 1;  // odd leading dimension: the P2 column reads below stay <= 2-way bank conflicted
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tile = reinterpret_cast<float*>(smem_raw);  // [ROWS][LDT]
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const size_t plane = (size_t)a.rows_pad * R_PAD;
  constexpr int R4 = R_PAD / 4;

  for (int idx = tid; idx < ROWS * R4; idx += NT) {
    const int rl = idx / R4, r = (idx - rl * R4) * 4;
    const int row = row0 + rl;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < a.rows && r < a.rank) {
      float* fp = a.f + (size_t)row * a.rank + r;
      const int nv = min(4, a.rank - r);
      for (int i = 0; i < nv; ++i) f[i] = fp[i];
      const size_t e = (size_t)row * R_PAD + r;
      // (apply_kernel's slab sum: rounds of 16, then 8, then 1, combined in slab order)
      float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
      int s0 = 0;
      typedef float f32x4_t __attribute__((ext_vector_type(4)));
      for (; s0 + 16 <= a.nslab; s0 += 16) {
        f32x4_t v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(a.num + (size_t)(s0 + u) * plane + e));
#pragma unroll
        for (int u = 0; u < 16; ++u) n4.x += v[u].x, n4.y += v[u].y, n4.z += v[u].z, n4.w += v[u].w;
      }
      for (; s0 + 8 <= a.nslab; s0 += 8) {
        f32x4_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(a.num + (size_t)(s0 + u) * plane + e));
#pragma unroll
        for (int u = 0; u < 8; ++u) n4.x += v[u].x, n4.y += v[u].y, n4.z += v[u].z, n4.w += v[u].w;
      }
      for (; s0 < a.nslab; ++s0) {
        const float4 v = *reinterpret_cast<const float4*>(a.num + (size_t)s0 * plane + e);
        n4.x += v.x, n4.y += v.y, n4.z += v.z, n4.w += v.w;
      }
      const float neg[4] = {n4.x, n4.y, n4.z, n4.w};
      float pos[4];
      if (a.kl_den) {  // closed form, no relu / eps
        const float4 d4 = *reinterpret_cast<const float4*>(a.kl_den + r);
        pos[0] = d4.x, pos[1] = d4.y, pos[2] = d4.z, pos[3] = d4.w;
      } else {
        float4 d4 = *reinterpret_cast<const float4*>(a.den + e);
        for (int s = 1; s < a.nslab; ++s) {
          const float4 v = *reinterpret_cast<const float4*>(a.den + s * plane + e);
          d4.x += v.x, d4.y += v.y, d4.z += v.z, d4.w += v.w;
        }
        pos[0] = fmaxf(d4.x, 0.f) + kEps, pos[1] = fmaxf(d4.y, 0.f) + kEps;
        pos[2] = fmaxf(d4.z, 0.f) + kEps, pos[3] = fmaxf(d4.w, 0.f) + kEps;
      }
      const float4 p4 = *reinterpret_cast<const float4*>(pen + r);   // phi / lambda_r of this thread's four components
      const float pn[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nv) {
          const float ng = fmaxf(neg[i], 0.f) + kEps;
          float ps = pos[i];
          if constexpr (L2) ps += pn[i] * f[i];   // (contracted to one fma, like apply_kernel's  ps += a.l2 * f[i])
          else ps += pn[i];
          float mult = ng / ps;
          if (a.gamma != 1.f) mult = powf(mult, a.gamma);
          f[i] *= mult;
          fp[i] = f[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[rl * LDT + r + i] = f[i];
  }
  __syncthreads();

  // P1: ROWS rows x (R_PAD/8) sixteen-byte slots, swizzled inside each row
  constexpr int SP = R_PAD / 8;
  bool clamped = false;   // fp16 images: a factor value above 65504 is stored as 65504 -- tell the caller (status word)
  for (int idx = tid; idx < ROWS * SP; idx += NT) {
    const int rl = idx / SP, slot = idx - rl * SP;
    const float* src = tile + rl * LDT + slot * 8;
    u32x4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x0 = src[2 * i], x1 = src[2 * i + 1];
      clamped |= fmaxf(x0, x1) > 65504.f;
      const uint32_t h = pack_img(x0, x1, a.f16);
      hi[i] = h;
      lo[i] = pack_bf16(x0 - bf16_lo(h), x1 - bf16_hi(h));
    }
    const int64_t off = p1_offset(row0 + rl, slot * 8, R_PAD);
    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.p1_hi) + off) = hi;
    if constexpr (X3) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.p1_lo) + off) = lo;
  }
  if (a.f16 && a.status && __any(clamped) && (tid & 63) == 0) atomicOr(a.status, 1u);
  // P2: [R_PAD][64] tiles; this block owns ROWS/8 of the 8 slots (8 consecutive factor rows each) of every rank row
  constexpr int NS = ROWS / 8;
  for (int idx = tid; idx < (a.p2_hi ? R_PAD * NS : 0); idx += NT) {   // (p2_hi == nullptr: nobody reads the transposed images)
    const int r = idx / NS, sl = idx - r * NS;
    u32x4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x0 = tile[(sl * 8 + 2 * i) * LDT + r], x1 = tile[(sl * 8 + 2 * i + 1) * LDT + r];
      const uint32_t h = pack_img(x0, x1, a.f16);
      hi[i] = h;
      lo[i] = pack_bf16(x0 - bf16_lo(h), x1 - bf16_hi(h));
    }
    const int64_t off = p2_offset(row0 + sl * 8, r, R_PAD);
    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.p2_hi) + off) = hi;
    if constexpr (X3) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.p2_lo) + off) = lo;
  }
  // partial column sums of this stripe (fixed order -> deterministic); 'l1': they ARE the prior's partial norms (f >= 0).
  // 'l2': 1/2 sum f^2 in the same order.  Padded rows and ranks are zero in the tile.
  for (int r = tid; r < R_PAD; r += NT) {
    float s = 0.f, q = 0.f;
#pragma unroll 8
    for (int rl = 0; rl < ROWS; ++rl) {
      const float t = tile[rl * LDT + r];
      s += t;
      if constexpr (L2) q += t * t;
    }
    a.colsum_part[(size_t)blockIdx.x * R_PAD + r] = s;
    if constexpr (L2) norm_part[(size_t)blockIdx.x * R_PAD + r] = 0.5f * q;
  }
}

// Second stage, shaped like colsum_finalize_kernel (same loads, same order of additions: colsum is bit-identical to what
// nmfmu_mu_apply leaves).  blockIdx.y == 0: colsum[r] = sum_b colsum_part[b][r], and with norm_part == nullptr ('l1') the same
// value to norm[r]; blockIdx.y == 1 ('l2'): norm[r] = sum_b norm_part[b][r].
__global__ void __launch_bounds__(256) ard_finalize_kernel(const float* __restrict__ colsum_part, const float* __restrict__ norm_part,
                                                           int nblk, int r_pad, float* __restrict__ colsum, float* __restrict__ norm) {
  __shared__ float4 red[32][8];
  const float* part = blockIdx.y == 0 ? colsum_part : norm_part;
  const int c4 = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int col = blockIdx.x * 32 + c4 * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int b = g;
  for (; b + 7 * 32 < nblk; b += 8 * 32) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(part + (size_t)(b + 32 * u) * r_pad + col);
#pragma unroll
    for (int u = 0; u < 8; ++u) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
  }
  for (; b < nblk; b += 32) {
    const float4 v = *reinterpret_cast<const float4*>(part + (size_t)b * r_pad + col);
    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
  }
  red[g][c4] = s;
  __syncthreads();
  if (g == 0) {
    float4 t = red[0][c4];
#pragma unroll
    for (int i = 1; i < 32; ++i) {
      const float4 v = red[i][c4];
      t.x += v.x, t.y += v.y, t.z += v.z, t.w += v.w;
    }
    if (blockIdx.y == 0) {
      *reinterpret_cast<float4*>(colsum + col) = t;
      if (!norm_part) *reinterpret_cast<float4*>(norm + col) = t;
    } else {
      *reinterpret_cast<float4*>(norm + col) = t;
    }
  }
}

template <int R_PAD, int ROWS>
static int launch_ard_apply_rr(const ApplyArgs& a, bool x3, const float* pen, bool l2, float* norm_part, float* norm, hipStream_t s) {
  const int grid = a.rows_pad / ROWS;
  const size_t lds = (size_t)ROWS * (R_PAD + 1) * sizeof(float);
  constexpr int NT = ard_threads<ROWS, R_PAD>();
#define L(X, P)                                                                                                      \
  {                                                                                                                  \
    auto k = ard_apply_kernel<R_PAD, X, P, ROWS, NT>;                                                                  \
    if (lds > 64 * 1024) {                                                                                           \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                         (int)lds);                                                                  \
      if (e != hipSuccess) return (int)e;                                                                            \
    }                                                                                                                \
    hipLaunchKernelGGL(k, dim3(grid), dim3(NT), lds, s, a, pen, norm_part);                                           \
  }
  if (x3 && l2) L(true, true)
  else if (x3) L(true, false)
  else if (l2) L(false, true)
  else L(false, false)
#undef L
  const int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(ard_finalize_kernel, dim3(R_PAD / 32, l2 ? 2 : 1), dim3(256), 0, s, a.colsum_part, l2 ? norm_part : nullptr,
                     grid, R_PAD, a.colsum, norm);
  return (int)hipGetLastError();
}

template <int R_PAD>
static int launch_ard_apply_r(const ApplyArgs& a, bool x3, const float* pen, bool l2, float* norm_part, float* norm, hipStream_t s) {
  if (apply_stripe_rows(a.rows_pad) == 16) return launch_ard_apply_rr<R_PAD, 16>(a, x3, pen, l2, norm_part, norm, s);
  return launch_ard_apply_rr<R_PAD, 64>(a, x3, pen, l2, norm_part, norm, s);
}

int launch_ard_apply(int r_pad, const ApplyArgs& a, bool x3, const float* pen, bool l2_prior, float* norm_part, float* norm,
                     hipStream_t s) {
  switch (r_pad) {
    case 32: return launch_ard_apply_r<32>(a, x3, pen, l2_prior, norm_part, norm, s);
    case 64: return launch_ard_apply_r<64>(a, x3, pen, l2_prior, norm_part, norm, s);
    case 128: return launch_ard_apply_r<128>(a, x3, pen, l2_prior, norm_part, norm, s);
    case 256: return launch_ard_apply_r<256>(a, x3, pen, l2_prior, norm_part, norm, s);
  }
  return -2;
}

// ------------------------------------------------------------------------------------------------------------
// ard_relevance: lambda_k = ((norm_w[k] + norm_h[k]) + b) / c, pen[k] = phi / lambda_k (0 in the padding), and
// delta[0] = max_k |lambda_k - old| / old against the lam it overwrites.  One workgroup, one component per thread (r_pad <= 256).
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ard_relevance_kernel(const float* __restrict__ norm_w, const float* __restrict__ norm_h, int rank,
                                                            int r_pad, float b, float c, float phi, float* __restrict__ lam,
                                                            float* __restrict__ pen, float* __restrict__ delta) {
  __shared__ float red[256];
  const int k = threadIdx.x;
  float d = 0.f;
  if (k < r_pad) {
    float l = 0.f, p = 0.f;
    if (k < rank) {
      const float old = lam[k];
      l = ((norm_w[k] + norm_h[k]) + b) / c;
      p = phi / l;
      d = fabsf(l - old) / old;
      if (!(d == d)) d = __builtin_inff();   // (a NaN never passes for "converged")
    }
    lam[k] = l;
    pen[k] = p;
  }
  red[k] = d;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (k < o) red[k] = fmaxf(red[k], red[k + o]);
    __syncthreads();
  }
  if (k == 0) delta[0] = red[0];
}

int launch_ard_relevance(const float* norm_w, const float* norm_h, int rank, int r_pad, float b, float c, float phi, float* lam,
                         float* pen, float* delta, hipStream_t s) {
  hipLaunchKernelGGL(ard_relevance_kernel, dim3(1), dim3(256), 0, s, norm_w, norm_h, rank, r_pad, b, c, phi, lam, pen, delta);
  return (int)hipGetLastError();
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_ard_apply(const nmfmu_step* st, const float* kl_den, const float* pen, int prior, float* norm_part, float* norm,
                    void* stream) {
  if (!st || !st->owner.f || !pen || !norm || (prior != NMFMU_ARD_L1 && prior != NMFMU_ARD_L2)) return NMFMU_ERR_ARG;
  if (prior == NMFMU_ARD_L2 && !norm_part) return NMFMU_ERR_ARG;
  if (st->r_pad != pad_rank(st->rank) || st->owner.rows_pad != pad_rows(st->owner.rows)) return NMFMU_ERR_ARG;
  const bool kl = nmfmu_beta_kind(st->beta) == NMFMU_BETA_KL;
  ApplyArgs a{};   // (as apply_common fills it for nmfmu_mu_apply(st, NULL, NULL, 0, kl_den); l1 / l2 are not read)
  a.f = st->owner.f;
  a.num = st->slab_num, a.den = st->slab_den, a.nslab = st->nsplit;
  a.kl_den = kl ? kl_den : nullptr;
  if (!a.num || a.nslab < 1) return NMFMU_ERR_ARG;
  if (kl ? !a.kl_den : !a.den) return NMFMU_ERR_ARG;
  a.p1_hi = st->owner.p1_hi, a.p1_lo = st->owner.p1_lo, a.p2_hi = st->owner.p2_hi, a.p2_lo = st->owner.p2_lo;
  a.colsum_part = st->owner.colsum_part, a.colsum = st->owner.colsum;
  a.rows = st->owner.rows, a.rank = st->rank, a.rows_pad = st->owner.rows_pad;
  a.gamma = st->gamma;
  a.f16 = st->precision == NMFMU_PREC_F16 || st->precision == NMFMU_PREC_F16X || st->precision == NMFMU_PREC_F16R;
  a.status = st->status;
  if (!a.p1_hi || !a.p2_hi || !a.colsum || !a.colsum_part) return NMFMU_ERR_ARG;
  const bool x3 = st->precision == NMFMU_PREC_BF16X3;
  bool writes_p2 = true;
  if (const int e = apply_writes_p2(st, &writes_p2)) return e;
  if (!writes_p2) a.p2_hi = a.p2_lo = nullptr;   // nobody reads the transposed images where the stage promises so
  if (x3 && (!a.p1_lo || (a.p2_hi && !a.p2_lo))) return NMFMU_ERR_ARG;
  return launch_ard_apply(st->r_pad, a, x3, pen, prior == NMFMU_ARD_L2, norm_part, norm, reinterpret_cast<hipStream_t>(stream));
}

int nmfmu_ard_relevance(const float* norm_w, const float* norm_h, int rank, int r_pad, float b, float c, float phi, float* lam,
                        float* pen, float* delta, void* stream) {
  if (!norm_w || !norm_h || !lam || !pen || !delta || rank < 1 || r_pad != pad_rank(rank)) return NMFMU_ERR_ARG;
  if (!(b > 0.f) || !(c > 0.f) || !(phi > 0.f)) return NMFMU_ERR_ARG;
  return launch_ard_relevance(norm_w, norm_h, rank, r_pad, b, c, phi, lam, pen, delta, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
