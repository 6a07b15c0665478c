// Fold-in by coordinate descent: new rows of a sparse target against a FIXED panel W, every iteration of every row inside one
// launch -- fold_in_cd(solver='ccd' | 'hals') / NMF.transform_cd, DESIGN.md section 28.  beta = 2; the objective of a row
// h with stored entries e (column j_e, value v_e) has one parameter 0 <= omega <= 1, c = 1.0f - omega (fp32, on the host):
//
//   1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 + l1 sum h + l2/2 |h|^2,     y_j = <h, W[j]>
//
// omega = 0: 'missing' (the sweep of nmfmu_sparse_ccd.hip); 0 < omega < 1: implicit feedback (nmfmu_sparse_wccd.hip);
// omega = 1: 'zero', HALS on the row.  With W fixed the rows are independent, so a row is iterated to its end by one wave
// (at most long_rows entries) or by the four waves of its workgroup (more), which never leave the kernel.
//
// Once per row:
//   the W rows of the row's entries -> LDS, row stride rank | 1 (odd: the lanes, one per entry, hit different banks), when the
//   largest share of a wave (the count; per = ceil(count / 4) with four waves) is at most `block`; otherwise every use gathers
//   W[j_e][k] from the row-major W again;
//   d_k = sum_e W[j_e][k]^2,  D_k = fma(c, d_k, omega * G[k][k])  (omega = 0: D_k = d_k, G is not read);
//   omega = 1 (c = 0) also n_k = sum_e v_e W[j_e][k]: the residual t_e = v_e never changes.
// Every iteration:
//   t_e = fma(-c, s_e, v_e),  s_e = sum_k h[k] W[j_e][k]       (k ascending, one fmaf chain from 0) -- formed ANEW from h, so
//                                                               K iterations are bitwise K chained one-iteration calls
//   for k = 0 .. R-1:  n = sum_e t_e W[j_e][k]   (omega = 1: the hoisted n_k)
//                      q = sum_j h[j] G[k][j]    (j < k: this iteration's values, j >= k: the previous ones; omega = 0: none)
//                      num = fma(h[k], D_k, fma(-omega, q, n)) - l1        (omega = 0: fma(h[k], D_k, n) - l1)
//                      h'  = max(eps, num / ((D_k + l2) + eps)),   eps = 2^-23
//                      t_e = fma(-(c * (h' - h[k])), W[j_e][k], t_e) for every e;   h[k] = h'
//   stop after the iteration when max_r |h_k - h_{k-1}| <= tol * max_r h_k (fp32, tol > 0 only).
// That is nmfmu_sp_wccd_sweep's recurrence operation for operation (for omega = 0 nmfmu_sp_ccd_sweep's: fma(-1, s, v) = v - s,
// fma(1, d, 0) = d and -(1 * x) = -x are exact), with d_k and D_k taken out of the loop -- the same chain every time.
//
// The order of the fp32 operations.  With NW waves on the row (1 or 4) wave w owns the entries [w per, (w + 1) per) of the
// row, per = ceil(count / NW); its local entry i sits on lane i mod 64 as slot i / 64.  d, n (and the hoisted n_k): per-lane
// fmaf chains over the slots in ascending order from 0, an xor butterfly 32 .. 1 per wave, and with four waves the waves'
// totals added in wave order ((w0 + w1) + w2) + w3 by every thread (a wave without entries adds +0).  q: lane l runs
// fma(h[l + 64 m], G[k][l + 64 m], q) for m = 0 .. 3 from 0 (coordinates beyond the rank left out), then the same butterfly;
// every wave computes q on its own from its own registers, with identical bits.  After the reductions every thread holds the
// same n, q, D_k and old h[k], computes the same h', and lane k mod 64 of every wave keeps it in its slot k / 64.
//
// One pass over the entries per coordinate: the pass that applies coordinate k's step to t_e also runs, with t_e as it then
// stands, the chain of n for coordinate k + 1 (W[j_e][k] and W[j_e][k + 1] are neighbours: one fetch); the first chain rides
// on the pass that forms the residuals.  The chains are the ones two passes would run.  A lane's reads of a batch of eight
// slots carry no condition (a lane without an entry reads the wave's last one and drops the value by a select), so they are
// in flight together; a share of at most 64 entries (one slot per lane) uses a batch of one.  The Gram row of coordinate
// k + 1 is fetched while coordinate k is worked.
//
// Where the residuals live: in the wave's LDS (every lane reads and writes its own entries only) when the largest share fits
// what the wave has (about 1800 .. 2400 floats, by the rank); a longer row -- beyond 7000 entries -- keeps none and forms
// t_e = fma(-c, <h as it stands, W[j_e]>, v_e) again for every coordinate (the same value with R + 2 roundings instead of
// R + 5 + k; rank times the work, so that any count up to n_cols is served without scratch memory).
//
// A row without entries: omega = 0 leaves it as it came (count 1 with tol > 0: the stop rule holds on the unchanged row,
// max_iter otherwise); omega > 0 sweeps it, the Gram term takes it to the floor.
//
// Which path a row takes (waves, staged or gathered, residuals) is a function of its count, long_rows, block and the rank;
// the three sources of W[j_e][k] and of t_e hold the same floats except for the no-residual rows.  Nothing is shared between
// rows: a row's bits depend on its entries, H0[row], W, gram, omega, l1, l2, max_iter, tol and long_rows alone.  Fixed-order
// reductions, plain vector stores, no atomics, no fences; H is read and written by the row's own wave / workgroup, W, gram
// and the entries are only read.  The four waves of a long row meet at one barrier per coordinate (the totals' buffer
// alternates: a wave writes a buffer again only after the barrier that follows every wave's read of it).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

constexpr float kFcdEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps
constexpr int kFcdWaves = 4;
constexpr int kFcdLdsFloats = 10240;                 // 40 KiB per workgroup: four workgroups, sixteen waves, per CU
constexpr int kFcdRed = 4 * kFcdWaves;               // [2][2][waves]: the long rows' totals
constexpr int kFcdPerWave = ((kFcdLdsFloats - kFcdRed) / kFcdWaves) & ~3;
constexpr int kFcdOwn = 4;                           // coordinates of h a lane holds: rank <= 256
constexpr int kFcdStageU = 4;                        // W rows in flight while staging
constexpr int kFcdBatch = 8;                         // slots of a lane whose reads are in flight together (a share above 64)

enum { kFcdMissing = 0, kFcdWeighted = 1, kFcdHals = 2 };          // omega = 0, 0 < omega < 1, omega = 1
enum { kFcdStaged = 0, kFcdGather = 1, kFcdNoRes = 2 };            // W rows in LDS; gathered; gathered and no residuals kept

struct FcdArgs {
  const int32_t* rowptr;
  const int32_t* colidx;
  const float* vals;
  const int32_t* order;     // NULL: rows in their own order
  float* H;
  const float* W;
  const float* gram;        // [rank][rank]; NULL with omega == 0
  int32_t* n_iter;          // NULL, or [n_rows]
  int n_rows, rank, block, long_rows, max_iter, avail;
  float omega, c, l1, l2, tol;
};

__host__ __device__ inline int fcd_rs(int rank) { return (rank + 63) & ~63; }
// floats a wave has for residuals and staged W rows, after h, D and n
__host__ __device__ inline int fcd_avail(int rank) { return kFcdPerWave - 3 * fcd_rs(rank); }
// the largest share whose residuals AND W rows fit: share * (S + 1) + 3 <= avail
__host__ __device__ inline int fcd_block_cap(int rank) { return (fcd_avail(rank) - 3) / ((rank | 1) + 1); }

template <int MODE, bool WG, int SRC, int kFcdU>
__device__ __forceinline__ void fcd_body(const FcdArgs& a, int row, int p0, int cnt, float* lw, float* red, int lane,
                                         int wave) {
  constexpr int NW = WG ? kFcdWaves : 1;
  constexpr bool kGram = MODE != kFcdMissing, kConstN = MODE == kFcdHals, kRes = SRC != kFcdNoRes && !kConstN;
  const int rank = a.rank, S = rank | 1, rs = fcd_rs(rank);
  const float c = a.c, omega = a.omega;
  float* hs = lw;            // h: the previous iteration's row (kFcdNoRes: as it stands)
  float* Ds = hs + rs;
  float* ns = Ds + rs;
  float* res = ns + rs;
  const int per = (cnt + NW - 1) / NW;           // the largest share: what decides the path, uniform over the workgroup
  const int e0 = WG ? min(cnt, wave * per) : 0;
  const int nloc = min(cnt, e0 + per) - e0;
  const int T = (per + 63) >> 6;
  float* panel = res + ((per + 3) & ~3);
  const int32_t* __restrict__ idx = a.colidx + p0 + e0;
  const float* __restrict__ vals = a.vals + p0 + e0;
  const float* __restrict__ W = a.W;
  int par = 0;

  float fr[kFcdOwn], fo[kFcdOwn];
#pragma unroll
  for (int m = 0; m < kFcdOwn; ++m) {
    const int j = lane + 64 * m;
    fr[m] = j < rank ? a.H[(size_t)row * rank + j] : 0.f;
  }

  if constexpr (SRC == kFcdStaged) {
    for (int i0 = 0; i0 < nloc; i0 += kFcdStageU) {
      float b[kFcdStageU][kFcdOwn];
#pragma unroll
      for (int u = 0; u < kFcdStageU; ++u) {
        const bool ok = i0 + u < nloc;
        const int col = ok ? idx[i0 + u] : 0;
#pragma unroll
        for (int m = 0; m < kFcdOwn; ++m) {
          const int k = lane + 64 * m;
          b[u][m] = (ok && k < rank) ? W[(size_t)col * rank + k] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kFcdStageU; ++u)
#pragma unroll
        for (int m = 0; m < kFcdOwn; ++m) {
          const int k = lane + 64 * m;
          if (i0 + u < nloc && k < rank) panel[(i0 + u) * S + k] = b[u][m];
        }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // W[j_i][k] of local entry i
  auto P = [&](int i, int k) -> float {
    if constexpr (SRC == kFcdStaged) return panel[i * S + k];
    else return W[(size_t)idx[i] * rank + k];
  };
  // the residual of local entry i from h as it stands in hs
  auto fresh = [&](int i) -> float {
    float s = 0.f;
    for (int k = 0; k < rank; ++k) s = fmaf(hs[k], P(i, k), s);
    return fmaf(-c, s, vals[i]);
  };
  // the wave's totals -> the row's, in wave order
  auto total = [&](float& x, float& y) {
    if constexpr (WG) {
      float* rd = red + par * 2 * NW;
      par ^= 1;
      if (lane == 0) rd[wave] = x, rd[NW + wave] = y;
      __syncthreads();
      x = rd[0], y = rd[NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) x += rd[w], y += rd[NW + w];
    }
  };

  // Slots t0 .. t0 + kFcdU - 1 of this lane: whether it has the entry, and the local entry to read -- a lane without one
  // reads the wave's last entry and drops the value, so that the loads of a batch carry no condition and are all in flight
  // together (nloc > 0 where this is called).
  auto slots = [&](int t0, bool (&ok)[kFcdU], int (&ii)[kFcdU]) {
#pragma unroll
    for (int u = 0; u < kFcdU; ++u) {
      const int i = lane + 64 * (t0 + u);
      ok[u] = i < nloc;
      ii[u] = ok[u] ? i : nloc - 1;
    }
  };

  // once per row: D_k, and n_k where the residual is constant
  for (int k = 0; k < rank; ++k) {
    float d = 0.f, n = 0.f;
    if (nloc > 0) {
      for (int t0 = 0; t0 < T; t0 += kFcdU) {
        bool ok[kFcdU];
        int ii[kFcdU];
        float p[kFcdU], v[kFcdU];
        slots(t0, ok, ii);
#pragma unroll
        for (int u = 0; u < kFcdU; ++u) {
          p[u] = P(ii[u], k);
          v[u] = kConstN ? vals[ii[u]] : 0.f;   // t_e = fma(-0, s_e, v_e) = v_e
        }
#pragma unroll
        for (int u = 0; u < kFcdU; ++u) {
          d = ok[u] ? fmaf(p[u], p[u], d) : d;
          if constexpr (kConstN) n = ok[u] ? fmaf(v[u], p[u], n) : n;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      d += __shfl_xor(d, o, 64);
      if constexpr (kConstN) n += __shfl_xor(n, o, 64);
    }
    total(d, n);
    if (lane == 0) {
      Ds[k] = kGram ? fmaf(c, d, omega * a.gram[(size_t)k * rank + k]) : d;
      if constexpr (kConstN) ns[k] = n;
    }
  }

  int it = 0;
  while (it < a.max_iter) {
    __builtin_amdgcn_wave_barrier();      // Ds / ns above, and the last iteration's reads of hs
#pragma unroll
    for (int m = 0; m < kFcdOwn; ++m) {
      const int j = lane + 64 * m;
      fo[m] = fr[m];
      if (j < rs) hs[j] = fr[m];
    }
    __builtin_amdgcn_wave_barrier();
    float nk = 0.f;                         // this lane's chain of n for the coordinate at hand
    if constexpr (kRes) {                   // the residuals anew from h, and coordinate 0's chain in the same pass
      if (nloc > 0) {
        for (int t0 = 0; t0 < T; t0 += kFcdU) {
          bool ok[kFcdU];
          int ii[kFcdU];
          float r[kFcdU], p0[kFcdU];
          slots(t0, ok, ii);
#pragma unroll
          for (int u = 0; u < kFcdU; ++u) r[u] = 0.f, p0[u] = P(ii[u], 0);
          for (int k = 0; k < rank; ++k) {
            const float hk = hs[k];
#pragma unroll
            for (int u = 0; u < kFcdU; ++u) r[u] = fmaf(hk, P(ii[u], k), r[u]);
          }
#pragma unroll
          for (int u = 0; u < kFcdU; ++u) {
            r[u] = fmaf(-c, r[u], vals[ii[u]]);
            if (ok[u]) res[ii[u]] = r[u];
            nk = ok[u] ? fmaf(r[u], p0[u], nk) : nk;
          }
        }
      }
    }
    float gk[kFcdOwn], gn[kFcdOwn];         // row k of the Gram matrix, and row k + 1 on its way: off the coordinate's chain
    if constexpr (kGram) {
#pragma unroll
      for (int m = 0; m < kFcdOwn; ++m) {
        const int j = lane + 64 * m;
        gk[m] = j < rank ? a.gram[j] : 0.f;
      }
    }
    for (int k = 0; k < rank; ++k) {
      const float f = hs[k];
      float n = nk, q = 0.f;
      if constexpr (kGram) {
        const float* __restrict__ gnext = a.gram + (size_t)(k + 1 < rank ? k + 1 : k) * rank;
#pragma unroll
        for (int m = 0; m < kFcdOwn; ++m) {
          const int j = lane + 64 * m;
          gn[m] = j < rank ? gnext[j] : 0.f;
        }
#pragma unroll
        for (int m = 0; m < kFcdOwn; ++m)
          if (lane + 64 * m < rank) q = fmaf(fr[m], gk[m], q);
#pragma unroll
        for (int m = 0; m < kFcdOwn; ++m) gk[m] = gn[m];
      }
      if constexpr (!kConstN && !kRes) {    // no residuals kept: each formed from h as it stands
        n = 0.f;
        for (int t = 0; t < T; ++t) {
          const int i = lane + 64 * t;
          if (i < nloc) n = fmaf(fresh(i), P(i, k), n);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        if constexpr (!kConstN) n += __shfl_xor(n, o, 64);
        if constexpr (kGram) q += __shfl_xor(q, o, 64);
      }
      if constexpr (kConstN) {
        n = ns[k];
      } else {
        float unused = 0.f;
        total(n, unused);
      }
      const float D = Ds[k];
      const float num = (kGram ? fmaf(f, D, fmaf(-omega, q, n)) : fmaf(f, D, n)) - a.l1;
      const float den = (D + a.l2) + kFcdEps;
      const float fn = fmaxf(kFcdEps, num / den);   // (a NaN quotient gives eps)
      if constexpr (kRes) {
        // one pass over the entries: t_e takes coordinate k's step and, as it then stands, joins coordinate k + 1's chain
        // (W[j_e][k] and W[j_e][k + 1] are neighbours: one fetch).  The chains are the ones two passes would run.
        const float back = -(c * (fn - f));
        const int kn = k + 1 < rank ? k + 1 : k;
        nk = 0.f;
        if (nloc > 0) {
          for (int t0 = 0; t0 < T; t0 += kFcdU) {
            bool ok[kFcdU];
            int ii[kFcdU];
            float r[kFcdU], pk[kFcdU], pn[kFcdU];
            slots(t0, ok, ii);
#pragma unroll
            for (int u = 0; u < kFcdU; ++u) {
              if constexpr (SRC == kFcdStaged) {
                pk[u] = panel[ii[u] * S + k], pn[u] = panel[ii[u] * S + kn];
              } else {
                const float* __restrict__ wr = W + (size_t)idx[ii[u]] * rank;
                pk[u] = wr[k], pn[u] = wr[kn];
              }
              r[u] = res[ii[u]];
            }
#pragma unroll
            for (int u = 0; u < kFcdU; ++u) {
              r[u] = fmaf(back, pk[u], r[u]);
              if (ok[u]) res[ii[u]] = r[u];
              nk = ok[u] ? fmaf(r[u], pn[u], nk) : nk;
            }
          }
        }
      }
      if constexpr (SRC == kFcdNoRes && !kConstN) {   // the next coordinate's residuals read h as it stands
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) hs[k] = fn;
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int m = 0; m < kFcdOwn; ++m)   // every thread holds the same h': the lane that owns coordinate k keeps it
        if (lane + 64 * m == k) fr[m] = fn;
    }
    ++it;
    float dmax = 0.f, hmax = 0.f;
#pragma unroll
    for (int m = 0; m < kFcdOwn; ++m)
      if (lane + 64 * m < rank) {
        dmax = fmaxf(dmax, fabsf(__fsub_rn(fr[m], fo[m])));
        hmax = fmaxf(hmax, fr[m]);
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
      hmax = fmaxf(hmax, __shfl_xor(hmax, o, 64));
    }
    if (a.tol > 0.f && dmax <= a.tol * hmax) break;   // (the same bits in every wave of the row)
  }
  if (!WG || wave == 0) {
#pragma unroll
    for (int m = 0; m < kFcdOwn; ++m) {
      const int j = lane + 64 * m;
      if (j < rank) a.H[(size_t)row * rank + j] = fr[m];
    }
    if (a.n_iter && lane == 0) a.n_iter[row] = it;
  }
}

template <int MODE, bool WG>
__device__ __forceinline__ void fcd_row(const FcdArgs& a, int row, float* lw, float* red, int lane, int wave) {
  const int p0 = __builtin_amdgcn_readfirstlane(a.rowptr[row]);
  const int cnt = __builtin_amdgcn_readfirstlane(a.rowptr[row + 1]) - p0;
  if constexpr (MODE == kFcdMissing && !WG) {
    if (cnt <= 0) {       // nothing measured: the row stays; the stop rule holds on it at once
      if (a.n_iter && lane == 0) a.n_iter[row] = a.tol > 0.f ? 1 : a.max_iter;
      return;
    }
  }
  if constexpr (WG) __syncthreads();   // the row before this one is done with the totals' buffer
  __builtin_amdgcn_wave_barrier();
  const int per = WG ? (cnt + kFcdWaves - 1) / kFcdWaves : cnt;
  // (the batch: one slot per lane needs none; the operations and their order are the same either way)
  if (per <= 64) {
    if (per <= a.block) fcd_body<MODE, WG, kFcdStaged, 1>(a, row, p0, cnt, lw, red, lane, wave);
    else fcd_body<MODE, WG, kFcdGather, 1>(a, row, p0, cnt, lw, red, lane, wave);   // (64 <= avail at every rank)
  } else if (per <= a.block) {
    fcd_body<MODE, WG, kFcdStaged, kFcdBatch>(a, row, p0, cnt, lw, red, lane, wave);
  } else if (per <= a.avail) {
    fcd_body<MODE, WG, kFcdGather, kFcdBatch>(a, row, p0, cnt, lw, red, lane, wave);
  } else {
    fcd_body<MODE, WG, kFcdNoRes, kFcdBatch>(a, row, p0, cnt, lw, red, lane, wave);
  }
}

// A workgroup takes four rows of the order: first its long rows, one after the other with all four waves, then its short
// rows, one per wave.  (Every decision before a barrier is a function of the counts: uniform over the workgroup.)
template <int MODE>
__global__ void __launch_bounds__(64 * kFcdWaves, 4) fold_in_cd_kernel(FcdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kFcdWaves * kFcdPerWave + kFcdRed];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* lw = lds + wave * kFcdPerWave;
  float* red = lds + kFcdWaves * kFcdPerWave;
  int mine = -1;
  for (int i = 0; i < kFcdWaves; ++i) {
    const int at = blockIdx.x * kFcdWaves + i;
    if (at >= a.n_rows) break;
    const int row = a.order ? a.order[at] : at;
    const int cnt = a.rowptr[row + 1] - a.rowptr[row];
    if (cnt > a.long_rows) fcd_row<MODE, true>(a, row, lw, red, lane, wave);
    else if (i == wave) mine = row;
  }
  if (mine >= 0) fcd_row<MODE, false>(a, mine, lw, red, lane, wave);
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int nmfmu_fold_in_cd_block(int rank) {
  if (rank <= 0 || rank > 256) return 0;
  return fcd_block_cap(rank);
}

int nmfmu_fold_in_cd_long_rows(int rank) {
  if (rank <= 0 || rank > 256) return 0;
  const int cap = fcd_block_cap(rank);
  return cap < 128 ? cap : 128;
}

int nmfmu_fold_in_cd(const int32_t* rowptr, const int32_t* colidx, const float* vals, int n_rows, float* H, const float* W,
                     int n_cols, int rank, const float* gram, float omega, float l1, float l2, int max_iter, float tol,
                     int32_t* n_iter_rows, const int32_t* order, int block, int long_rows, void* stream) {
  if (!rowptr || !colidx || !vals || !H || !W || H == W) return NMFMU_ERR_ARG;
  if (rank <= 0 || n_rows < 0 || n_cols <= 0 || max_iter < 0 || !(tol >= 0.f) || block < 0 || long_rows < 0)
    return NMFMU_ERR_ARG;
  if (!(omega >= 0.f && omega <= 1.f)) return NMFMU_ERR_ARG;   // (a NaN fails both comparisons)
  if (omega > 0.f && !gram) return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  if (n_rows == 0 || max_iter == 0) return NMFMU_OK;

  const int cap = fcd_block_cap(rank);
  FcdArgs a;
  a.rowptr = rowptr, a.colidx = colidx, a.vals = vals, a.order = order, a.H = H, a.W = W, a.gram = gram;
  a.n_iter = n_iter_rows;
  a.n_rows = n_rows, a.rank = rank, a.max_iter = max_iter;
  a.block = block == 0 ? cap : (block < cap ? block : cap);
  a.long_rows = long_rows == 0 ? nmfmu_fold_in_cd_long_rows(rank) : long_rows;   // a function of the rank alone
  a.avail = fcd_avail(rank);
  a.omega = omega, a.c = 1.0f - omega, a.l1 = l1, a.l2 = l2, a.tol = tol;
  const dim3 grid((n_rows + kFcdWaves - 1) / kFcdWaves), blk(64 * kFcdWaves);
  if (omega == 0.f) hipLaunchKernelGGL(fold_in_cd_kernel<kFcdMissing>, grid, blk, 0, S(stream), a);
  else if (omega == 1.f) hipLaunchKernelGGL(fold_in_cd_kernel<kFcdHals>, grid, blk, 0, S(stream), a);
  else hipLaunchKernelGGL(fold_in_cd_kernel<kFcdWeighted>, grid, blk, 0, S(stream), a);
  return (int)hipGetLastError();
}

}  // extern "C"
