// CCD on the CP model through the NORMAL EQUATIONS of an owner row -- the route of ntf.ntf_ccd_sweep(gram_rows=) for rows
// with many stored entries, DESIGN.md section 41.  With missing data the quadratic of owner row i is 1/2 f^T Q_i f - b_i^T f,
//
//   Q_i = sum_e q_e q_e^T,   b_i = sum_e v_e q_e,   q_e,k = __fmul_rn(Pa[a_e][k], Pb[b_e][k])      (the sweep's q: one rounded product)
//
// summed over the row's stored entries.  Forming Q_i has no dependence between entries, so a long row is cut into PARTS (runs
// of `part` entries, a multiple of 32; the last part of a row is shorter) that run on the whole device, where the maintained-
// residual sweep (nmfmu_sparse_ntf_ccd.hip) keeps a row on one workgroup.  Two kernels:
//
// 1. sp_ntf_ccd_gram_parts_kernel<NB, G>: a workgroup of four waves takes one part.  NB = r_pad / 32, r_pad = 32 / 64 / 128 / 256.
//    Per tile of 32 entries:
//      gather  G = 4 (rank % 4 == 0, both panels 16-byte aligned): 16-byte loads of Pa[a_e][4g ..] and Pb[b_e][4g ..]; G = 1:
//              4-byte loads.  r_pad / (8 G) loads per panel and thread, issued ONE TILE AHEAD into registers and multiplied and
//              stored to LDS after the current tile's matrix work; the index pairs come from LDS, loaded TWO tiles ahead.
//      LDS     sq [2][32][LD]: entry-major, LD = r_pad + 32 floats (r_pad == 32: 32), zeros in the padded rank columns and in
//              the entries past the part's end; double-buffered, one barrier per tile.  Lane l reads q[e0 + l / 32][32 b + l % 32]
//              for either operand of v_mfma_f32_32x32x2_f32 on block b: 32 consecutive floats per half wave, the two halves
//              32 banks apart -- conflict-free ds_read_b32.
//      MFMA    only the blocks (bi, bj) with bi <= bj.  A wave owns the block rows p and NB - 1 - p: NB + 1 blocks (one block
//              at NB == 1), the A operand read once per block row and k-step.  NB == 8: p = wave; NB == 4: p = wave % 2 and
//              the two waves of a pair split the tile's entries in halves; NB <= 2: every wave owns all blocks and a quarter
//              of the tile's entries.  Waves that split a tile add their accumulators in wave order at the part's end,
//              through the tile buffers.  No wave is without matrix work at any r_pad.
//      b       thread c < r_pad: b_c = fmaf(v_e, q[e][c], b_c) over the tile's entries in entry order (v_e a broadcast).
//    The part's upper blocks (bi <= bj, each a full 32 x 32) and b go to its slot of the workspace with plain vector stores: no
//    atomics, no fences; a part's bits depend on its entries, the panels and the part length alone.
//
// 2. sp_ntf_ccd_gram_solve_kernel<NB>: a workgroup per long row.  First the 256 threads add the row's parts IN PART ORDER (one
//    chain per element, from the upper triangle only) into a full symmetric r_pad x r_pad image in the workspace (element
//    (i, j), i <= j, is stored to both places), b and the diagonal into LDS.  Done first, not fused into the sweep: the sweep is
//    one dependent chain per coordinate, and the parts of a row would put `parts` loads on every link of it.  Then wave 0 runs
//    section 23's sweep on the row's own matrix, k = 0 .. R-1:
//        s   = sum_{j != k} f_j Q[k][j]        lane l owns j = l + 64 m: one fmaf chain over m, the own term an exact +0,
//                                              then the xor butterfly 32 .. 1
//        f_k = max(eps, ((b_k - l1) - s) / ((Q[k][k] + l2) + eps))
//    Row k of the image is 4 r_pad bytes, coalesced, and row k + 1 is fetched before coordinate k is reduced.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_sparse_common.h"

namespace nmfmu {

using gq_f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr float kGqEps = 1.1920928955078125e-07f;   // 2^-23 = constants.eps
constexpr int kGqTile = 32;                          // entries per tile
constexpr int kGqMinPart = 256;                      // the library's shortest part: 8 tiles
constexpr int64_t kGqCapFloats = (int64_t)1 << 26;   // the workspace cap of nmfmu_sp_ntf_ccd_gram_part: 256 MiB

constexpr int gq_rpad(int rank) { return rank <= 32 ? 32 : rank <= 64 ? 64 : rank <= 128 ? 128 : 256; }
constexpr int gq_blocks(int nb) { return nb * (nb + 1) / 2; }                        // the blocks with bi <= bj
constexpr int64_t gq_part_floats(int rp) { return (int64_t)gq_blocks(rp / 32) * 1024 + rp; }

struct GqArgs {
  const int32_t* rowptr;
  const int32_t* idx_a;
  const int32_t* idx_b;
  const float* vals;
  const int32_t* rows;       // [n_long] the long rows
  const int32_t* row_part;   // [n_long + 1] the first part of every long row
  const int32_t* part_row;   // [n_parts] the position in `rows` of a part's row
  float* owner;
  const float* pa;
  const float* pb;
  float* ws;                 // [n_parts][blocks * 1024 + r_pad], then [n_long][r_pad][r_pad]
  int n_long, n_parts, part, rank;
  float l1, l2;
};

template <int NB, int G>
__global__ void __launch_bounds__(256) sp_ntf_ccd_gram_parts_kernel(GqArgs a) {
  constexpr int RP = 32 * NB, LD = RP == 32 ? 32 : RP + 32;
  constexpr int ES = NB <= 2 ? 4 : NB == 4 ? 2 : 1;   // waves that split a tile's entries
  constexpr int NP = 4 / ES;                          // pairs of block rows
  constexpr int NT = NB == 1 ? 1 : NB + 1;            // blocks of a wave
  constexpr int KS = kGqTile / ES / 2;                // k-steps of a wave per tile
  constexpr int NI = RP / (8 * G);                    // gather items of a thread per tile and panel
  constexpr int IPE = RP / G;                         // gather items of an entry
  static_assert(ES == 1 || NP * NT * 1024 <= 2 * kGqTile * LD, "the wave-order sum goes through the tile buffers");
  __shared__ __attribute__((aligned(16))) float sq[2 * kGqTile * LD];
  __shared__ float sv[2][kGqTile];
  __shared__ int32_t si[2][2][kGqTile];

  const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int part_at = blockIdx.x;
  const int r = a.part_row[part_at];
  const int row = a.rows[r];
  const int lo = a.rowptr[row] + (part_at - a.row_part[r]) * a.part, end = a.rowptr[row + 1];
  const int hi = end - lo > a.part ? lo + a.part : end;
  const int nt = (hi - lo + kGqTile - 1) / kGqTile;
  const int rank = a.rank;

  // the wave's blocks: t < na -- (ra, ra + t), else (rb, rb + t - na)
  const int pp = wave % NP, es = wave / NP;
  const int ra = pp, rb = NB - 1 - pp, na = NB - pp;
  gq_f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
  float bacc = 0.f;

  float xa[NI][G], xb[NI][G];      // the next tile's panel values on their way
  float vnext = 0.f;               // threads 64 .. 95: the next tile's values
  int32_t inext = 0;               // threads 0 .. 63: the index pairs of the tile after the next

  auto load_idx = [&](int tile) {                 // -> inext (threads 0 .. 63)
    const int e = lo + tile * kGqTile + (tid & 31);
    inext = 0;
    if (tid < 64 && tile < nt && e < hi) inext = (tid < 32 ? a.idx_a : a.idx_b)[e];
  };
  auto load_val = [&](int tile) {                 // -> vnext (threads 64 .. 95)
    const int e = lo + tile * kGqTile + (tid & 31);
    vnext = 0.f;
    if (tid >= 64 && tid < 96 && tile < nt && e < hi) vnext = a.vals[e];
  };
  auto gather = [&](int tile) {                   // si[tile & 1] -> xa, xb
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int it = tid + 256 * j, e = it / IPE, c0 = (it % IPE) * G;
#pragma unroll
      for (int g = 0; g < G; ++g) xa[j][g] = xb[j][g] = 0.f;
      if (lo + tile * kGqTile + e < hi && c0 < rank) {
        const float* pa = a.pa + (size_t)si[tile & 1][0][e] * rank + c0;
        const float* pb = a.pb + (size_t)si[tile & 1][1][e] * rank + c0;
        if constexpr (G == 4) {
          const float4 x = *reinterpret_cast<const float4*>(pa), y = *reinterpret_cast<const float4*>(pb);
          xa[j][0] = x.x, xa[j][1] = x.y, xa[j][2] = x.z, xa[j][3] = x.w;
          xb[j][0] = y.x, xb[j][1] = y.y, xb[j][2] = y.z, xb[j][3] = y.w;
        } else {
          xa[j][0] = pa[0], xb[j][0] = pb[0];
        }
      }
    }
  };
  auto store_q = [&](int tile) {                  // q = fl32(xa xb) -> sq[tile & 1] (an entry past the end, a padded column: 0)
    float* buf = sq + (tile & 1) * kGqTile * LD;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int it = tid + 256 * j, e = it / IPE, c0 = (it % IPE) * G;
      if constexpr (G == 4) {
        const float4 q = {__fmul_rn(xa[j][0], xb[j][0]), __fmul_rn(xa[j][1], xb[j][1]), __fmul_rn(xa[j][2], xb[j][2]),
                          __fmul_rn(xa[j][3], xb[j][3])};
        *reinterpret_cast<float4*>(buf + e * LD + c0) = q;
      } else {
        buf[e * LD + c0] = __fmul_rn(xa[j][0], xb[j][0]);
      }
    }
    if (tid >= 64 && tid < 96) sv[tile & 1][tid & 31] = vnext;
  };
  auto store_idx = [&](int tile) {
    if (tid < 64) si[tile & 1][tid >> 5][tid & 31] = inext;
  };

  // prologue: tile 0 staged, tile 1's index pairs in LDS
  load_idx(0);
  store_idx(0);
  load_idx(1);
  load_val(0);
  __syncthreads();
  gather(0);
  store_q(0);
  store_idx(1);
  __syncthreads();

  for (int tile = 0; tile < nt; ++tile) {
    if (tile + 1 < nt) gather(tile + 1);          // (uniform over the workgroup)
    load_val(tile + 1);
    load_idx(tile + 2);
    const float* buf = sq + (tile & 1) * kGqTile * LD;
    const float* rowp = buf + (es * (kGqTile / ES) + hl) * LD + (lane & 31);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float* rp = rowp + 2 * ks * LD;
      const float a0 = rp[32 * ra], a1 = rp[32 * rb];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bool first = t < na;
        const float bv = rp[32 * (first ? ra + t : rb + t - na)];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(first ? a0 : a1, bv, acc[t], 0, 0, 0);
      }
    }
    if (tid < RP) {
      const float* vp = sv[tile & 1];
#pragma unroll 8
      for (int e = 0; e < kGqTile; ++e) bacc = fmaf(vp[e], buf[e * LD + tid], bacc);
    }
    if (tile + 1 < nt) {
      store_q(tile + 1);
      store_idx(tile + 2);
    }
    __syncthreads();
  }

  // the waves that split the tiles' entries: their accumulators in wave order, through the tile buffers
  if constexpr (ES > 1) {
    float* stage = sq + pp * NT * 1024;
#pragma unroll 1
    for (int s2 = 1; s2 < ES; ++s2) {
      if (es == s2) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) stage[t * 1024 + v * 64 + lane] = acc[t][v];
      }
      __syncthreads();
      if (es == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[t][v] += stage[t * 1024 + v * 64 + lane];
      }
      __syncthreads();
    }
  }
  float* out = a.ws + (size_t)part_at * gq_part_floats(RP);
  if (es == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bool first = t < na;
      const int bi = first ? ra : rb, bj = first ? ra + t : rb + t - na;
      float* dst = out + (bi * NB - bi * (bi - 1) / 2 + (bj - bi)) * 1024 + (lane & 31);
#pragma unroll
      for (int v = 0; v < 16; ++v) dst[((v & 3) + 8 * (v >> 2) + 4 * hl) * 32] = acc[t][v];
    }
  }
  if (tid < RP) out[gq_blocks(NB) * 1024 + tid] = bacc;
}

template <int NB>
__global__ void __launch_bounds__(256) sp_ntf_ccd_gram_solve_kernel(GqArgs a) {
  constexpr int RP = 32 * NB, NBT = gq_blocks(NB), M = RP < 64 ? 1 : RP / 64;
  constexpr int64_t PER = gq_part_floats(RP);
  __shared__ float fs[RP], bs[RP], ds[RP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int r = blockIdx.x;
  const int row = a.rows[r], rank = a.rank;
  const int p0 = a.row_part[r], p1 = a.row_part[r + 1];
  const float* parts = a.ws;
  float* qf = a.ws + (size_t)a.n_parts * PER + (size_t)r * RP * RP;
  float* frow = a.owner + (size_t)row * rank;

  for (int at = tid; at < NBT * 1024; at += 256) {
    int bi = 0, rem = at >> 10;
    while (rem >= NB - bi) rem -= NB - bi, ++bi;
    const int gi = 32 * bi + ((at >> 5) & 31), gj = 32 * (bi + rem) + (at & 31);
    if (gi > gj) continue;                          // the upper triangle only: symmetric by construction
    float sum = parts[(size_t)p0 * PER + at];
#pragma unroll 4
    for (int p = p0 + 1; p < p1; ++p) sum += parts[(size_t)p * PER + at];
    qf[gi * RP + gj] = sum;
    if (gi != gj) qf[gj * RP + gi] = sum;
    else ds[gi] = sum;
  }
  if (tid < RP) {
    float sum = parts[(size_t)p0 * PER + NBT * 1024 + tid];
#pragma unroll 4
    for (int p = p0 + 1; p < p1; ++p) sum += parts[(size_t)p * PER + NBT * 1024 + tid];
    bs[tid] = sum;
    fs[tid] = tid < rank ? frow[tid] : 0.f;
  }
  __syncthreads();
  if (tid >= 64) return;

  float f[M], q[M], qn[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int j = lane + 64 * m;
    f[m] = j < RP ? fs[j] : 0.f;
    qn[m] = j < RP ? qf[j] : 0.f;
  }
  for (int k = 0; k < rank; ++k) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int j = lane + 64 * m;
      q[m] = qn[m];
      if (k + 1 < rank && j < RP) qn[m] = qf[(k + 1) * RP + j];
    }
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) s = fmaf(lane + 64 * m == k ? 0.f : f[m], q[m], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float num = (bs[k] - a.l1) - s;
    const float den = (ds[k] + a.l2) + kGqEps;
    const float fn = fmaxf(kGqEps, num / den);      // (a NaN quotient gives eps)
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (lane + 64 * m == k) f[m] = fn;
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int j = lane + 64 * m;
    if (j < rank) frow[j] = f[m];
  }
}

template <int NB>
static void gq_launch(const GqArgs& a, bool wide, hipStream_t s) {
  if (wide) hipLaunchKernelGGL((sp_ntf_ccd_gram_parts_kernel<NB, 4>), dim3((unsigned)a.n_parts), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((sp_ntf_ccd_gram_parts_kernel<NB, 1>), dim3((unsigned)a.n_parts), dim3(256), 0, s, a);
  hipLaunchKernelGGL((sp_ntf_ccd_gram_solve_kernel<NB>), dim3((unsigned)a.n_long), dim3(256), 0, s, a);
}

}  // namespace nmfmu

using namespace nmfmu;

extern "C" {

int64_t nmfmu_sp_ntf_ccd_gram_ws(int n_parts, int n_long, int rank) {
  if (n_parts <= 0 || n_long <= 0 || n_long > n_parts || rank <= 0 || rank > 256) return 0;
  const int rp = gq_rpad(rank);
  return (int64_t)n_parts * gq_part_floats(rp) + (int64_t)n_long * rp * rp;
}

int nmfmu_sp_ntf_ccd_gram_part(int64_t entries, int n_long, int longest, int rank, int cus) {
  if (entries <= 0 || n_long <= 0 || longest <= 0 || longest > entries || rank <= 0 || rank > 256) return 0;
  if (cus <= 0) cus = 256;
  const int rp = gq_rpad(rank);
  // parts the cap admits when every part came with a row's image (a batch of rows has at most as many rows as parts)
  const int64_t most = kGqCapFloats / (gq_part_floats(rp) + (int64_t)rp * rp);
  int64_t want = 4 * (int64_t)cus;                                  // a small multiple of the CU count ...
  if (want > most) want = most;                                     // ... unless the cap asks for fewer, longer parts
  const int64_t split = want > 2 * (int64_t)n_long ? want - n_long : want / 2;   // sum ceil(c / part) <= entries / part + n_long
  int64_t part = (entries + split - 1) / split;
  const int64_t alone = ((int64_t)longest + most - 2) / (most - 1);   // the longest row alone stays under the cap
  if (part < alone) part = alone;
  if (part < kGqMinPart) part = kGqMinPart;
  part = (part + 31) / 32 * 32;
  return (int)part;      // (entries < 2^31 over at least 326 splits)
}

int nmfmu_sp_ntf_ccd_gram(const int32_t* rowptr, const int32_t* idx_a, const int32_t* idx_b, const float* vals,
                          const int32_t* rows, const int32_t* row_part, const int32_t* part_row, int n_long, int n_parts,
                          int part, float* owner, const float* pa, int rows_a, const float* pb, int rows_b, int rank, float l1,
                          float l2, float* ws, int vec, void* stream) {
  if (!rowptr || !idx_a || !idx_b || !vals || !rows || !row_part || !part_row || !owner || !pa || !pb || !ws || owner == pa ||
      owner == pb)
    return NMFMU_ERR_ARG;
  if (n_long <= 0 || n_parts < n_long || rows_a <= 0 || rows_b <= 0 || rank <= 0 || part <= 0 || part % 32 != 0 || vec < 0 ||
      vec > 2)
    return NMFMU_ERR_ARG;
  if (rank > 256) return NMFMU_ERR_UNSUPPORTED;
  GqArgs a;
  a.rowptr = rowptr, a.idx_a = idx_a, a.idx_b = idx_b, a.vals = vals, a.rows = rows, a.row_part = row_part;
  a.part_row = part_row, a.owner = owner, a.pa = pa, a.pb = pb, a.ws = ws;
  a.n_long = n_long, a.n_parts = n_parts, a.part = part, a.rank = rank, a.l1 = l1, a.l2 = l2;
  // four-wide: every panel row starts on a 16-byte boundary
  const bool wide = vec != 1 && rank % 4 == 0 && ((uintptr_t)pa | (uintptr_t)pb) % 16 == 0;
  switch (gq_rpad(rank)) {
    case 32: gq_launch<1>(a, wide, S(stream)); break;
    case 64: gq_launch<2>(a, wide, S(stream)); break;
    case 128: gq_launch<4>(a, wide, S(stream)); break;
    default: gq_launch<8>(a, wide, S(stream)); break;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
