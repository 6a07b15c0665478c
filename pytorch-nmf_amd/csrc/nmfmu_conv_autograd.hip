// Backward of the convolutive reconstruction out[b,c,p] = sum_r sum_t W[c,r,t] H[b,r,p-t] (NMFD / NMF2D / NMF3D.reconstruct;
// p, t, j multi-indices over 1..3 shift axes, L_a = Lh_a + T_a - 1 per axis) for torch.autograd, G = d loss / d out:
//   grad_H[b,r,j] = sum_c sum_t W[c,r,t] G[b,c,j+t]        contraction over (c, t)
//   grad_W[c,r,t] = sum_b sum_j G[b,c,j+t] H[b,r,j]        contraction over (b, j)
// The convolution is full, so j + t is always inside G: no boundary case.  With goff(x) = (x0 L1 + x1) L2 + x2 the element of G
// is G[(b C + c) PL + goff(j) + goff(t)], and goff is linear -- the address is a sum of a (b, j) term and a (c, t) term.  Both
// halves are therefore ONE product
//   out[o][r] = sum_k F[k][r] G[gbase(o) + gbase(k)]
// over two flattened axes x = (outer, inner multi-index): gbase(x) = outer * gstride + goff(inner); the factor element is
// F[fbase(k) + r * inner_k] and the output element out[fbase(o) + r * inner_o], fbase(x) = outer * R * inner + inner index --
// the (B, R, *Lh) / (C, R, *T) layouts themselves.  grad_H: o = (b, j), k = (c, t), F = W;  grad_W: o = (c, t), k = (b, j), F = H.
// The Toeplitz operand exists only in LDS: every staged element of G is fetched with its own computed index (32 k terms per
// stage from a small LDS table, the o term kept in a register); nothing Pi T times an input is ever written to HBM.
//
// Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), tile and staging idiom of reconstruct_backward_kernel (nmfmu_autograd.hip): the
// contraction staged through LDS 32 steps at a time, the rank on the MFMA's row (register) index and o on its column (lane)
// index, so a store instruction writes 32 consecutive o -- consecutive floats of the output layout.  The rank tile is 32
// (one 32 x 32 accumulator per wave, four waves side by side along o) for R <= 32 and 128 (2 x 2 per wave) above; 128 o
// per workgroup either way.  The contraction is cut into parts by backward_nsplit (nmfmu_autograd.hip; its rank-tile count
// ceil(R / 128) is this kernel's too), partials go to a caller-owned slab [parts][output] and slab_sum_kernel adds them in
// part order: no floating-point atomics, bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "nmfmu_aux.h"

namespace nmfmu {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kCvBK = 32;     // contraction steps per LDS stage; a part is a whole number of stages (backward_part_len)
constexpr int kCvBO = 128;    // o positions per workgroup

// One flattened axis x = outer * inner + (x0 d1 + x1) d2 + x2 of the product above.
struct ConvAxis {
  int n;            // outer * inner
  int inner;        // d0 d1 d2: Pi Lh for (b, j), Pi T for (c, t)
  int d1, d2;
  int64_t gstride;  // elements of G per outer step: C * Pi L for b, Pi L for c
};

struct ConvBackwardArgs {
  ConvAxis o, k;
  int R, l1, l2;    // rank; L of the two inner shift axes
  int part_len;
};

// (offset into G, offset into the factor / output of rank 0) of index x; 64-bit element offsets
__device__ __forceinline__ void conv_axis_terms(const ConvAxis& ax, int x, int R, int l1, int l2, int64_t& g, int64_t& f) {
  const int outer = x / ax.inner, in = x - outer * ax.inner;
  const int q = in / ax.d2, x2 = in - q * ax.d2;
  const int x0 = q / ax.d1, x1 = q - x0 * ax.d1;
  g = (int64_t)outer * ax.gstride + ((int64_t)x0 * l1 + x1) * l2 + x2;
  f = (int64_t)outer * R * ax.inner + in;
}

// out (+ part * R * o.n) [fbase(o) + r * o.inner] = sum_{k in part} F[fbase(k) + r * k.inner] G[gbase(o) + gbase(k)]
// grid = (o tiles, rank tiles, parts).  RT = rank tile, 32 or 128.
template <int RT>
__global__ void __launch_bounds__(256) conv_backward_kernel(const float* __restrict__ G, const float* __restrict__ F,
                                                            ConvBackwardArgs a, float* __restrict__ out) {
  constexpr int NA = RT == 128 ? 2 : 1;          // 32 x 32 accumulators per wave: NA along the rank, NA along o
  constexpr int WT = 32 * NA;                    // a wave's tile is WT ranks x WT o
  constexpr int LDF = RT + 1;                    // sf[k][r]: written with lanes along k (odd stride), read along r
  __shared__ float sg[kCvBK * kCvBO];            // sg[k][o]: lanes along o both ways
  __shared__ float sf[kCvBK * LDF];
  __shared__ int64_t tg[2][kCvBK], tf[2][kCvBK]; // gbase(k), fbase(k) of a stage's 32 k (-1 outside the part); double buffered
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hl = lane >> 5, wave = tid >> 6;
  const int wr = RT == 128 ? wave >> 1 : 0, wo = RT == 128 ? wave & 1 : wave;
  const int o0 = blockIdx.x * kCvBO, r0 = blockIdx.y * RT;
  const int kbeg = blockIdx.z * a.part_len, kend = min(a.k.n, kbeg + a.part_len);   // axes <= 2^30 (conv_shape): kbeg cannot wrap
  f32x16 acc[NA][NA];
#pragma unroll
  for (int x = 0; x < NA; ++x)
#pragma unroll
    for (int y = 0; y < NA; ++y)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[x][y][e] = 0.f;
  // this thread stages column o0 + (tid & 127) of sg, rows (tid >> 7) + 2 p
  const int so = tid & (kCvBO - 1), sk0 = tid >> 7;
  int64_t og = -1, of_unused;
  if (o0 + so < a.o.n) conv_axis_terms(a.o, o0 + so, a.R, a.l1, a.l2, og, of_unused);
  auto fill_table = [&](int buf, int k0) {
    if (tid < kCvBK) {
      int64_t g = -1, f = -1;
      if (k0 + tid < kend) conv_axis_terms(a.k, k0 + tid, a.R, a.l1, a.l2, g, f);
      tg[buf][tid] = g, tf[buf][tid] = f;
    }
  };
  fill_table(0, kbeg);
  __syncthreads();
  int cur = 0;
  for (int k0 = kbeg; k0 < kend; k0 += kCvBK, cur ^= 1) {
    // stage G(o0 .. o0+127, k0 .. k0+31) and F(k0 .. k0+31, r0 .. r0+RT-1), zero outside the axes / the part
#pragma unroll
    for (int p = 0; p < kCvBK / 2; ++p) {
      const int kr = sk0 + 2 * p;
      const int64_t kg = tg[cur][kr];
      sg[kr * kCvBO + so] = (og >= 0 && kg >= 0) ? G[og + kg] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < RT / 8; ++p) {
      const int idx = p * 256 + tid, kr = idx & (kCvBK - 1), r = idx >> 5;       // lanes along k: consecutive floats of F
      const int64_t kf = tf[cur][kr];
      sf[kr * LDF + r] = (kf >= 0 && r0 + r < a.R) ? F[kf + (int64_t)(r0 + r) * a.k.inner] : 0.f;
    }
    fill_table(cur ^ 1, k0 + kCvBK);             // the next stage's table; its last readers passed the barrier below
    __syncthreads();
    const float* pa = sf + hl * LDF + wr * WT + j;
    const float* pb = sg + hl * kCvBO + wo * WT + j;
#pragma unroll
    for (int s2 = 0; s2 < kCvBK; s2 += 2) {
      float av[NA], bv[NA];
#pragma unroll
      for (int x = 0; x < NA; ++x) av[x] = pa[s2 * LDF + 32 * x], bv[x] = pb[s2 * kCvBO + 32 * x];
#pragma unroll
      for (int x = 0; x < NA; ++x)
#pragma unroll
        for (int y = 0; y < NA; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
    __syncthreads();
  }
  float* dst = out + (int64_t)blockIdx.z * a.R * a.o.n;
#pragma unroll
  for (int y = 0; y < NA; ++y) {
    const int o = o0 + wo * WT + y * 32 + j;
    if (o < a.o.n) {
      int64_t g_unused, ofs;
      conv_axis_terms(a.o, o, a.R, a.l1, a.l2, g_unused, ofs);
#pragma unroll
      for (int x = 0; x < NA; ++x)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = r0 + wr * WT + x * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          if (r < a.R) dst[ofs + (int64_t)r * a.o.inner] = acc[x][y][e];
        }
    }
  }
}

namespace {

struct ConvShape {
  int64_t bj, ct, pl;     // B * Pi Lh, C * Pi T, Pi L
  int lh[3], taps[3];     // leading ones for ndim < 3
};

// sizes the kernel indexes with int: both flattened axes and (for the parts' rounding) a little headroom
constexpr int64_t kCvMaxAxis = (int64_t)1 << 30;

bool conv_shape(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, ConvShape* s) {
  if (batch <= 0 || channels <= 0 || rank <= 0 || ndim < 1 || ndim > 3 || !lh || !taps) return false;
  int64_t pj = 1, pt = 1, pl = 1;
  for (int d = 0; d < 3; ++d) {
    const int src = d - (3 - ndim);
    s->lh[d] = src < 0 ? 1 : lh[src], s->taps[d] = src < 0 ? 1 : taps[src];
    if (s->lh[d] <= 0 || s->taps[d] <= 0) return false;
    pj *= s->lh[d], pt *= s->taps[d], pl *= (int64_t)s->lh[d] + s->taps[d] - 1;
    if (pj > kCvMaxAxis || pt > kCvMaxAxis || pl > ((int64_t)1 << 40)) return false;
  }
  s->bj = batch * pj, s->ct = channels * pt, s->pl = pl;
  return s->bj <= kCvMaxAxis && s->ct <= kCvMaxAxis && rank <= (1 << 20);
}

ConvAxis conv_axis(int64_t n, const int* d, int64_t gstride) {
  return ConvAxis{(int)n, d[0] * d[1] * d[2], d[1], d[2], gstride};
}

// the product kernel alone: backward_nsplit(o.n, k.n, R) parts to dst ([parts][output]; the output itself with one part)
int conv_backward_product(const float* G, const float* F, const ConvAxis& o, const ConvAxis& k, int R, const ConvShape& s,
                          float* dst, hipStream_t st) {
  const int nsplit = backward_nsplit(o.n, k.n, R);
  ConvBackwardArgs a{o, k, R, s.lh[1] + s.taps[1] - 1, s.lh[2] + s.taps[2] - 1, backward_part_len(k.n, nsplit)};
  if (R <= 32)
    hipLaunchKernelGGL(conv_backward_kernel<32>, dim3((o.n + kCvBO - 1) / kCvBO, 1, nsplit), dim3(256), 0, st, G, F, a, dst);
  else
    hipLaunchKernelGGL(conv_backward_kernel<128>, dim3((o.n + kCvBO - 1) / kCvBO, (R + 127) / 128, nsplit), dim3(256), 0, st,
                       G, F, a, dst);
  return (int)hipGetLastError();
}

int conv_backward_half(const float* G, const float* F, const ConvAxis& o, const ConvAxis& k, int R, const ConvShape& s, float* out,
                       float* slab, hipStream_t st) {
  const int nsplit = backward_nsplit(o.n, k.n, R);
  int e = conv_backward_product(G, F, o, k, R, s, nsplit > 1 ? slab : out, st);
  if (e || nsplit == 1) return e;
  return launch_slab_sum(slab, nsplit, (int64_t)R * o.n, out, st);
}

}  // namespace

int64_t conv_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, bool want_h,
                                bool want_w, int* splits) {
  ConvShape s;
  if (!conv_shape(batch, channels, rank, ndim, lh, taps, &s)) return -1;
  const int sh = want_h ? backward_nsplit((int)s.bj, (int)s.ct, rank) : 0;
  const int sw = want_w ? backward_nsplit((int)s.ct, (int)s.bj, rank) : 0;
  if (splits) splits[0] = sh, splits[1] = sw;
  return (sh > 1 ? sh * s.bj * rank : 0) + (sw > 1 ? sw * s.ct * rank : 0);
}

int launch_conv_backward(const float* G, const float* W, const float* H, int batch, int channels, int rank, int ndim,
                         const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* ws, hipStream_t st) {
  ConvShape s;
  if (!conv_shape(batch, channels, rank, ndim, lh, taps, &s)) return -1;
  const ConvAxis bj = conv_axis(s.bj, s.lh, (int64_t)channels * s.pl), ct = conv_axis(s.ct, s.taps, s.pl);
  float* slab_w = ws;
  if (grad_h) {
    const int sh = backward_nsplit(bj.n, ct.n, rank);
    int e = conv_backward_half(G, W, bj, ct, rank, s, grad_h, ws, st);
    if (e) return e;
    if (sh > 1) slab_w = ws + sh * s.bj * rank;
  }
  if (grad_w) return conv_backward_half(G, H, ct, bj, rank, s, grad_w, slab_w, st);
  return 0;
}

// One half's product kernel alone (w_half: grad_w's, F = H; else grad_h's, F = W), its parts to dst: what
// nmfmu_plca_autograd.hip finishes itself.  -1 for the sizes conv_backward_ws_floats rejects.
int launch_conv_backward_product(bool w_half, const float* G, const float* F, int batch, int channels, int rank, int ndim,
                                 const int32_t* lh, const int32_t* taps, float* dst, hipStream_t st) {
  ConvShape s;
  if (!conv_shape(batch, channels, rank, ndim, lh, taps, &s)) return -1;
  const ConvAxis bj = conv_axis(s.bj, s.lh, (int64_t)channels * s.pl), ct = conv_axis(s.ct, s.taps, s.pl);
  return w_half ? conv_backward_product(G, F, ct, bj, rank, s, dst, st) : conv_backward_product(G, F, bj, ct, rank, s, dst, st);
}

}  // namespace nmfmu
