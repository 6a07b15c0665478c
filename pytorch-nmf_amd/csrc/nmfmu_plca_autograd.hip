// Backward of the PLCA reconstructions for torch.autograd: out = H diag(Z) W^T (PLCA) and out = convNd(H, (W Z).flip, padding =
// T - 1) (SIPLCA / SIPLCA2 / SIPLCA3), G = d loss / d out.  Z indexes the rank axis, which neither product contracts, so it
// factors out of both:
//   rawH = backward_H(G, W)  (unscaled W)        grad_H[.., r, ..] = Z[r] rawH[.., r, ..]
//   rawW = backward_W(G, H)                      grad_W[c, r, ..] = Z[r] rawW[c, r, ..]
//   grad_Z[r] = sum_{c,t} rawW[c,r,t] W[c,r,t]   ( = sum_{b,j} rawH[b,r,j] H[b,r,j] )
// rawH / rawW come from the exact-fp32 MFMA product kernels of nmfmu_autograd.hip / nmfmu_conv_autograd.hip, unchanged, through
// launch_backward_product / launch_conv_backward_product; no W Z temporary exists.  This file holds what finishes them: ONE
// pass per half over the output seen as [outer][R][inner] (dense: inner = 1; conv: outer = B or C, inner = prod(Lh) or prod(T))
// that adds the `parts` partial slabs in part order (it REPLACES slab_sum_kernel, so a split half costs no extra pass; with one
// part it runs in place over the product's output), multiplies by z[r], stores the gradient when it is wanted and accumulates
// sum raw F per rank against the factor F of the same layout when grad_Z is wanted.
//
// Determinism.  Workgroup (x, y) owns outer indices [x chunk, (x + 1) chunk) and inner positions [y seg, (y + 1) seg)
// (plca_finish_grid: a pure function of the shape).  Inside it every thread owns fixed ranks and walks its elements in a fixed
// order; the threads' sums meet in LDS and ONE thread per rank adds them in thread order; the workgroup's R sums go to
// zpart[y gridDim.x + x][R], and plca_zsum_kernel adds those in block order (a fixed association).  No floating-point atomics, no fences, no
// cooperative launch: bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "nmfmu_aux.h"

namespace nmfmu {

namespace {

constexpr int kFinThreads = 256;
constexpr int64_t kFinElemsPerWg = 8192;   // output elements a finishing workgroup should own at least ...
constexpr int kFinMaxWgs = 2048;           // ... and the most workgroups along one grid axis
constexpr int kFinMinSeg = 1024;           // an inner segment is at least this long
constexpr int kFinUnroll = 4;              // rows in flight per thread (dense)

struct FinishArgs {
  const float* src;    // [parts][outer][R][inner] raw partial products; src == dst when parts == 1 and the product wrote in place
  float* dst;          // the gradient [outer][R][inner], or nullptr
  const float* z;      // [R]
  const float* fac;    // the factor whose layout the output has, or nullptr: no per-rank sums
  float* zpart;        // [workgroups][R]
  int64_t plane;       // outer * R * inner
  int parts, outer, R, inner;
  int chunk, seg;      // outer indices / inner positions per workgroup
  int gs;              // conv: threads per line group (a power of two <= 256)
};

template <int VW>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ static Vec load(const float* p) { return Vec{{*p}}; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ static Vec load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    return Vec{{q.x, q.y, q.z, q.w}};
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ((slab[0] + slab[1]) + slab[2]) + ... at element offset e: the order of slab_sum_kernel
template <int VW>
__device__ __forceinline__ Vec<VW> sum_parts(const FinishArgs& a, int64_t e) {
  Vec<VW> v = Vec<VW>::load(a.src + e);
  for (int s = 1; s < a.parts; ++s) {
    const Vec<VW> w = Vec<VW>::load(a.src + (int64_t)s * a.plane + e);
#pragma unroll
    for (int q = 0; q < VW; ++q) v.v[q] += w.v[q];
  }
  return v;
}

// Dense output [rows][R] (inner == 1).  A thread owns VW consecutive ranks and every TY-th row of the workgroup's chunk; the
// active threads of one step cover TY consecutive rows, i.e. consecutive floats.  Ranks beyond 256 VW take further passes.
template <int VW>
__global__ void __launch_bounds__(kFinThreads) plca_finish_dense_kernel(FinishArgs a) {
  __shared__ float sm[kFinThreads * VW];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * a.chunk, row1 = min(a.outer, row0 + a.chunk);
  const int ncv = (a.R + VW - 1) / VW;                        // VW == 4 only with R % 4 == 0
  for (int cp = 0; cp < ncv; cp += kFinThreads) {
    const int nc = min(kFinThreads, ncv - cp), ty_n = kFinThreads / nc;
    const int tx = tid % nc, ty = tid / nc;
    const int col = (cp + tx) * VW;
    float acc[VW];
#pragma unroll
    for (int q = 0; q < VW; ++q) acc[q] = 0.f;
    if (ty < ty_n) {
      const Vec<VW> zv = Vec<VW>::load(a.z + col);
      for (int row = row0 + ty; row < row1; row += kFinUnroll * ty_n) {
        Vec<VW> raw[kFinUnroll], f[kFinUnroll];
#pragma unroll
        for (int u = 0; u < kFinUnroll; ++u) {
          const int rr = row + u * ty_n;
          if (rr < row1) {
            const int64_t e = (int64_t)rr * a.R + col;
            raw[u] = sum_parts<VW>(a, e);
            if (a.fac) f[u] = Vec<VW>::load(a.fac + e);
          }
        }
#pragma unroll
        for (int u = 0; u < kFinUnroll; ++u) {
          const int rr = row + u * ty_n;
          if (rr < row1) {
            const int64_t e = (int64_t)rr * a.R + col;
            if (a.fac) {
#pragma unroll
              for (int q = 0; q < VW; ++q) acc[q] += raw[u].v[q] * f[u].v[q];
            }
            if (a.dst) {
              Vec<VW> o;
#pragma unroll
              for (int q = 0; q < VW; ++q) o.v[q] = raw[u].v[q] * zv.v[q];
              o.store(a.dst + e);
            }
          }
        }
      }
    }
    if (a.fac) {                                               // (uniform) sm[ty][nc * VW] -> one thread per rank, ty order
      if (ty < ty_n) {
#pragma unroll
        for (int q = 0; q < VW; ++q) sm[(ty * nc + tx) * VW + q] = acc[q];
      }
      __syncthreads();
      for (int c = tid; c < nc * VW; c += kFinThreads) {        // (nc VW <= 1024 rank sums of this pass)
        float s = sm[c];
        for (int y = 1; y < ty_n; ++y) s += sm[y * nc * VW + c];
        a.zpart[(int64_t)blockIdx.x * a.R + cp * VW + c] = s;
      }
      __syncthreads();
    }
  }
}

// Output [outer][R][inner], inner > 1.  A group of gs threads owns one line (o, r, inner segment) at a time: group (gy, gx) the
// rank cp + gx and every GY-th outer index of the chunk, neighbouring groups neighbouring ranks -- neighbouring lines of the
// layout.  Ranks beyond the 256 / gs groups take further passes.
template <int VW>
__global__ void __launch_bounds__(kFinThreads) plca_finish_lines_kernel(FinishArgs a) {
  __shared__ float sm[kFinThreads];
  const int tid = threadIdx.x, gs = a.gs, ng = kFinThreads / gs;
  const int g = tid / gs, li = tid - g * gs;
  const int o0 = blockIdx.x * a.chunk, o1 = min(a.outer, o0 + a.chunk);
  const int i0 = blockIdx.y * a.seg, i1 = min(a.inner, i0 + a.seg);      // VW == 4: inner % 4 == 0 and seg % 4 == 0
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int cp = 0; cp < a.R; cp += ng) {
    const int nc = min(ng, a.R - cp), gy_n = ng / nc;
    const int gx = g % nc, gy = g / nc, r = cp + gx;
    float acc = 0.f;
    if (gy < gy_n) {
      const float zr = a.z[r];
      for (int o = o0 + gy; o < o1; o += gy_n) {
        const int64_t base = ((int64_t)o * a.R + r) * a.inner;
        for (int i = i0 + li * VW; i < i1; i += gs * VW) {
          const Vec<VW> raw = sum_parts<VW>(a, base + i);
          if (a.fac) {
            const Vec<VW> f = Vec<VW>::load(a.fac + base + i);
#pragma unroll
            for (int q = 0; q < VW; ++q) acc += raw.v[q] * f.v[q];
          }
          if (a.dst) {
            Vec<VW> o4;
#pragma unroll
            for (int q = 0; q < VW; ++q) o4.v[q] = raw.v[q] * zr;
            o4.store(a.dst + base + i);
          }
        }
      }
    }
    if (a.fac) {                                               // (uniform) one thread per rank adds its groups' threads in order
      sm[tid] = acc;                                           // idle groups hold 0 and are not read
      __syncthreads();
      if (tid < nc) {
        float s = 0.f;
        for (int y = 0; y < gy_n; ++y)
          for (int l = 0; l < gs; ++l) s += sm[(y * nc + tid) * gs + l];
        a.zpart[blk * a.R + cp + tid] = s;
      }
      __syncthreads();
    }
  }
}

// grad_z[r] = sum over blocks of zpart[block][r], in block order: 16 lanes per rank add 16 consecutive ranges of blocks, each in
// block order (four loads in flight), and one thread adds the 16 range sums in range order.  16 ranks per workgroup.
constexpr int kZsRanks = 16, kZsLanes = 16;
__global__ void __launch_bounds__(kZsRanks * kZsLanes) plca_zsum_kernel(const float* __restrict__ zpart, int blocks, int R,
                                                                        float* __restrict__ grad_z) {
  __shared__ float sm[kZsLanes][kZsRanks];
  const int tx = threadIdx.x % kZsRanks, ty = threadIdx.x / kZsRanks;
  const int r = blockIdx.x * kZsRanks + tx;
  const int per = (blocks + kZsLanes - 1) / kZsLanes;
  const int b0 = ty * per, b1 = min(blocks, b0 + per);
  float s = 0.f;
  if (r < R) {
    for (int b = b0; b < b1; b += 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = b + u < b1 ? zpart[(int64_t)(b + u) * R + r] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u];
    }
  }
  sm[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && r < R) {
    float t = sm[0][tx];
    for (int y = 1; y < kZsLanes; ++y) t += sm[y][tx];
    grad_z[r] = t;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_finish(const float* src, int parts, float* dst, const float* z, const float* fac, float* zpart, int64_t outer, int R,
                  int64_t inner, hipStream_t s) {
  const PlcaFinishGrid fg = plca_finish_grid(outer, R, inner);
  FinishArgs a{src, dst, z, fac, zpart, outer * R * inner, parts, (int)outer, R, (int)inner, fg.chunk, fg.seg, 1};
  // 16-byte accesses need 16-byte aligned rows / lines: the rule of reconstruct_backward_kernel
  const bool ptrs = aligned16(src) && (!dst || aligned16(dst)) && (!fac || aligned16(fac)) && (a.plane & 3) == 0;
  if (inner == 1) {
    if (ptrs && (R & 3) == 0 && aligned16(z))
      hipLaunchKernelGGL(plca_finish_dense_kernel<4>, dim3(fg.nbo), dim3(kFinThreads), 0, s, a);
    else
      hipLaunchKernelGGL(plca_finish_dense_kernel<1>, dim3(fg.nbo), dim3(kFinThreads), 0, s, a);
  } else {
    const bool vec = ptrs && (inner & 3) == 0;
    const int64_t lv = (std::min<int64_t>(fg.seg, inner) + (vec ? 3 : 0)) / (vec ? 4 : 1);
    while (a.gs < lv && a.gs < kFinThreads) a.gs *= 2;
    if (vec)
      hipLaunchKernelGGL(plca_finish_lines_kernel<4>, dim3(fg.nbo, fg.nseg), dim3(kFinThreads), 0, s, a);
    else
      hipLaunchKernelGGL(plca_finish_lines_kernel<1>, dim3(fg.nbo, fg.nseg), dim3(kFinThreads), 0, s, a);
  }
  return (int)hipGetLastError();
}

int launch_zsum(const float* zpart, int blocks, int R, float* grad_z, hipStream_t s) {
  hipLaunchKernelGGL(plca_zsum_kernel, dim3((R + kZsRanks - 1) / kZsRanks), dim3(kZsRanks * kZsLanes), 0, s, zpart, blocks, R,
                     grad_z);
  return (int)hipGetLastError();
}

// One half as the entries below see it
struct Half {
  bool run = false, z = false;    // launched at all; feeds grad_Z
  int parts = 0, blocks = 0;
  int64_t elems = 0;              // outer * R * inner
  int64_t slab_floats = 0;        // scratch of the raw product: round4(parts * elems) when split or when the gradient itself is not wanted
};

struct Plan {
  Half h, w;
  int64_t zpart_floats = 0;
  int64_t ws_floats() const { return h.slab_floats + w.slab_floats + zpart_floats; }
};

int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }   // every region of ws starts 16-byte aligned when ws is

// The half-selection rule of include/nmfmu.h
Plan make_plan(bool want_h, bool want_w, bool want_z, int parts_h, int parts_w, int64_t outer_h, int64_t inner_h, int64_t outer_w,
               int64_t inner_w, int R) {
  Plan p;
  p.h.run = want_h;
  p.h.z = want_z && want_h && !want_w;
  p.w.run = want_w || (want_z && !want_h);
  p.w.z = want_z && !p.h.z;
  if (p.h.run) {
    p.h.parts = parts_h, p.h.elems = outer_h * R * inner_h, p.h.blocks = plca_finish_grid(outer_h, R, inner_h).blocks();
    p.h.slab_floats = parts_h > 1 ? round4(parts_h * p.h.elems) : 0;
  }
  if (p.w.run) {
    p.w.parts = parts_w, p.w.elems = outer_w * R * inner_w, p.w.blocks = plca_finish_grid(outer_w, R, inner_w).blocks();
    p.w.slab_floats = (parts_w > 1 || !want_w) ? round4(parts_w * p.w.elems) : 0;
  }
  if (want_z) p.zpart_floats = (int64_t)(p.h.z ? p.h.blocks : p.w.blocks) * R;
  return p;
}

void plan_info(const Plan& p, int* info) {
  if (!info) return;
  info[0] = p.h.parts, info[1] = p.w.parts, info[2] = p.h.blocks, info[3] = p.w.blocks;
  info[4] = p.h.z ? 1 : (p.w.z ? 2 : 0);
}

}  // namespace

PlcaFinishGrid plca_finish_grid(int64_t outer, int rank, int64_t inner) {
  const int64_t per = (int64_t)rank * inner;                   // <= 2^50 (rank <= 2^20, inner <= 2^30)
  const int64_t want = per >= kFinElemsPerWg * kFinMaxWgs
                           ? kFinMaxWgs
                           : std::min<int64_t>(kFinMaxWgs, (outer * per + kFinElemsPerWg - 1) / kFinElemsPerWg);
  PlcaFinishGrid g;
  const int64_t nbo = std::min(want, outer);
  g.chunk = (int)((outer + nbo - 1) / nbo);
  g.nbo = (int)((outer + g.chunk - 1) / g.chunk);
  g.nseg = 1, g.seg = (int)inner;
  if (inner > 1) {
    const int64_t ns = std::max<int64_t>(1, std::min((want + g.nbo - 1) / g.nbo, inner / kFinMinSeg));
    g.seg = (int)(((inner + ns - 1) / ns + 3) / 4 * 4);
    g.nseg = (int)((inner + g.seg - 1) / g.seg);
  }
  return g;
}

int64_t plca_backward_ws_floats(int m, int k, int rank, bool want_h, bool want_w, bool want_z, int* info) {
  const Plan p = make_plan(want_h, want_w, want_z, backward_nsplit(m, k, rank), backward_nsplit(k, m, rank), m, 1, k, 1, rank);
  plan_info(p, info);
  return p.ws_floats();
}

int launch_plca_backward(const float* G, int64_t ld, int m, int k, const float* H, const float* W, const float* Z, int rank,
                         float* grad_h, float* grad_w, float* grad_z, float* ws, hipStream_t s) {
  const Plan p = make_plan(grad_h != nullptr, grad_w != nullptr, grad_z != nullptr, backward_nsplit(m, k, rank),
                           backward_nsplit(k, m, rank), m, 1, k, 1, rank);
  float* slab_h = ws;
  float* slab_w = ws + p.h.slab_floats;
  float* zpart = slab_w + p.w.slab_floats;
  if (p.h.run) {
    float* raw = p.h.slab_floats ? slab_h : grad_h;
    int e = launch_backward_product(false, G, ld, m, k, W, rank, raw, s);
    if (!e) e = launch_finish(raw, p.h.parts, grad_h, Z, p.h.z ? H : nullptr, zpart, m, rank, 1, s);
    if (e) return e;
  }
  if (p.w.run) {
    float* raw = p.w.slab_floats ? slab_w : grad_w;
    int e = launch_backward_product(true, G, ld, k, m, H, rank, raw, s);
    if (!e) e = launch_finish(raw, p.w.parts, grad_w, Z, p.w.z ? W : nullptr, zpart, k, rank, 1, s);
    if (e) return e;
  }
  if (grad_z) return launch_zsum(zpart, p.h.z ? p.h.blocks : p.w.blocks, rank, grad_z, s);
  return 0;
}

namespace {

// B prod(lh), C prod(taps) and the two inner sizes, or false for what launch_conv_backward rejects
bool conv_sizes(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, int64_t* pj, int64_t* pt) {
  if (conv_backward_ws_floats(batch, channels, rank, ndim, lh, taps, true, true, nullptr) < 0) return false;
  *pj = 1, *pt = 1;
  for (int d = 0; d < ndim; ++d) *pj *= lh[d], *pt *= taps[d];
  return true;
}

Plan conv_plan(int batch, int channels, int rank, int64_t pj, int64_t pt, bool want_h, bool want_w, bool want_z) {
  const int bj = (int)(batch * pj), ct = (int)(channels * pt);
  return make_plan(want_h, want_w, want_z, backward_nsplit(bj, ct, rank), backward_nsplit(ct, bj, rank), batch, pj, channels, pt,
                   rank);
}

}  // namespace

int64_t conv_plca_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                                     bool want_h, bool want_w, bool want_z, int* info) {
  int64_t pj, pt;
  if (!conv_sizes(batch, channels, rank, ndim, lh, taps, &pj, &pt)) return -1;
  const Plan p = conv_plan(batch, channels, rank, pj, pt, want_h, want_w, want_z);
  plan_info(p, info);
  return p.ws_floats();
}

int launch_conv_plca_backward(const float* G, const float* W, const float* H, const float* Z, int batch, int channels, int rank,
                              int ndim, const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* grad_z,
                              float* ws, hipStream_t s) {
  int64_t pj, pt;
  if (!conv_sizes(batch, channels, rank, ndim, lh, taps, &pj, &pt)) return -1;
  const Plan p = conv_plan(batch, channels, rank, pj, pt, grad_h != nullptr, grad_w != nullptr, grad_z != nullptr);
  float* slab_h = ws;
  float* slab_w = ws + p.h.slab_floats;
  float* zpart = slab_w + p.w.slab_floats;
  if (p.h.run) {
    float* raw = p.h.slab_floats ? slab_h : grad_h;
    int e = launch_conv_backward_product(false, G, W, batch, channels, rank, ndim, lh, taps, raw, s);
    if (!e) e = launch_finish(raw, p.h.parts, grad_h, Z, p.h.z ? H : nullptr, zpart, batch, rank, pj, s);
    if (e) return e;
  }
  if (p.w.run) {
    float* raw = p.w.slab_floats ? slab_w : grad_w;
    int e = launch_conv_backward_product(true, G, H, batch, channels, rank, ndim, lh, taps, raw, s);
    if (!e) e = launch_finish(raw, p.w.parts, grad_w, Z, p.w.z ? W : nullptr, zpart, channels, rank, pt, s);
    if (e) return e;
  }
  if (grad_z) return launch_zsum(zpart, p.h.z ? p.h.blocks : p.w.blocks, rank, grad_z, s);
  return 0;
}

}  // namespace nmfmu
