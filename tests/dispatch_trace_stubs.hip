// TEST-ONLY stand-in for every kernel unit that csrc/nmfmu_capi.hip links against (tools/make_golden_dispatch.py,
// tests/test_dispatch_trace.py).  It defines the nmfmu:: launchers and queries that nmfmu_capi.o leaves undefined, plus
// nmfmu_comm_allreduce_sum_f32.  A launcher launches nothing: it appends one line to a log -- its name, its scalar arguments,
// every field of FusedArgs / ApplyArgs, pointers as their offset from a base address (or `null`) -- and returns 0, so that
// what the C ABI decides for a half-step can be read on a machine without a GPU.  No HIP runtime call is made here.
#include <cstdio>
#include <string>
#include <type_traits>

// (found through -I: the headers of the csrc tree whose nmfmu_capi.hip this unit is linked with, and that tree's include/)
#include "nmfmu.h"
#include "nmfmu_aux.h"
#include "nmfmu_fused.h"
#include "nmfmu_pp.h"
#include "nmfmu_sp.h"
#include "nmfmu_sp128.h"
#include "nmfmu_sp2.h"

namespace {

std::string g_log, g_out;
const char* g_base = nullptr;

void put(const nmfmu::FusedArgs& a);
void put(const nmfmu::ApplyArgs& a);
template <class T>
void put(const T& v) {
  char buf[48];
  if constexpr (std::is_pointer_v<T>) {
    if (!v) {
      g_log += "null";
      return;
    }
    std::snprintf(buf, sizeof buf, "+%td", reinterpret_cast<const char*>(v) - g_base);
  } else if constexpr (std::is_floating_point_v<T>) {
    std::snprintf(buf, sizeof buf, "%.9g", (double)v);
  } else {
    std::snprintf(buf, sizeof buf, "%lld", (long long)v);
  }
  g_log += buf;
}
#define FIELD(x) (g_log += " " #x "=", put(a.x))
void put(const nmfmu::FusedArgs& a) {
  g_log += "{";
  FIELD(xp), FIELD(p1_hi), FIELD(p1_lo), FIELD(p2_hi), FIELD(p2_lo), FIELD(a1_hi), FIELD(a1_lo), FIELD(slab_num), FIELD(slab_den);
  FIELD(loss_part), FIELD(M), FIELD(K), FIELD(M_pad), FIELD(ktiles), FIELD(nsplit), FIELD(tiles_per_split), FIELD(beta);
  FIELD(fuse_apply), FIELD(rank), FIELD(f), FIELD(kl_den), FIELD(o1_hi), FIELD(o1_lo), FIELD(o2_hi), FIELD(o2_lo), FIELD(colsum_part);
  FIELD(l1), FIELD(l2), FIELD(gamma), FIELD(cs_owner), FIELD(cs_panel), FIELD(gram_hi), FIELD(gram_lo), FIELD(gram_scale);
  FIELD(status), FIELD(debug);
  g_log += " }";
}
void put(const nmfmu::ApplyArgs& a) {
  g_log += "{";
  FIELD(f), FIELD(num), FIELD(den), FIELD(kl_den), FIELD(nslab), FIELD(p1_hi), FIELD(p1_lo), FIELD(p2_hi), FIELD(p2_lo);
  FIELD(colsum_part), FIELD(colsum), FIELD(rows), FIELD(rank), FIELD(rows_pad), FIELD(l1), FIELD(l2), FIELD(gamma), FIELD(scale);
  FIELD(trainer), FIELD(ortho), FIELD(grad), FIELD(f16), FIELD(status), FIELD(den_nslab), FIELD(skip_colsum);
  g_log += " }";
}
#undef FIELD

template <class... A>
int line(const char* name, const A&... a) {
  g_log += name;
  ((g_log += ' ', put(a)), ...);
  g_log += '\n';
  return 0;
}

}  // namespace

// The log since the last call (valid until the next one); pointers logged from now on are offsets from `base`.
extern "C" const char* nmfmu_trace_take(const void* base) {
  g_out.swap(g_log);
  g_log.clear();
  g_base = static_cast<const char*>(base);
  return g_out.c_str();
}

extern "C" int nmfmu_comm_allreduce_sum_f32(nmfmu_comm* comm, float* buf, size_t count, void* stream) {
  return line("comm_allreduce_sum_f32", comm, buf, count, stream);
}

namespace nmfmu {

// the three queries answer as the kernel units do (nmfmu_inst_pp.hip, nmfmu_inst_sp128.hip, nmfmu_aux.hip)
bool pp_trl_available(int r_pad, int opt, int mode) { return r_pad == 128 && (opt == kOpBf16 || opt == kOpF16) && mode == kModeMU; }
bool sp128_available(int r_pad, int opt, int mode) { return r_pad == 128 && opt == kOpF16 && mode == kModeMU; }
int apply_stripe_rows(int rows_pad) { return rows_pad / 64 < 512 ? 16 : 64; }

int launch_fused_r32(int beta_kind, int prec, int mode, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_fused_r32", beta_kind, prec, mode, a, grid, s);
}
int launch_fused_r64(int beta_kind, int prec, int mode, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_fused_r64", beta_kind, prec, mode, a, grid, s);
}
int launch_fused_r128(int beta_kind, int prec, int mode, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_fused_r128", beta_kind, prec, mode, a, grid, s);
}
int launch_fused_r256(int beta_kind, int prec, int mode, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_fused_r256", beta_kind, prec, mode, a, grid, s);
}
int launch_pp(int r_pad, int opt, int mode, const FusedArgs& a, int grid, hipStream_t s, bool xr, bool lacc, bool trl) {
  return line("launch_pp", r_pad, opt, mode, a, grid, s, xr, lacc, trl);
}
int launch_sp(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) { return line("launch_sp", r_pad, opt, a, grid, s); }
int launch_sp2(int r_pad, int beta_kind, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_sp2", r_pad, beta_kind, a, grid, s);
}
int launch_sp128(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) { return line("launch_sp128", r_pad, opt, a, grid, s); }
int launch_sp128_rb0(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) {
  return line("launch_sp128_rb0", r_pad, opt, a, grid, s);
}

int launch_pack_x(const float* v, int64_t ld, int rows, int cols, bool transpose, int fmt, void* xp, int m_pad, int k_pad,
                  uint32_t* flags, int G, hipStream_t s) {
  return line("launch_pack_x", v, ld, rows, cols, transpose, fmt, xp, m_pad, k_pad, flags, G, s);
}
int launch_apply(int r_pad, const ApplyArgs& a, bool x3, bool pack_only, hipStream_t s) {
  return line("launch_apply", r_pad, a, x3, pack_only, s);
}
int launch_colsum_finalize(const float* part, int nblk, int r_pad, float* out, hipStream_t s) {
  return line("launch_colsum_finalize", part, nblk, r_pad, out, s);
}
int launch_slab_reduce(const float* slab, int nslab, int64_t plane, float* out, hipStream_t s) {
  return line("launch_slab_reduce", slab, nslab, plane, out, s);
}
int launch_sum_finalize_f32(const float* part, int n, double* out, hipStream_t s) { return line("launch_sum_finalize_f32", part, n, out, s); }
int launch_target_sums(const float* v, int64_t ld, int rows, int cols, double* part, int nparts, double* out4, hipStream_t s) {
  return line("launch_target_sums", v, ld, rows, cols, part, nparts, out4, s);
}
int launch_riding_finish(const float* part, int npairs, const double* ac, double n_all, const uint32_t* status, double* out2,
                         hipStream_t s) {
  return line("launch_riding_finish", part, npairs, ac, n_all, status, out2, s);
}
int launch_checkpoint(const float* part, int n, const uint32_t* status, double* out, const float* a, float* a_snap, int64_t na,
                      const float* b, float* b_snap, int64_t nb, hipStream_t s) {
  return line("launch_checkpoint", part, n, status, out, a, a_snap, na, b, b_snap, nb, s);
}
int launch_beta_div(const float* x, const float* y, int64_t n, float beta, int kind, double* part, double* out, hipStream_t s) {
  return line("launch_beta_div", x, y, n, beta, kind, part, out, s);
}
int launch_mu_terms(const float* s, const float* v, int64_t n, float beta, int kind, float* gn, float* gp, hipStream_t st) {
  return line("launch_mu_terms", s, v, n, beta, kind, gn, gp, st);
}
int launch_beta_div_grad(const float* x, const float* y, int64_t n, float beta, int kind, const float* upstream, float* gx,
                         hipStream_t st) {
  return line("launch_beta_div_grad", x, y, n, beta, kind, upstream, gx, st);
}
int launch_trainer_update(float* f, int rows, int cols, const float* neg, const float* pos, float l1, float l2, float ortho,
                          float gamma, float* grad, hipStream_t st) {
  return line("launch_trainer_update", f, rows, cols, neg, pos, l1, l2, ortho, gamma, grad, st);
}
int launch_norms(const float* x, int64_t n, double* part, double* out, hipStream_t s) { return line("launch_norms", x, n, part, out, s); }
int launch_reconstruct(const float* A, int M, const float* B, int K, int R, float* out, int64_t ld, hipStream_t s) {
  return line("launch_reconstruct", A, M, B, K, R, out, ld, s);
}
int64_t backward_ws_floats(int m, int k, int rank, bool want_owner, bool want_panel, int* splits) {
  return line("backward_ws_floats", m, k, rank, want_owner, want_panel, splits);
}
int launch_reconstruct_backward(const float* G, int64_t ld, int m, int k, const float* owner, const float* panel, int rank,
                                float* grad_owner, float* grad_panel, float* ws, hipStream_t s) {
  return line("launch_reconstruct_backward", G, ld, m, k, owner, panel, rank, grad_owner, grad_panel, ws, s);
}
int64_t conv_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, bool want_h,
                                bool want_w, int* splits) {
  return line("conv_backward_ws_floats", batch, channels, rank, ndim, lh, taps, want_h, want_w, splits);
}
int launch_conv_backward(const float* G, const float* W, const float* H, int batch, int channels, int rank, int ndim,
                         const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* ws, hipStream_t st) {
  return line("launch_conv_backward", G, W, H, batch, channels, rank, ndim, lh, taps, grad_h, grad_w, ws, st);
}
int64_t plca_backward_ws_floats(int m, int k, int rank, bool want_h, bool want_w, bool want_z, int* info) {
  return line("plca_backward_ws_floats", m, k, rank, want_h, want_w, want_z, info);
}
int launch_plca_backward(const float* G, int64_t ld, int m, int k, const float* H, const float* W, const float* Z, int rank,
                         float* grad_h, float* grad_w, float* grad_z, float* ws, hipStream_t s) {
  return line("launch_plca_backward", G, ld, m, k, H, W, Z, rank, grad_h, grad_w, grad_z, ws, s);
}
int64_t conv_plca_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                                     bool want_h, bool want_w, bool want_z, int* info) {
  return line("conv_plca_backward_ws_floats", batch, channels, rank, ndim, lh, taps, want_h, want_w, want_z, info);
}
int launch_conv_plca_backward(const float* G, const float* W, const float* H, const float* Z, int batch, int channels, int rank,
                              int ndim, const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* grad_z,
                              float* ws, hipStream_t s) {
  return line("launch_conv_plca_backward", G, W, H, Z, batch, channels, rank, ndim, lh, taps, grad_h, grad_w, grad_z, ws, s);
}
int launch_probe_mfma(const uint16_t* a, const uint16_t* b, float* d, hipStream_t s) { return line("launch_probe_mfma", a, b, d, s); }
int launch_probe_lds_dma(const uint32_t* src, uint32_t* dst, int n_dwords, hipStream_t s) {
  return line("launch_probe_lds_dma", src, dst, n_dwords, s);
}
int launch_ubench_mfma_hbm(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile, int waves,
                           int tiles, int grid, float* out, hipStream_t s, int wrap_tiles, unsigned long long* stamps) {
  return line("launch_ubench_mfma_hbm", operands, operand_bytes, f16, stream_src, kib_per_tile, waves, tiles, grid, out, s, wrap_tiles,
              stamps);
}

}  // namespace nmfmu
