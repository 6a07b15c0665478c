// Launchers of the auxiliary (non-MFMA) kernels; see nmfmu_aux.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct nmfmu_step;   // include/nmfmu.h

namespace nmfmu {

struct ApplyArgs {
  float* f;             // fp32 master [rows][rank]
  const float* num;     // [nslab][rows_pad][R_PAD]
  const float* den;     // same or nullptr
  const float* kl_den;  // [R_PAD] or nullptr
  int nslab;
  void* p1_hi;
  void* p1_lo;
  void* p2_hi;
  void* p2_lo;
  float* colsum_part;   // [rows_pad/16][R_PAD] (worst case)
  float* colsum;        // [R_PAD]
  int rows, rank, rows_pad;
  float l1, l2, gamma;
  // trainer.BetaMu semantics (trainer.py:93-112) instead of fit's (nmf.py:78-92): eps added after the penalties,
  // orthogonality penalty, and grad[row][r] = relu(den) - relu(num) written out (p.grad of trainer.py:98)
  const float* scale;   // PACK_ONLY: images (and column sums) of f[row][r] * scale[r]; the master is not touched
  int trainer;
  float ortho;
  float* grad;          // [rows][rank] or nullptr
  int f16;              // images in fp16 (clamped to 65504) instead of bf16; no lo planes
  uint32_t* status;     // or nullptr: bit 0 is set when an fp16 image value had to be clamped
  int den_nslab;        // slabs of `den` when it differs from nslab (kModeXB leaves ONE denominator slab); 0 = nslab
  int skip_colsum;      // do not launch the column-sum finalize (beta == 2: nothing reads the column sums)
};

int apply_stripe_rows(int rows_pad);   // rows per apply workgroup (= rows per column-sum partial): 16 or 64

// fmt: 0 = bf16, 1 = fp32, 2 = fp16 (clamped to 65504)
int launch_pack_x(const float* v, int64_t ld, int rows, int cols, bool transpose, int fmt, void* xp, int m_pad,
                  int k_pad, uint32_t* flags, int G, hipStream_t s);
int launch_apply(int r_pad, const ApplyArgs& a, bool x3, bool pack_only, hipStream_t s);
int launch_colsum_finalize(const float* part, int nblk, int r_pad, float* out, hipStream_t s);
int launch_slab_reduce(const float* slab, int nslab, int64_t plane, float* out, hipStream_t s);
int launch_sum_finalize_f32(const float* part, int n, double* out, hipStream_t s);
int launch_target_sums(const float* v, int64_t ld, int rows, int cols, double* part, int nparts, double* out4, hipStream_t s);
int launch_riding_finish(const float* part, int npairs, const double* ac, double n_all, const uint32_t* status, double* out2,
                         hipStream_t s);
int launch_checkpoint(const float* part, int n, const uint32_t* status, double* out, const float* a, float* a_snap, int64_t na,
                      const float* b, float* b_snap, int64_t nb, hipStream_t s);
int launch_beta_div(const float* x, const float* y, int64_t n, float beta, int kind, double* part, double* out,
                    hipStream_t s);
int launch_mu_terms(const float* s, const float* v, int64_t n, float beta, int kind, float* gn, float* gp, hipStream_t st);
int launch_beta_div_grad(const float* x, const float* y, int64_t n, float beta, int kind, const float* upstream, float* gx,
                         hipStream_t st);
int launch_trainer_update(float* f, int rows, int cols, const float* neg, const float* pos, float l1, float l2, float ortho,
                          float gamma, float* grad, hipStream_t st);
int launch_norms(const float* x, int64_t n, double* part, double* out, hipStream_t s);
int launch_reconstruct(const float* A, int M, const float* B, int K, int R, float* out, int64_t ld, hipStream_t s);
// nmfmu_autograd.hip: backward of launch_reconstruct.  backward_nsplit is the split rule (parts of the contraction per
// output tile, a pure function of the shape); ws holds the [nsplit][rows][R] slabs of the halves that are split.
int backward_nsplit(int rows, int contraction, int rank);
int backward_part_len(int contraction, int nsplit);
// out[i] = ((slab[0][i] + slab[1][i]) + ...) over `plane` floats: slab_sum_kernel, parts added in part order
int launch_slab_sum(const float* slab, int nslab, int64_t plane, float* out, hipStream_t s);
int64_t backward_ws_floats(int m, int k, int rank, bool want_owner, bool want_panel, int* splits);
int launch_reconstruct_backward(const float* G, int64_t ld, int m, int k, const float* owner, const float* panel, int rank,
                                float* grad_owner, float* grad_panel, float* ws, hipStream_t s);
// nmfmu_conv_autograd.hip: backward of the convolutive reconstruction (NMFD / NMF2D / NMF3D), 1..3 shift axes.  Same split rule
// (rows = the output's long axis: B prod(lh) for grad_h, C prod(taps) for grad_w; contraction = the other one) and slab scheme.
// Both return -1 for sizes that are not positive or do not fit the kernel's 32-bit flattened axes (2^30).
int64_t conv_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, bool want_h,
                                bool want_w, int* splits);
int launch_conv_backward(const float* G, const float* W, const float* H, int batch, int channels, int rank, int ndim,
                         const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* ws, hipStream_t st);
// the product kernel of ONE half alone (no slab sum): backward_nsplit parts to dst = [parts][output]
int launch_backward_product(bool trans, const float* G, int64_t ld, int rows, int C, const float* B, int R, float* dst,
                            hipStream_t s);
int launch_conv_backward_product(bool w_half, const float* G, const float* F, int batch, int channels, int rank, int ndim,
                                 const int32_t* lh, const int32_t* taps, float* dst, hipStream_t st);
// nmfmu_plca_autograd.hip: backward of the PLCA / SIPLCA reconstructions (H, W, Z).  plca_finish_grid is the workgroup rule of
// the finishing kernel over an output [outer][rank][inner] (include/nmfmu.h states it): nbo chunks of `chunk` outer indices
// times nseg segments of `seg` inner positions.  info: {parts H, parts W, blocks H, blocks W, half of grad_Z (0 / 1 = H / 2 = W)}.
struct PlcaFinishGrid {
  int nbo, chunk, nseg, seg;
  int blocks() const { return nbo * nseg; }
};
PlcaFinishGrid plca_finish_grid(int64_t outer, int rank, int64_t inner);
int64_t plca_backward_ws_floats(int m, int k, int rank, bool want_h, bool want_w, bool want_z, int* info);
int launch_plca_backward(const float* G, int64_t ld, int m, int k, const float* H, const float* W, const float* Z, int rank,
                         float* grad_h, float* grad_w, float* grad_z, float* ws, hipStream_t s);
int64_t conv_plca_backward_ws_floats(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                                     bool want_h, bool want_w, bool want_z, int* info);
int launch_conv_plca_backward(const float* G, const float* W, const float* H, const float* Z, int batch, int channels, int rank,
                              int ndim, const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* grad_z,
                              float* ws, hipStream_t s);
// nmfmu_ard.hip: the apply stage with a per-component penalty (ARD-NMF) and its relevance update.  ApplyArgs as for
// launch_apply (l1 / l2 / the trainer fields are not read); pen: [r_pad]; l2_prior: pos += pen[r] * f instead of pos += pen[r];
// norm_part: [rows_pad / 16][r_pad] (worst case; the 'l2' prior only), norm: [r_pad]
int launch_ard_apply(int r_pad, const ApplyArgs& a, bool x3, const float* pen, bool l2_prior, float* norm_part, float* norm,
                     hipStream_t s);
// the apply stage's side of the one-image stages (nmfmu_capi.hip: apply_image_rule): NMFMU_OK or the refusal; *writes_p2: the
// owner's transposed images are written
int apply_writes_p2(const nmfmu_step* st, bool* writes_p2);
int launch_ard_relevance(const float* norm_w, const float* norm_h, int rank, int r_pad, float b, float c, float phi, float* lam,
                         float* pen, float* delta, hipStream_t s);
int launch_probe_mfma(const uint16_t* a, const uint16_t* b, float* d, hipStream_t s);
int launch_probe_lds_dma(const uint32_t* src, uint32_t* dst, int n_dwords, hipStream_t s);
int launch_ubench_mfma_hbm(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile,
                           int waves, int tiles, int grid, float* out, hipStream_t s, int wrap_tiles = 0,
                           unsigned long long* stamps = nullptr);

}  // namespace nmfmu
