/* nmfmu.h -- C ABI of the MI355X-native NMF multiplicative-update engine.
 *
 * This is the drop-in boundary for the one hot path of yoyololicon/pytorch-NMF
 * (torchnmf 0.3.5) that this project accelerates: the dense beta-divergence MU
 * iteration of `torchnmf.nmf.NMF.fit` / `NMFD.fit`.  The reference has no FFI
 * of its own (it is pure Python over ATen), so each entry point below names the
 * reference code it replaces (file:line under the reference checkout).  A
 * maintainer's binding (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer unless noted;
 *  - the library never allocates device memory: the caller owns every buffer
 *    and sizes it with the nmfmu_*_bytes() queries;
 *  - every call enqueues work on `stream` (a hipStream_t passed as void*) and
 *    returns without synchronising; no hidden host<->device sync;
 *  - return value: 0 = NMFMU_OK, > 0 = a hipError_t, < 0 = NMFMU_ERR_*;
 *  - re-entrant; one host thread per device.
 *
 * Orientation.  The reference factorises V (N x C) ~ H (N x R) @ W (C x R)^T
 * (nmf.py:659-662).  A half-step updates one factor (the "owner", M rows) using
 * the other (the "panel", K rows) and X = V (H half-step) or V^T (W half-step),
 * stored in a kernel-specific tiled layout (see csrc/nmfmu_layout.h).
 */
#ifndef NMFMU_H_
#define NMFMU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMFMU_ABI_VERSION 10 /* 2: nmfmu_gemm_desc grew the implicit-operand fields; trainer / convnd / tables entries;
                               3: nmfmu_gemm_desc.tile_rows, NMFMU_EPI_FOLD, NMFMU_PREC_F16;
                               4: NMFMU_PREC_F16 for every beta and padded rank 256 (four-wave kernel); nmfmu_mu_step_parts /
                                  nmfmu_parts_supported / nmfmu_gemm_tile256_supported removed (measured neutral / not faster);
                                  NMFMU_STAGE_REG and the 256 x 256 GEMM tile no longer built; nmfmu_step.status;
                               5: nmfmu_gemm_desc.rag_c0 / rag_channels (ragged channels inside the GEMM grid), nmfmu_gemm_ragged_supported,
                                  nmfmu_conv_fold_parts_apply_h_tables / nmfmu_fold_hsum_parts_tables;
                               6: NMFMU_PREC_F16X (fp16 operands, fp32 target); nmfmu_gram_panel / nmfmu_xb_* (beta == 2 without
                                  the reconstruction); NMFMU_ERR_ALLOC;
                               7: nmfmu_gemm_desc.win_* / NMFMU_OPS_A_WIN (H numerator of NMFD / NMF2D / NMF3D without the unfolded Y),
                                  nmfmu_conv_pack_wk, nmfmu_conv_apply_h_rows; nmfmu_gemm_desc.t_koff, nmfmu_convnd_tables / _table_bytes / _koff (implicit
                                  operands with several shift axes);
                               8: nmfmu_abi_check (load-time guard for bindings that are not the bundled Python host),
                                  nmfmu_ubench_mfma_hbm (in-run ceiling of the MU step for bench.py); the NMFD GEMMs stage an implicit
                                  operand as a sliding window of table entries where its tiles hold no padding (nmfmu_gemm_desc.stage_mode,
                                  nmfmu_gemm_window_staged); nmfmu_conv_apply_pack_w_wk / nmfmu_conv_apply_h_rows_sums / nmfmu_conv_h_rows_parts;
                               9: nmfmu_kernel_family / nmfmu_choose_nsplit_for (round 6: beta == 1 at padded rank 256 with fp16 operands runs the
                                  software-pipelined one-wave-per-SIMD kernel, ONE workgroup per CU -- the split must know the kernel);
                                  nmfmu_step.stamps (in-kernel clock stamps in the product build); nmfmu_ubench_mfma_hbm2;
                                  NMFMU_PREC_F16R (3-byte target);
                                  still 9, purely additive: nmfmu_reconstruct_backward / nmfmu_reconstruct_backward_ws /
                                  nmfmu_beta_div_grad (torch.autograd through NMF.forward and the divergences);
                                  nmfmu_conv_backward / nmfmu_conv_backward_ws (the same through NMFD / NMF2D / NMF3D.forward);
                                  nmfmu_hoyer_project / nmfmu_hoyer_project_ws (batched Hoyer projection behind sparse_fit and
                                  trainer.SparsityProj);
                                  nmfmu_plca_backward / nmfmu_plca_backward_ws / nmfmu_conv_plca_backward /
                                  nmfmu_conv_plca_backward_ws (torch.autograd through PLCA / SIPLCA / SIPLCA2 / SIPLCA3.forward:
                                  the two products above, finished with the latent vector Z);
                                  nmfmu_sp_masked_terms / nmfmu_sp_masked_step / nmfmu_sp_masked_loss / nmfmu_sp_masked_ws
                                  (missing-data NMF: sparse targets fitted over their stored entries only, every beta);
                                  nmfmu_sp_plca_estep / nmfmu_sp_plca_gather (PLCA.fit on sparse-COO targets: the E-step over
                                  the stored entries; added at ABI 10, additive);
                                  nmfmu_score_pairs / nmfmu_topk / nmfmu_topk_ws (scoring a fitted model: values at (row, column)
                                  pairs and the k best columns per row; added at ABI 10, additive);
                                  nmfmu_fold_in / nmfmu_fold_in_block (NMF.transform: new rows folded into a fitted model, every
                                  iteration of a row in one launch; added at ABI 10, additive);
                                  nmfmu_hals_sweep (NMF.fit(solver='hals'): the coordinate-descent sweep over the rank for
                                  beta == 2; added at ABI 10, additive);
                                  nmfmu_sp_ccd_sweep / nmfmu_sp_ccd_limit / nmfmu_sp_ccd_wg_waves / nmfmu_sp_ccd_lds_rows (NMF.fit(solver='ccd'):
                                  coordinate descent over the stored entries of a missing-data target, beta == 2; added at
                                  ABI 10, additive);
                                  nmfmu_sp_wccd_sweep (NMF.fit(solver='ccd', unstored=omega): the same sweep with every
                                  unstored entry a zero of confidence omega, 0 < omega < 1; added at ABI 10, additive);
                                  nmfmu_fold_in_cd / nmfmu_fold_in_cd_block / nmfmu_fold_in_cd_long_rows (NMF.transform_cd(solver='ccd' |
                                  'hals'): new rows folded in by coordinate descent, every iteration of a row in one launch;
                                  added at ABI 10, additive);
                                  nmfmu_rank_pairs / nmfmu_rank_pass / nmfmu_rank_ws (full-ranking evaluation: the rank of every
                                  held-out pair among the admissible columns of its row; added at ABI 10, additive);
                                  nmfmu_wmu_terms / nmfmu_wmu_step / nmfmu_wmu_loss / nmfmu_wmu_ws / nmfmu_wmu_nsplit /
                                  nmfmu_wmu_loss_parts (NMF.fit(V, weights=M): dense per-entry weights or a dense mask on one
                                  fused exact-fp32 MFMA kernel; added at ABI 10, additive);
                                  nmfmu_bmu_terms / nmfmu_bmu_step / nmfmu_bmu_loss / nmfmu_bmu_v_term / nmfmu_bmu_judge / nmfmu_bmu_ws /
                                  nmfmu_bmu_nsplit / nmfmu_bmu_loss_parts (batched.BatchedNMF: many problems of one shape per
                                  launch, each stopped on the device; added at ABI 10, additive);
                                  nmfmu_bwmu_terms / nmfmu_bwmu_step / nmfmu_bwmu_loss / nmfmu_bwmu_v_term (the batched entries with
                                  per-problem dense weights and a per-problem regulariser: weighted BatchedNMF and
                                  model_selection.cross_validate; added at ABI 10, additive);
                                  nmfmu_separate / nmfmu_separate_planes / nmfmu_separate_accumulate / nmfmu_separate_max_rank / nmfmu_separate_tables_bytes
                                  (separation.separate: per-group soft masks of a fitted model times the mixture; added at ABI 10,
                                  additive);
                                  nmfmu_ard_apply / nmfmu_ard_relevance (NMF.fit_ard: the apply stage with a per-component
                                  penalty and the relevance update of ARD-NMF; added at ABI 10, additive);
                               10: nmfmu_plca_normalize / nmfmu_plca_z / nmfmu_plca3 take alpha as double (an argument changed its
                                  type: not additive).  The Dirichlet prior adds fp32(alpha - 1) with the subtraction in double,
                                  as the reference's in-place add does; fp32(alpha) - 1.f was off by 4.7e-5 relative at
                                  alpha = 1.001 */

#define NMFMU_OK 0
#define NMFMU_ERR_UNSUPPORTED (-2) /* rank / precision / beta combination not built */
#define NMFMU_ERR_ARG (-3)         /* inconsistent sizes or null pointer */
#define NMFMU_ERR_ALLOC (-4)       /* a host allocation inside the library failed (communicator / timer handles) */

/* precision of the MFMA operands (accumulation is always fp32, factors are kept in fp32) */
#define NMFMU_PREC_BF16 0   /* X stored bf16; operands bf16                                   */
#define NMFMU_PREC_BF16X3 1 /* X stored fp32; operands split hi+lo, 3 MFMAs per product        */
#define NMFMU_PREC_F16 2    /* X stored fp16; operands fp16 (11 significant bits, same MFMA rate as bf16); values are
                               clamped to 65504 when packed, conversions saturate.  The single-plane mode that meets the
                               reference within 1e-4 at the BASELINE shapes.  beta == 1 at padded rank <= 128 runs on the
                               ping-pong kernel (nmfmu_pp.h), everything else on the four-wave kernel (nmfmu_fused.h) */
#define NMFMU_PREC_F16X 3   /* X stored fp32 (nmfmu_xp_bytes: 4 bytes per element), operands fp16: the target is never rounded
                               (nmf.py:65 is where X enters; it stays in fp32 VALU arithmetic, for beta == 2 it is an fp16
                               hi + lo operand pair), so the mode is parity-grade on targets fp16 does not hold exactly, at 1x
                               MFMA work and twice the X stream.  Four-wave kernel, every beta, padded rank <= 256 */
#define NMFMU_PREC_F16R 4   /* (ABI 9) as F16X at THREE bytes per element of X: the target rounded (nearest even) to the top 24 bits
                               of its fp32 word -- 16 significant bits (relative error <= 2^-16), fp32's whole range -- stored as
                               the f16 layout's 16-bit words (bits 31..16) plus one byte per element (bits 15..8); the kernels
                               rebuild the fp32 with one v_perm_b32 per element.  What 'auto' takes for a target fp16 does not
                               hold exactly.  beta == 1 at padded rank <= 128: ping-pong kernel; every other beta but 2: the
                               four-wave kernel, padded rank <= 256 */

/* beta branches of nmf.py:61-74 / metrics.py:78-96 */
#define NMFMU_BETA_KL 0  /* beta == 1 */
#define NMFMU_BETA_EUC 1 /* beta == 2 */
#define NMFMU_BETA_IS 2  /* beta == 0 */
#define NMFMU_BETA_GEN 3 /* anything else */

/* how the panel tile reaches LDS */
#define NMFMU_STAGE_REG 0 /* global -> VGPR -> ds_write: no longer built, NMFMU_ERR_UNSUPPORTED */
#define NMFMU_STAGE_DMA 1 /* global_load_lds (LDS-DMA)  */
#define NMFMU_STAGE_DMA_NOP2 3 /* (ABI 9) as NMFMU_STAGE_DMA, and the caller promises that NOTHING reads the transposed images (p2_*) of
                                  this step's factors: where the step's kernel does not read the panel's p2 itself -- beta == 1 at
                                  padded rank 256 with fp16 operands (the software-pipelined kernel: ONE image + transposing LDS
                                  reads) -- the fused apply / nmfmu_mu_apply no longer refresh the owner's p2 (64 of the 384 KiB a
                                  workgroup's epilogue moves).  Everywhere else it behaves as NMFMU_STAGE_DMA */
#define NMFMU_STAGE_DMA_LDSTR 4 /* as NMFMU_STAGE_DMA, for the steps nmfmu_pp_lds_transpose_supported() names (the ping-pong kernel's
                                   MU half-step at padded rank 128): the kernel fetches ONE panel image (p1) and builds the
                                   transposed tile of the second GEMM in LDS from it (ds_read_b64_tr_b16 + ds_write_b64 in the
                                   elementwise segments; same operands, same MFMA order: bit-identical results) -- half the
                                   L2 -> LDS panel stream.  The caller promises that NOTHING reads the transposed images (p2_*) of
                                   this step's factors: the step neither reads panel.p2_* nor refreshes owner.p2_* (fused apply and
                                   nmfmu_mu_apply / nmfmu_trainer_apply alike; the buffers must still be allocated).  nmfmu_loss
                                   treats it as NMFMU_STAGE_DMA; any other step answers NMFMU_ERR_UNSUPPORTED.  Appended under
                                   ABI 9: no struct layout changes */
#define NMFMU_STAGE_DMA_SP128 5 /* as NMFMU_STAGE_DMA_LDSTR (same promise about p2_*, same steps refused), and the MU half-step with
                                   fp16 operands and a 2-byte target (NMFMU_PREC_F16) at padded rank 128 runs the
                                   software-pipelined four-wave kernel with 64 owner rows per wave (nmfmu_sp128.h; tiles per
                                   workgroup rounded up to a multiple of four): same MFMA order per accumulator, bit-identical
                                   results at equal contraction splits.  The loss-carrying half-step stays on the ping-pong kernel;
                                   any other precision answers NMFMU_ERR_UNSUPPORTED.  Appended under ABI 10: no struct layout changes */
#define NMFMU_STAGE_DMA_SP128_RB0 6 /* as NMFMU_STAGE_DMA_SP128 in every respect but the placement of the kernel's ratio stage: the
                                       whole of a tile's ratio stage stays behind the first GEMM of the next tile (RB = 0 in
                                       nmfmu_sp128.h), where NMFMU_STAGE_DMA_SP128 runs the shipped placement.  Bit-identical
                                       results; kept as the other arm of an A/B in one library.  No struct layout changes */
#define NMFMU_STAGE_DMA_SPLIT 2 /* as NMFMU_STAGE_DMA, and panel.p1_* / panel.p2_* are images of DIFFERENT matrices (PLCA: the
                                   Z-scaled factor for the reconstruction, the unscaled one for the second GEMM).  Since ABI 6
                                   the single-plane four-wave kernels stage ONE panel image and gather the second GEMM's
                                   operands from it (ds_read_b64_tr_b16); a split panel must say so.  beta == 1, nmfmu_mu_partial */

/* One factor (W or H) as the engine sees it. */
typedef struct nmfmu_factor {
  float* f;           /* fp32 master, [rows][rank] row-major contiguous: the nn.Parameter storage (nmf.py:216-237) */
  void* p1_hi;        /* bf16 row-major image  [rows_pad][r_pad]          (nmfmu_image_bytes)                     */
  void* p1_lo;        /* low plane, BF16X3 only (else NULL)                                                        */
  void* p2_hi;        /* bf16 transposed tiles [rows_pad/64][r_pad][64]                                            */
  void* p2_lo;
  float* colsum;      /* [r_pad]  sum over rows of f: the beta==1 denominators of nmf.py:122-131                   */
  float* colsum_part; /* nmfmu_colsum_part_bytes(): scratch for the deterministic two-stage column sum            */
  int32_t rows;
  int32_t rows_pad;   /* nmfmu_pad_rows(rows) */
} nmfmu_factor;

/* One MU half-step: everything `_double_backward_update` (nmf.py:52-92) needs. */
typedef struct nmfmu_step {
  const void* xp;      /* X in fragment order: owner.rows_pad x panel.rows_pad (nmfmu_pack_x)                      */
  nmfmu_factor owner;  /* the factor being updated */
  nmfmu_factor panel;  /* the factor held fixed    */
  float* slab_num;     /* [nsplit][owner.rows_pad][r_pad] partial numerators                                       */
  float* slab_den;     /* same, partial denominators (beta != 1; may be NULL for beta == 1)                        */
  int32_t rank;
  int32_t r_pad;       /* nmfmu_pad_rank(rank) */
  int32_t nsplit;      /* contraction-axis split (workgroups per owner block), nmfmu_choose_nsplit                 */
  int32_t precision;   /* NMFMU_PREC_*  */
  int32_t stage;       /* NMFMU_STAGE_* */
  int32_t block_rows;  /* owner rows per workgroup tile: nmfmu_block_rows(); xp must have been packed with it        */
  float beta;
  float gamma;         /* nmf.py:341-346 */
  float l1, l2;        /* nmf.py:348-349 */
  uint32_t* status;    /* NULL or one device word (ABI 4): bit 0 is OR-ed in when an update had to clamp a factor value
                          at 65504 for its fp16 image (NMFMU_PREC_F16) -- the fit has left the mode's range           */
  void* stamps;        /* NULL, or (ABI 9) a device buffer of >= 64 + 5 * workgroups uint64: the ping-pong and the
                          software-pipelined kernel record their clocks there -- workgroup 0, wave 0 (and wave 4 of the
                          ping-pong pair): shader cycles (s_memtime), the constant 100 MHz clock (s_memrealtime) and the tile
                          count at kernel entry / loop start / loop end / exit; every workgroup the 100 MHz clock at the same four
                          points and where it ran.  Nothing is stamped inside the tile loop.  bench.py derives cycles per tile,
                          the in-kernel clock and the matrix pipe's busy fraction from it (roofline.in_kernel); layout in
                          tools/pp_timeline.py                                                                          */
} nmfmu_step;

/* ---- static queries (host only, no device work) ------------------------------------------------------------ */
int nmfmu_abi_version(void);
/* Load-time guard for bindings other than the bundled Python host: pass the NMFMU_ABI_VERSION the binding was
 * COMPILED against; NMFMU_OK iff it is the library's, NMFMU_ERR_ARG otherwise.  Struct layouts are append-only, but the
 * MEANING of a field may tighten between versions -- e.g. since ABI 6 a split panel (panel.p1_* and panel.p2_* images of
 * different matrices) must say NMFMU_STAGE_DMA_SPLIT: with NMFMU_STAGE_DMA the single-plane kernels stage p1 only and
 * derive the second GEMM's operand from it, so an ABI-5 caller's split panel would give wrong numerators without any
 * error.  A binding that calls this once after dlopen cannot run into that silently. */
int nmfmu_abi_check(int compiled_against);
int nmfmu_pad_rows(int rows);             /* rows rounded up to a multiple of 256                                  */
int nmfmu_pad_rank(int rank);             /* 32 / 64 / 128 / 256, or NMFMU_ERR_UNSUPPORTED                         */
int nmfmu_beta_kind(float beta);          /* NMFMU_BETA_*                                                          */
int nmfmu_supported(int r_pad, int precision);
int nmfmu_block_rows(int r_pad, int precision, float beta); /* 128 or 256: owner rows per workgroup tile          */
int nmfmu_choose_nsplit(int owner_rows_pad, int panel_rows_pad, int block_rows, int num_cu);
/* which fused kernel a half-step of this (padded rank, precision, beta) runs on, and the split that fills the chip with ITS
 * workgroups per CU (the ping-pong and the software-pipelined kernel: one; the four-wave kernel: two where its registers allow) */
#define NMFMU_KERNEL_FUSED 0 /* nmfmu::fused_kernel, four waves, 128-row tiles (nmfmu_fused.h)                         */
#define NMFMU_KERNEL_PP 1    /* nmfmu::pp_kernel, eight waves in two half-phases, 256-row tiles (nmfmu_pp.h)            */
#define NMFMU_KERNEL_SP 2    /* nmfmu::sp_kernel / sp2_kernel, four waves, software-pipelined across tiles, 128-row tiles
                                (nmfmu_sp.h: beta == 1 at padded rank 256; nmfmu_sp2.h: beta != 1, 2 at padded rank 128; fp16) */
int nmfmu_kernel_family(int r_pad, int precision, float beta);
/* 1 when a half-step of this (padded rank, precision, beta) on 256-row tiles has the instance that NMFMU_STAGE_DMA_LDSTR selects */
int nmfmu_pp_lds_transpose_supported(int r_pad, int precision, float beta);
int nmfmu_choose_nsplit_for(int owner_rows_pad, int panel_rows_pad, int r_pad, int precision, float beta, int block_rows, int num_cu);
/* tile height for ONE half-step of this shape (128 where the owner axis alone fills the chip, else nmfmu_block_rows) */
int nmfmu_step_block_rows(int owner_rows_pad, int panel_rows_pad, int r_pad, int precision, float beta, int num_cu);
size_t nmfmu_xp_bytes(int owner_rows_pad, int panel_rows_pad, int precision);
size_t nmfmu_image_bytes(int rows_pad, int r_pad);            /* one plane of p1 or of p2                          */
size_t nmfmu_slab_bytes(int owner_rows_pad, int r_pad, int nsplit);
size_t nmfmu_colsum_part_bytes(int rows_pad, int r_pad);

/* ---- one-time packing ----------------------------------------------------------------------------------------
 * nmfmu_pack_x: V (fp32, rows x cols, row stride ld elements) -> fragment-order X.
 *   transpose = 0: owner axis = V rows  (X = V,   H half-step and the loss)
 *   transpose = 1: owner axis = V cols  (X = V^T, W half-step)
 * Also performs the target validation of nmf.py:329-336 in the same pass:
 *   flags[0] |= 1 if any element fails (v >= 0)   (negative or NaN)
 *   flags[1]  = min over elements of the fp32 bit pattern (caller presets 0x7f800000); == 0 iff V.min() == 0
 */
int nmfmu_pack_x(const float* v, int64_t ld, int rows, int cols, int transpose, int precision, int block_rows, void* xp,
                 int owner_rows_pad, int panel_rows_pad, uint32_t* flags, void* stream);

/* nmfmu_pack_factor: build the bf16 images and the column sums from the fp32 master (after the user or
 * load_state_dict changed W/H; the apply step keeps them current afterwards). */
int nmfmu_pack_factor(const nmfmu_factor* fac, int rank, int r_pad, int precision, void* stream);

/* nmfmu_pack_factor_scaled: images of f[row][r] * scale[r] (the master stays as it is; since ABI 6 fac->colsum is NOT
 * refreshed -- only the partial sums in colsum_part are written -- PLCA's EM reads none).  PLCA feeds the first GEMM of
 * the fused kernel with the Z-scaled panel and the second with the unscaled one (scale = ones). */
int nmfmu_pack_factor_scaled(const nmfmu_factor* fac, int rank, int r_pad, int precision, const float* scale,
                             void* stream);

/* ---- the MU half-step ----------------------------------------------------------------------------------------
 * nmfmu_mu_partial: reconstruct + both backward passes of nmf.py:376-378 / 389-391, fused:
 *   slab_num[s] = sum over the s-th contraction chunk of  Gn(X, owner panel^T) @ panel      (nmf.py:77)
 *   slab_den[s] = likewise with Gp                                                    (nmf.py:82, beta != 1)
 * st->stage: NMFMU_STAGE_DMA when panel.p1_* and panel.p2_* are the two images of ONE matrix (every NMF half-step; the
 * single-plane kernels then read p1 only), NMFMU_STAGE_DMA_SPLIT when they are images of different matrices (PLCA's
 * Z-scaled / unscaled pair; beta == 1, this entry only).  Passing a split panel with NMFMU_STAGE_DMA is not detectable
 * here and yields the numerators of p1's matrix -- see nmfmu_abi_check.
 */
int nmfmu_mu_partial(const nmfmu_step* st, void* stream);

/* nmfmu_den_partial: the positive term alone for a generic beta (not 0, 1, 2), WITHOUT a target:
 *   slab_num[s] = sum over the s-th contraction chunk of (owner panel^T + eps)^(beta-1) @ panel      (st->xp may be NULL)
 * This is the dense pass the reference makes for sparse targets (nmf.py:628-636).  nmfmu_loss likewise accepts
 * st->xp == NULL and then evaluates beta_div against an all-zero target, i.e. sum (S + eps)^beta / beta. */
int nmfmu_den_partial(const nmfmu_step* st, void* stream);

/* nmfmu_mu_step: one complete single-device half-step = nmfmu_mu_partial + nmfmu_mu_apply (st->stage as there; a split
 * panel is not meaningful for a complete MU half-step and NMFMU_STAGE_DMA_SPLIT is rejected).  When the contraction is
 * not split (nsplit == 1) and beta == 1 the apply runs inside the fused kernel's epilogue (no slab round trip).
 * kl_den: column sums of the panel (beta == 1), else ignored.  phase: 0 = everything, 1 = only the fused kernel,
 * 2 = only what follows it (lets a caller bracket the dominant kernel with events). */
int nmfmu_mu_step(const nmfmu_step* st, const float* kl_den, int phase, void* stream);

/* beta == 2 WITHOUT the reconstruction (round 4).  The reference's beta == 2 branch (nmf.py:61-63) puts no eps inside the
 * two grad_outputs, so the update's numerator is X @ panel exactly and its denominator owner @ (panel^T panel): one
 * streaming MFMA GEMM over X (4 N C R flops per iteration instead of 12 N C R, HBM-bound) plus a rank x rank Gram matrix.
 *   nmfmu_gram_panel : G = panel^T panel from the panel's transposed 16-bit image (MFMA, fp32 accumulate, deterministic
 *                      two-stage sum).  Outputs: gram [r_pad][r_pad] fp32 (zero in the padding); g_hi / g_lo 16-bit
 *                      images of row r scaled by 2^-e[r] (inside fp16's range), g_scale[r] = 2^e[r].  ws: nmfmu_gram_ws_bytes.
 *   nmfmu_xb_partial : numerator slabs only (st->slab_num; st->slab_den is not touched) -- for callers that reduce across
 *                      devices before the apply.
 *   nmfmu_xb_step    : the complete half-step; phase as in nmfmu_mu_step.  The denominator is one more small MFMA product
 *                      (owner fragments x Gram image rows) inside the same kernel.  Unsplit contraction and padded rank
 *                      <= 128: everything in one kernel (nmf.py:78-92 in its epilogue); otherwise st->nsplit numerator slabs
 *                      + ONE denominator slab in st->slab_den (owner_rows_pad x r_pad floats suffice) + the apply kernel.
 * Single-plane precisions only (NMFMU_PREC_BF16 / F16 / F16X; with F16X the fp32 target enters the GEMM as an fp16
 * hi + lo pair). */
int nmfmu_xb_supported(int r_pad, int precision, float beta);
size_t nmfmu_gram_ws_bytes(int r_pad);
int nmfmu_gram_panel(const nmfmu_factor* panel, int r_pad, int precision, void* ws, float* gram, void* g_hi, void* g_lo,
                     float* g_scale, void* stream);
int nmfmu_xb_partial(const nmfmu_step* st, void* stream);
int nmfmu_xb_step(const nmfmu_step* st, const void* g_hi, const void* g_lo, const float* g_scale, int phase, void* stream);

/* Column-sum bookkeeping (nmf.py:122-131's H.sum / W.sum, deterministic two-stage sums): the number of partial sums
 * [nparts][r_pad] a half-step (nmfmu_colsum_nparts) or nmfmu_pack_factor (nmfmu_pack_nparts) leaves in colsum_part, and
 * the second stage on its own. */
int nmfmu_colsum_nparts(const nmfmu_step* st);
int nmfmu_pack_nparts(int rows_pad);
int nmfmu_colsum_finalize(const nmfmu_factor* fac, int nparts, int r_pad, void* stream);

/* nmfmu_slab_reduce: num_out = sum_s slab_num[s] (and den_out likewise unless NULL).  Used by the column-sharded
 * multi-GPU path so that one all-reduce carries [owner.rows_pad x r_pad] floats. */
int nmfmu_slab_reduce(const nmfmu_step* st, float* num_out, float* den_out, void* stream);

/* nmfmu_mu_apply: nmf.py:78-92.  neg = relu(sum of `nslab` numerator slabs) + eps;
 *   beta == 1: pos = kl_den[r]  (closed form nmf.py:122-131, no relu/eps)   else pos = relu(sum den slabs) + eps;
 *   pos += l1; pos += l2 * f;  f *= (neg / pos) ** gamma;
 * then refreshes owner's bf16 images and column sums.  num/den = NULL means "use st->slab_* with st->nsplit slabs".
 */
int nmfmu_mu_apply(const nmfmu_step* st, const float* num, const float* den, int nslab, const float* kl_den,
                   void* stream);

/* nmfmu_trainer_apply: the update of trainer.BetaMu.step (trainer.py:93-112) for one parameter, fed by the same
 * partial sums as nmfmu_mu_apply (the closure's WH.backward(output_neg) / WH.backward(output_pos) of trainer.py:93-97
 * are exactly the numerator / denominator contractions of nmfmu_mu_partial):
 *   neg = relu(sum num slabs);  pos = relu(sum den slabs)   [beta == 1: pos = kl_den[r], the ones-backward]
 *   grad = pos - neg                                          (p.grad of trainer.py:98; grad may be NULL)
 *   pos += l1;  pos += l2 * f;  pos += ortho * (sum_r f[row][r] - f);  pos += eps;  neg += eps
 *   f *= (neg / pos) ** gamma
 * l1 / l2 / gamma come from *st.  Refreshes owner's bf16 images and column sums like nmfmu_mu_apply. */
int nmfmu_trainer_apply(const nmfmu_step* st, const float* num, const float* den, int nslab, const float* kl_den,
                        float ortho, float* grad, void* stream);

/* ARD-NMF (Tan & Fevotte 2013; torchnmf_amd/ard.py, NMF.fit_ard): column k of W and column k of H share a scale lambda_k,
 * the update's denominator carries the PER-COMPONENT penalty pen[k] = phi / lambda_k, and lambda follows the factors.
 * nmfmu_ard_apply: nmfmu_mu_apply(st, NULL, NULL, 0, kl_den) -- st->slab_* with st->nsplit slabs, the same sums in the same
 * order, the same images, column sums and status bit -- with pen[st->r_pad] (device) in place of st->l1 / st->l2:
 *   prior NMFMU_ARD_L1 (exponential prior, f(x) = sum x):      pos += pen[r];
 *   prior NMFMU_ARD_L2 (half-normal prior, f(x) = 1/2 sum x^2): pos += pen[r] * f;       f *= (neg / pos) ** st->gamma
 * A pen entry of 0 leaves the bits of the unpenalised update; with pen == p everywhere the result is nmfmu_mu_apply's with
 * st->l1 = p (st->l2 = p), bit for bit.  Also leaves norm[r] = f(owner[:, r]) for r < r_pad (0 in the padding), a
 * deterministic two-stage sum: 'l1' it is the column sum (norm_part is not touched and may be NULL), 'l2' the per-stripe
 * partials go to norm_part (nmfmu_colsum_part_bytes floats' worth, like colsum_part).
 * nmfmu_ard_relevance: one small launch after the two half-steps.  For k < rank:
 *   lambda = ((norm_w[k] + norm_h[k]) + b) / c;  pen[k] = phi / lambda;  delta[0] = max_k |lambda - lam[k]| / lam[k];  lam[k] = lambda
 * and lam[k] = pen[k] = 0 for rank <= k < r_pad.  b, c, phi > 0; all pointers device memory. */
#define NMFMU_ARD_L1 1
#define NMFMU_ARD_L2 2
int nmfmu_ard_apply(const nmfmu_step* st, const float* kl_den, const float* pen, int prior, float* norm_part, float* norm,
                    void* stream);
int nmfmu_ard_relevance(const float* norm_w, const float* norm_h, int rank, int r_pad, float b, float c, float phi, float* lam,
                        float* pen, float* delta, void* stream);

/* trainer.BetaMu on a CHAIN of NMF layers (nn.Sequential, tests/test_trainer.py:10-32): the matrix products of the
 * forward / backward passes are nmfmu_reconstruct calls; these are the two pieces in between.
 *   nmfmu_mu_terms      : gn, gp = the seeds of trainer.py:75-91 from the prediction s and the target v (n elements;
 *                         beta == 1 gives gp = 1)
 *   nmfmu_trainer_update: trainer.py:93-112 on a plain row-major parameter f[rows][cols] with neg / pos of the same shape
 *                         (grad may be NULL) */
int nmfmu_mu_terms(const float* s, const float* v, int64_t n, float beta, float* gn, float* gp, void* stream);
int nmfmu_trainer_update(float* f, int rows, int cols, const float* neg, const float* pos, float l1, float l2, float ortho,
                         float gamma, float* grad, void* stream);

/* ---- loss -----------------------------------------------------------------------------------------------------
 * nmfmu_loss: beta_div(owner panel^T, X) of metrics.py:60-96 without materialising the reconstruction
 * (replaces nmf.py:360-361 and 400-401).  loss_part: nmfmu_loss_part_count() floats of scratch; *out (device
 * double) receives the divergence (NOT yet sqrt(2 x)).  rows/cols are the logical sizes of X.
 */
int nmfmu_loss_part_count(int owner_rows_pad, int block_rows, int nsplit);
int nmfmu_loss(const nmfmu_step* st, float* loss_part, double* out, void* stream);
/* (ABI 9) nmfmu_loss + everything else a loss checkpoint of the fit loop needs, in two launches: out2[0] = the same value
 * nmfmu_loss writes (same kernels, same summation order), out2[1] = 1.0 when bit 0 of st->status is set (a factor left fp16's
 * range; 0.0 without a status word), and the two factors' fp32 masters fa / fb (na / nb floats, multiples of 4, 16-byte
 * aligned) copied into fa_snap / fb_snap -- the snapshot a deferred stop decision rolls back to (nmf.py:393-407 judged one
 * checkpoint late). */
/* (ABI 9) "riding loss": the periodic KL loss of the fit loop (nmf.py:400-401) WITHOUT its own pass over the target.
 * metrics.py:22 is  target @ (log(target + eps) - log(input + eps)) - target.sum() + input.sum():
 *   nmfmu_target_sums        once per fit: out4 = { sum x ln(x + eps), sum x, max x, 1.0 if any x != fp16(x) else 0.0 } of the fp32
 *                            target in ONE pass (part: 4 * nmfmu_target_sums_nparts() doubles of scratch); the last two are what a
 *                            host needs to admit the fp16 modes (nmfmu_mu_step_with_loss reads the first two)
 *   nmfmu_mu_step_with_loss  the half-step that FOLLOWS a checkpoint (= nmfmu_mu_step(st, kl_den, 0, ..)), its kernel also
 *                            accumulating sum x log2(s) and sum s over its elements -- s = owner panel^T + eps is the reconstruction
 *                            of the factors before the update, i.e. the input the reference evaluates, from the same operand
 *                            images nmfmu_loss reads -- into xlogs_part (nmfmu_riding_loss_part_count() floats), then
 *                            out2 = { loss, fp16-range flag } (device doubles, as nmfmu_loss_checkpoint).  The caller snapshots
 *                            the factors at the checkpoint itself (they are the ones this loss belongs to)
 * nmfmu_riding_loss_supported: beta == 1 on the ping-pong kernel, fp16 operands (NMFMU_PREC_F16 / F16R), the buffers of
 * nmfmu_mu_step present.  Three VALU instructions per element on the half-steps that carry it. */
int nmfmu_riding_loss_supported(const nmfmu_step* st);
int nmfmu_riding_loss_part_count(const nmfmu_step* st);
int nmfmu_target_sums_nparts(void);
int nmfmu_target_sums(const float* v, int64_t ld, int rows, int cols, double* part, double* out4, void* stream);
int nmfmu_mu_step_with_loss(const nmfmu_step* st, const float* kl_den, float* xlogs_part, const double* target_sums,
                            double* out2, void* stream);
int nmfmu_loss_checkpoint(const nmfmu_step* st, float* loss_part, double* out2, const float* fa, float* fa_snap, int64_t na,
                          const float* fb, float* fb_snap, int64_t nb, void* stream);

/* nmfmu_beta_div: metrics.beta_div(x, y, beta) on two plain fp32 device arrays of n elements.
 * part: 1024 doubles of scratch. */
int nmfmu_beta_div(const float* x, const float* y, int64_t n, float beta, double* part, double* out, void* stream);

/* nmfmu_norms: out[0] = sum |x|, out[1] = sum x^2 over n fp32 elements (metrics.sparseness, metrics.py:99-115).
 * part: 1024 doubles of scratch. */
int nmfmu_norms(const float* x, int64_t n, double* part, double* out, void* stream);

/* nmfmu_reconstruct: out[m][k] = sum_r owner[m][r] panel[k][r]  (NMF.reconstruct, nmf.py:691-693) computed from the
 * fp32 masters with fp32 MFMA; out is row-major [owner.rows][panel.rows], ld elements per row. */
int nmfmu_reconstruct(const float* owner, int m, const float* panel, int k, int rank, float* out, int64_t ld,
                      void* stream);

/* nmfmu_reconstruct_backward: the two gradients of out = owner panel^T given g = d loss / d out (m x k fp32, ld >= k
 * elements per row, read in place -- no transposed copy is made):
 *   grad_owner[m][r] = sum_k g[m][k] panel[k][r]          grad_panel[k][r] = sum_m g[m][k] owner[m][r]
 * Exact-fp32 MFMA like nmfmu_reconstruct; any m, k, rank >= 1.  Either output may be NULL and is then not computed (the
 * factor it multiplies may be NULL with it).  Each half cuts its contraction into parts, one workgroup per (128 x 128 output
 * tile, part); with more than one part the partial products go to slabs in ws and are summed in part order by a second
 * kernel -- no floating-point atomics, results are bit-identical run to run.  Two launches of the product kernel when both
 * outputs are wanted: g is read twice.
 * Split rule (a pure function of the shape; rows / contraction = m / k for grad_owner, k / m for grad_panel):
 *   tiles = ceil(rows / 128) * ceil(rank / 128);  stages = ceil(contraction / 32)
 *   n     = max(1, min(ceil(512 / tiles), stages / 4, 64));  parts = ceil(stages / ceil(stages / n))
 *   every part is ceil(stages / parts) * 32 contraction steps long, the last one possibly shorter.
 * nmfmu_reconstruct_backward_ws returns the floats of scratch `ws` must hold for these outputs (0: ws may be NULL) and, when
 * splits is not NULL, writes splits[0] = parts of grad_owner, splits[1] = parts of grad_panel (0 for a half not wanted). */
int64_t nmfmu_reconstruct_backward_ws(int m, int k, int rank, int want_owner, int want_panel, int* splits);
int nmfmu_reconstruct_backward(const float* g, int64_t ld, int m, int k, const float* owner, const float* panel, int rank,
                               float* grad_owner, float* grad_panel, float* ws, void* stream);

/* nmfmu_beta_div_grad: gx[i] = upstream[0] * d nmfmu_beta_div(x, y) / d x[i] over n fp32 elements; upstream is the 0-dim
 * incoming gradient ON THE DEVICE (no host read).  eps as in metrics.py:6-96:
 *   beta == 2: x - y     beta == 1: 1 - y / (x + eps)     beta == 0: 1 / (x + eps) - (y + eps) / (x + eps)^2
 *   otherwise: (x + eps)^(beta - 1) - y' (x + eps)^(beta - 2), y' = y + eps for beta < 0 only.  y is a constant. */
int nmfmu_beta_div_grad(const float* x, const float* y, int64_t n, float beta, const float* upstream, float* gx,
                        void* stream);

/* nmfmu_conv_backward: the two gradients of the convolutive reconstruction (NMFD / NMF2D / NMF3D.reconstruct, nmf.py:776-779 /
 * 857-860 / 937-940: F.convNd(H, W.flip(..), padding = T - 1)) given g = d loss / d out.  ndim = 1..3 shift axes, lh / taps hold
 * ndim entries (outermost axis first), l_a = lh_a + taps_a - 1.  All tensors fp32, contiguous:
 *   g (batch, channels, *l)     w (channels, rank, *taps)     h (batch, rank, *lh)
 *   grad_h[b][r][j] = sum_c sum_t w[c][r][t] g[b][c][j + t]          grad_w[c][r][t] = sum_b sum_j g[b][c][j + t] h[b][r][j]
 * written straight into the layouts of h and w.  Exact-fp32 MFMA like nmfmu_reconstruct_backward.  No unfolded operand is built:
 * with goff(x) = (x_0 l_1 + x_1) l_2 + x_2 the element g[b][c][j + t] lies at (b channels + c) prod(l) + goff(j) + goff(t), and
 * the kernel fetches it with that index while staging to LDS.  Either output may be NULL and is then not computed (the factor
 * it multiplies -- w for grad_h, h for grad_w -- may be NULL with it); the other output is bit-equal to the both-outputs call.
 * Each half cuts its contraction into parts by the split rule of nmfmu_reconstruct_backward with
 *   grad_h: rows = batch prod(lh), contraction = channels prod(taps)      grad_w: rows = channels prod(taps), contraction = batch prod(lh)
 * (the rank tile is 32 wide for rank <= 32 and 128 wide above, so ceil(rank / 128) counts its tiles too), one workgroup per
 * (128 rows, rank tile, part); with more than one part the partial products go to slabs [parts][output] in ws -- grad_h's
 * first -- and are summed in part order: no floating-point atomics, bit-identical run to run.  batch prod(lh) and
 * channels prod(taps) must not exceed 2^30 (NMFMU_ERR_ARG).
 * nmfmu_conv_backward_ws (host only) returns the floats `ws` must hold (0: ws may be NULL) and, when splits is not NULL, writes
 * splits[0] = parts of grad_h, splits[1] = parts of grad_w (0 for a half not wanted). */
int64_t nmfmu_conv_backward_ws(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, int want_h,
                               int want_w, int* splits);
int nmfmu_conv_backward(const float* g, const float* w, const float* h, int batch, int channels, int rank, int ndim,
                        const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* ws, void* stream);

/* nmfmu_plca_backward / nmfmu_conv_plca_backward: the three gradients of the PLCA reconstructions (plca.py:371-373, 447-449,
 * 522-525, 602-605) given g = d loss / d out:
 *   dense   out[m][k] = sum_r h[m][r] z[r] w[k][r]                         g, ld, m, k, rank as nmfmu_reconstruct_backward
 *   conv    out = convNd(h, (w z).flip(..), padding = taps - 1)            g, w, h, batch .. taps as nmfmu_conv_backward
 * z (rank floats) indexes the rank axis, which no product contracts, so with the UNSCALED products
 *   rawH = g w  resp.  sum_c sum_t w[c][r][t] g[b][c][j + t]              rawW = g^T h  resp.  sum_b sum_j g[b][c][j + t] h[b][r][j]
 * (exactly what nmfmu_reconstruct_backward / nmfmu_conv_backward compute, by the same kernels, split rule and part order)
 *   grad_h[..][r][..] = z[r] rawH[..][r][..]        grad_w[c][r][..] = z[r] rawW[c][r][..]
 *   grad_z[r] = sum rawW[c][r][t] w[c][r][t]  ( = sum rawH[b][r][j] h[b][r][j] )
 * No w z temporary is built.  g, h, w, z must all be given; any of grad_h / grad_w / grad_z may be NULL (not all three).
 * Half selection.  The H half (rawH) is launched iff grad_h is wanted.  grad_z comes from the H half iff grad_h is wanted and
 * grad_w is not; otherwise from the W half.  The W half (rawW) is launched iff grad_w is wanted, or grad_z is wanted and grad_h
 * is not (then, with grad_w NULL, its raw product lives in ws only).
 * Finishing kernel.  Each launched half is finished in ONE pass over its output seen as [outer][rank][inner] (dense: outer = m
 * resp. k, inner = 1; conv: outer = batch resp. channels, inner = prod(lh) resp. prod(taps)): it adds the half's parts in part
 * order (in place of the slab-sum pass of the two entries above; with one part it runs in place over the product's output),
 * multiplies by z[r], stores the gradient if wanted, and, for the half grad_z comes from, accumulates sum raw F per rank against
 * the factor F of the output's layout.  Workgroup rule (a pure function of outer, rank, inner):
 *   want  = min(2048, ceil(outer rank inner / 8192))
 *   chunk = ceil(outer / min(want, outer));  nbo = ceil(outer / chunk)                     outer indices per workgroup
 *   inner == 1: nseg = 1;  else ns = max(1, min(ceil(want / nbo), floor(inner / 1024))),
 *               seg = ceil(inner / ns) rounded up to a multiple of 4,  nseg = ceil(inner / seg)   inner positions per workgroup
 *   blocks = nbo nseg; workgroup (x, y) owns outer [x chunk, (x + 1) chunk) and inner [y seg, (y + 1) seg), block index y nbo + x.
 * Every thread owns fixed ranks and a fixed sequence of elements; one thread per rank adds the workgroup's thread sums in
 * thread order; the [blocks][rank] partials in ws are added in block order by a second small kernel.  No floating-point
 * atomics, no fences: bit-identical run to run.  16-byte accesses where rows / lines are 16-byte aligned (rank resp. inner a
 * multiple of 4, aligned pointers), scalar otherwise.
 * ws (floats):  [H half: parts_h outer rank inner, if parts_h > 1]  [W half: parts_w outer rank inner, if parts_w > 1 or grad_w
 * is NULL]  [blocks rank of the half grad_z comes from, if grad_z is wanted]; the first two regions are rounded up to a multiple
 * of 4 floats each, so that every region of a 16-byte aligned ws is 16-byte aligned.
 * The _ws functions (host only) return the floats ws must hold (0: ws may be NULL) or NMFMU_ERR_ARG, and, when info is not NULL,
 *   info[0] = parts of the H half, info[1] = parts of the W half (0: not launched), info[2] / info[3] = finishing workgroups
 *   of the H / W half (0: not launched), info[4] = the half grad_z comes from (0 none, 1 H, 2 W).
 * Argument checks as the two entries above: NULL inputs, non-positive sizes, ld < k, flattened conv axes above 2^30, a missing
 * ws: NMFMU_ERR_ARG, before any device work. */
int64_t nmfmu_plca_backward_ws(int m, int k, int rank, int want_h, int want_w, int want_z, int* info);
int nmfmu_plca_backward(const float* g, int64_t ld, int m, int k, const float* h, const float* w, const float* z, int rank,
                        float* grad_h, float* grad_w, float* grad_z, float* ws, void* stream);
int64_t nmfmu_conv_plca_backward_ws(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                                    int want_h, int want_w, int want_z, int* info);
int nmfmu_conv_plca_backward(const float* g, const float* w, const float* h, const float* z, int batch, int channels, int rank,
                             int ndim, const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* grad_z,
                             float* ws, void* stream);

/* nmfmu_hoyer_project: Hoyer's projection onto {v >= 0, sum v = k1, sum v^2 = k2} (Hoyer 2004, section 3.3; the reference's
 * nmf.py:21-49) of every slice of a factor, in place, in ONE call with no host round trip.  x is a contiguous fp32 tensor seen
 * as [outer][J][inner]; slice j is every element with index j on the middle axis (n = outer * inner elements): dim = 1 of
 * W (C, R), H (N, R), W (C, R, *T), H (B, R, *L), or any dim of any contiguous tensor.  k1[j] / k2[j] are slice j's L1 and squared
 * L2 targets, device arrays of J floats.  Per slice:
 *   v = s + (k1 - sum s) / n;  zeroed = {}
 *   repeat:  m = k1 / (n - |zeroed|);  w_i = v_i - m for i not zeroed, w_i = v_i for i zeroed (sic, as the reference)
 *            alpha = (-b + sqrt(max(b^2 - 4 a c, 0))) / (2 a),  a = w.w, b = 2 w.v, c = v.v - k2;  v += alpha w
 *            no v_i < 0: stop (a NaN compares false and ends the loop too)
 *            zeroed |= {v_i < 0};  v = max(v, 0);  v += (k1 - sum v) / (n - |zeroed|) on EVERY coordinate (sic);  v = max(v, 0)
 * One workgroup of 256 threads owns a slice for its whole loop (grid = J workgroups; no atomics, no spin-waits).  Elementwise
 * arithmetic is fp32; the block-wide sums and the scalars derived from them are fp64.  The loop is capped at n passes:
 * status[j] (J ints on the device, may be NULL) = the number of passes made, negated when the cap ended the loop.  Degenerate
 * slices (n = 1, all zero, k2 = 0) return NaN like the reference.
 * Residency: n <= lds_max_elems (<= 0 or anything above the built maximum of 40896 means that maximum) keeps the slice in
 * LDS between its one strided read and its one strided write; a longer slice is streamed from a slice-major copy in `ws`,
 * built and written back by a tiled transpose (a tensor with outer == 1 or J == 1 is slice-major already and streamed in place).
 * nmfmu_hoyer_project_ws (host only) returns the BYTES `ws` must hold for these arguments (0: ws may be NULL) or an error
 * code.  n >= 2^31 or J < 1: NMFMU_ERR_UNSUPPORTED.  Nothing is allocated inside the library. */
int64_t nmfmu_hoyer_project_ws(int64_t outer, int J, int64_t inner, int lds_max_elems);
int nmfmu_hoyer_project(float* x, int64_t outer, int J, int64_t inner, const float* k1, const float* k2, int lds_max_elems,
                        void* ws, int* status, void* stream);

/* ---- convolutive NMF (NMFD, nmf.py:700-779) --------------------------------------------------------------------
 * NMFD is dense NMF on unfolded operands with effective rank R*T: with W (C,R,T) viewed as Wm (C x R*T) and
 * Hu[(b,l)][(r,t)] = H[b][r][l-t], the reconstruction F.conv1d(H, W.flip(2), padding=T-1) (nmf.py:776-779) is
 * Wm Hu^T and both conv-backward passes (nmf.py:77, 82) are GEMMs too.  The entry points below are the pieces
 * NMFD.fit is assembled from (torchnmf_amd/nmfd_engine.py shows the order).  All matrices are zero padded to
 * multiples of 128 in every dimension; bf16 operands are (hi[, lo]) planes with the contraction index contiguous.
 */
#define NMFMU_EPI_RATIO 0 /* D = A B^T (+eps); Gn = f(D, x) [and Gp, beta != 1] stored as bf16 planes (nmf.py:61-74)   */
#define NMFMU_EPI_F32 1   /* D stored as fp32                                                                         */
#define NMFMU_EPI_LOSS 2  /* beta_div(D, x) partial per workgroup into out[(m_pad/128) * (n_pad/128)] (metrics.py)    */
#define NMFMU_EPI_FOLD 3  /* D = Y[(r,t)][(b,l)] (H numerator before the col2im sum, nmf.py:77/82 conv backward wrt the
                             input) is not stored; out receives the diagonal sums of every 128 x 128 tile
                             (nmfmu_fold_part_bytes) for nmfmu_conv_fold_parts_apply_h.  Planes only; t_batch .. t_lh
                             describe H; needs taps >= 128 and Lh + taps - 1 >= 128 (nmfmu_fold_parts_supported)       */

typedef struct nmfmu_gemm_desc {
  const void* a_hi; /* [m_pad][k_pad] bf16 */
  const void* a_lo; /* BF16X3 only */
  const void* b_hi; /* [n_pad][k_pad] bf16 */
  const void* b_lo;
  int32_t m_pad, n_pad, k_pad;
  int32_t precision; /* NMFMU_PREC_* */
  float beta;
  const float* x;   /* [m_pad][n_pad] fp32 target (RATIO, LOSS) */
  void* gn_hi;      /* RATIO outputs, [m_pad][n_pad] bf16 */
  void* gn_lo;
  void* gp_hi;      /* beta != 1 */
  void* gp_lo;
  float* out;       /* F32: [m_pad][n_pad]; LOSS: partials */
  int32_t m_valid, n_valid; /* LOSS: logical extent */
  /* Implicit conv-unfold operands (nmfmu_conv_tables): instead of materialising the Toeplitz matrix
   * Hu[(b,l)][(r,t)] = H[b][r][l-t] (T times larger than H), an operand may be fetched chunk by chunk from a
   * window table that is only 8x H.  ops selects which operand is implicit; its hi / lo pointers then address the table. */
  int32_t ops;              /* NMFMU_OPS_* */
  int32_t t_batch, t_rank, t_taps, t_lh; /* B, R, T, Lh of H (implicit operands and NMFMU_EPI_FOLD) */
  /* Workgroup tile: 0 or 128 = 128 x 128.  (ABI 3 also had a 256 x 256 tile; without a stream-K scheduler it never
   * paid at the BASELINE shapes and is no longer built: NMFMU_ERR_UNSUPPORTED.) */
  int32_t tile_rows;
  /* Leading dimension of x / gn / gp / out when the GEMM covers only the first n_pad columns of wider matrices
   * (0 = n_pad).  Together with a reduced m_pad this lets a caller leave a few ragged rows / columns to
   * nmfmu_conv_ragged_rows instead of paying a whole 128-wide tile row for them. */
  int32_t n_ld;
  /* Contraction length actually run (0 = k_pad; a multiple of 64 covering the logical extent): the zero tail of
   * 128-padded planes need not be multiplied. */
  int32_t k_len;
  /* NMFMU_EPI_F32: k_split (> 1) workgroups share the contraction of every tile; partial z goes to
   * out + z * m_pad * n_ld (the consumer adds them).  For long-k GEMMs with too few tiles to fill the chip.
   * NMFMU_EPI_FOLD: with tail_rows > 0 the LAST tail_rows tile rows are contraction-split k_split ways (the tail-round
   * split: when the tile count is N full rounds of the chip plus a few tiles, those few cost a fraction of a round
   * instead of a whole one); partial z of their diagonal sums goes to out + z * nmfmu_fold_part_bytes() / 4 and
   * nmfmu_conv_fold_parts_apply_h_tail adds them in a fixed order. */
  int32_t k_split;
  int32_t tail_rows;   /* (ABI 4, appended) */
  /* (ABI 5, appended) Ragged channels inside the grid of a reconstruction GEMM (NMFMU_EPI_RATIO with ops B_HU or A_HU):
   * channels [rag_c0, rag_channels), at most 16 -- those beyond the GEMM's own m_pad (B_HU) resp. n_pad (A_HU) rows of
   * the explicit operand, whose planes must hold rows rag_c0 .. rag_c0 + 15 (zero beyond the logical extent) -- ride
   * along as one extra 16 x 16 x 32 MFMA block per workgroup, with the same elementwise epilogue into the same planes
   * (row / column rag_c0.. of x / gn / gp at pitch n_ld).  Replaces a separate nmfmu_conv_ragged_rows launch (modes
   * 0 / 1) when nmfmu_gemm_ragged_supported().  rag_channels == 0: off. */
  int32_t rag_c0, rag_channels;
  /* (ABI 7, appended) Window operand, ops == NMFMU_OPS_A_WIN with NMFMU_EPI_F32: the H numerator of the convolutive
   * models without the unfolded Y matrix.  A is never stored: A[(b,j)][(t,c)] = P[(b, j + t)][c], where P = a_hi / a_lo
   * are the row-major ratio planes of the H half-step ([t_batch * prod(l)][win_pitch] elements, l = lh + taps - 1 per
   * shift axis) -- tile row (b, j) of k-tile (t, 64 channels) is row (b, j + t) of P, so the operand fetch is the plain
   * plane fetch with a per-lane row map and a scalar tap offset.  B = [n_pad][k_pad] planes of W ordered
   * k = (t * ceil(win_channels / 64) + ck) * 64 + c' (nmfmu_conv_pack_wk); k_len = prod(taps) * ceil(win_channels / 64) * 64;
   * m_pad >= t_batch * prod(lh) rows (b, j), j flattened over the shift axes; n_pad a multiple of 32 (the padded rank);
   * the planes P must be smaller than 2 GiB each (32-bit lane offsets).
   * out[(b,j)][r] = sum_{c,t} P[(b, j + t)][c] W[c][r][t]   (conv backward wrt H, nmf.py:776-779 / 857-860 / 937-940). */
  int32_t win_nd;          /* shift axes, 1 .. 3 */
  int32_t win_lh[3];       /* H extent per axis (outermost first; the first win_nd entries) */
  int32_t win_taps[3];     /* taps per axis */
  int32_t win_channels;    /* C */
  int32_t win_pitch;       /* elements per row of P (multiple of 64, >= ceil(C / 64) * 64) */
  /* Fold F (0 / 1: none): with a rank of at most 32 / F the 32-wide N tile would multiply mostly padding; instead F
   * consecutive taps of the LAST axis, t = F q + d, share one k position and go to F columns:
   *   out[(b, jo, j')][r F + d] = sum_{c, to, q} P[(b, jo + to, j' + F q)][c] W[c][r][to][F q + d],   j' in [0, lh_last + F - 1)
   * (1 / F of the MFMA work and operand traffic); the consumer adds num[..][j] = sum_d out[(.., j + d)][r F + d]
   * (nmfmu_conv_apply_h_rows).  taps_last % F == 0, rank * F <= n_pad, m_pad >= batch * prod(lh_outer) * (lh_last + F - 1),
   * k_len = prod(taps) / F * ceil(C / 64) * 64, B from nmfmu_conv_pack_wk with the same F. */
  int32_t win_fold;
  /* (ABI 7) Implicit operands (ops B_HU / B_HUT / A_HU) of an H with SEVERAL shift axes (NMF2D / NMF3D): win_nd > 1,
   * win_lh / win_taps as above, the operand's hi / lo = the tables of nmfmu_convnd_tables, and t_koff = DEVICE copy of
   * nmfmu_convnd_koff(ops, ..., k_pad) -- one int per 8-wide k-chunk.  Needs taps and V extent of the LAST axis to be
   * multiples of 8.  NULL with win_nd <= 1: the one-axis form above (t_taps, t_lh). */
  const int32_t* t_koff;
  /* (ABI 8, appended) How an implicit operand (ops B_HU / B_HUT / A_HU, one shift axis) reaches LDS: 0 = automatic -- as a
   * sliding WINDOW of the distinct table entries a k-tile touches (128 + 56 entries = 2.9 KiB instead of the 16 KiB of a
   * chunk-major tile, which holds most entries eight times: 19 instead of 32 LDS-DMA pieces per k-tile) wherever the
   * implicit operand's tiles hold no padding (nmfmu_gemm_window_staged), chunk-major elsewhere; 1 = chunk-major always
   * (the form of ABI <= 7; same results bit for bit -- the products and their order are unchanged). */
  int32_t stage_mode;
} nmfmu_gemm_desc;

#define NMFMU_OPS_PLANES 0   /* A and B are bf16 planes                                                            */
#define NMFMU_OPS_B_HU 1     /* B = Hu : rows (b,l), k = (r,t)  -- reversed-window table  (W half-step reconstruction) */
#define NMFMU_OPS_B_HUT 2    /* B = HuT: rows (r,t), k = (b,l)  -- forward-window table   (W numerator)              */
#define NMFMU_OPS_A_HU 3     /* A = Hu                                                     (H half-step reconstruction) */
#define NMFMU_OPS_A_WIN 4    /* A = shifted rows of the ratio planes, B = W as [r][(t,c)]  (H numerator; see win_* below)  */

/* nmfmu_conv_tables: the two window tables of H (B, R, Lh) for T taps, bf16 (hi[, lo]):
 *   rev[1 + (b R + r) JJ + jj] = { H[b][r][j], H[b][r][j-1], ..., H[b][r][j-7] }     j = jj - (T-1)
 *   fwd[1 + (b R + r) JJ + jj] = { H[b][r][j], H[b][r][j+1], ..., H[b][r][j+7] }
 * with JJ = Lh + 2T - 2 (= L + T - 1), entries outside [0, Lh) zero, chunk 0 all zero.  Requires T % 8 == 0 and
 * (Lh + T - 1) % 8 == 0; nmfmu_conv_table_bytes() gives the size of ONE plane of ONE table. */
size_t nmfmu_conv_table_bytes(int batch, int rank, int lh, int taps);
int nmfmu_conv_tables(const float* h, int batch, int rank, int lh, int taps, void* rev_hi, void* rev_lo, void* fwd_hi,
                      void* fwd_lo, void* stream);

/* Window tables for several shift axes, H (batch, rank, lh[0..ndim-1]), taps[0..ndim-1] (outermost axis first).  Let
 * jj_d = lh_d + 2 taps_d - 2 and number the zero-padded lines of H (b, r, p_0, .., p_{n-2}), p_d in [0, jj_d), line
 * (.., p_d, ..) = H[b][r][p_0 - (taps_0 - 1)] .. (all zero when an index falls outside H).  The tables are the one-axis
 * tables of these lines along the last axis, concatenated:
 *   rev[1 + (((b R + r) jj_0 + p_0) .. ) jj_last + p] = { line[j], line[j-1], .., line[j-7] },  j = p - (taps_last - 1)
 *   fwd[...]                                          = { line[j], line[j+1], .., line[j+7] }
 * chunk 0 all zero.  The chunk a GEMM lane fetches is (term of its tile row) + koff[k-chunk]:
 *   rows (b, l), k = (r, t)  (B_HU, A_HU):  row term = b R JJ + sum_d (l_d + taps_d - 1) S_d,
 *                                           koff[kc] = 1 + r JJ - sum_d t_d S_d              (t = the chunk's first tap)
 *   rows (r, t), k = (b, l)  (B_HUT):       row term = r JJ + sum_d (taps_d - 1 - t_d) S_d,
 *                                           koff[kc] = 1 + b R JJ + sum_d l_d S_d
 * with S_last = 1, S_d = S_{d+1} jj_{d+1}, JJ = prod jj_d; koff = INT32_MIN for k-chunks in the padding of k.
 * nmfmu_convnd_koff is host code and fills k_pad / 8 + 8 ints (the last 8 are spare: the kernel reads one k-tile ahead);
 * the caller copies the array to the device. */
size_t nmfmu_convnd_table_bytes(int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps);
int nmfmu_convnd_tables(const float* h, int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps, int precision,
                        void* rev_hi, void* rev_lo, void* fwd_hi, void* fwd_lo, void* stream);   /* BF16 | BF16X3 (lo planes) | F16 */
int nmfmu_convnd_koff(int ops, int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps, int k_pad,
                      int32_t* koff_host);

int nmfmu_gemm(const nmfmu_gemm_desc* d, int epilogue, void* stream);
/* 1 when nmfmu_gemm(d, epilogue) stages its implicit operand as a window of table entries (stage_mode 0 and a shape whose
 * implicit operand has no padding inside any tile: rows (b,l): (Lh + T - 1) % 128 == 0, T >= 64, n_pad resp. m_pad ==
 * batch * (Lh + T - 1), k_len == rank * T (a multiple of 64); rows (r,t): n_pad == rank * T (a multiple of 128), T >= 128,
 * (Lh + T - 1) % 64 == 0, k_len == batch * (Lh + T - 1)); 0 otherwise; < 0: the descriptor is invalid. */
int nmfmu_gemm_window_staged(const nmfmu_gemm_desc* d, int epilogue);
/* NMFMU_PREC_F16 in the GEMM engine: fp16 operand planes / window tables (nmfmu_conv_tables_f16,
 * nmfmu_conv_apply_pack_w_sums with precision F16) and fp16 ratio planes, one plane each, same MFMA rate as bf16 with
 * 11 significant bits; ratios saturate at 65504.  Built for the combinations of the beta == 1 NMFD iteration on implicit
 * operands: RATIO with B or A = Hu, LOSS with B = Hu, F32 with B = HuT, FOLD (else NMFMU_ERR_UNSUPPORTED). */
int nmfmu_gemm_f16_supported(float beta, int epilogue, int ops);
int nmfmu_conv_tables_f16(const float* h, int batch, int rank, int lh, int taps, void* rev, void* fwd, void* stream);

/* Ragged channels of the NMFD reconstruction (RATIO / LOSS epilogues with A or B = Wm): channels c0 .. channels-1 by
 * direct summation S[c][(b,l)] = sum_{r,t} w[c][r][t] h[b][r][l-t] from the fp32 masters, so that the GEMM only has to
 * cover the first c0 = floor(channels / 128) * 128 of them (m_pad resp. n_pad = c0, n_ld = the planes' width): a
 * spectrogram with 2^k + 1 bins otherwise pays a whole 128-row tile row for one channel.
 *   mode 0: ratio planes gn (gp) [c][ld]   (W half-step)      mode 1: [(b,l)][ld]   (H half-step)
 *   mode 2: beta_div partials, loss_part[nmfmu_conv_ragged_blocks() * (channels - c0)]
 * x has the layout of the outputs.  BF16 / BF16X3 / F16. */
int nmfmu_conv_ragged_supported(int rank, int taps);
int nmfmu_conv_ragged_blocks(int batch, int lh, int taps);
/* 1 if nmfmu_gemm can take `extra` (1..16) ragged channels into its own grid (nmfmu_gemm_desc.rag_*): eight workgroups
 * share out the 128 frames of an implicit-operand tile, so the explicit operand needs >= 8 whole 128-row tiles. */
int nmfmu_gemm_ragged_supported(int ops, int m_pad, int n_pad, int extra);
int nmfmu_conv_ragged_rows(const float* w, int channels, int rank, int taps, const float* h, int batch, int lh, int c0,
                           int precision, float beta, int mode, const float* x, int64_t ld, void* gn_hi, void* gn_lo,
                           void* gp_hi, void* gp_lo, float* loss_part, void* stream);

/* Strided 2-D gather of an fp32 tensor into a zero-padded row-major matrix (fp32 copy and/or bf16 hi[,lo] planes):
 *   dst[row][col] = src[(row / row_inner) * row_outer_stride + (row % row_inner) * row_inner_stride
 *                     + (col / col_inner) * col_outer_stride + (col % col_inner) * col_inner_stride]
 * Covers V (B,C,L) -> [c][(b,l)] and [(b,l)][c], and W (C,R*T) -> Wm / Wm^T.  Optional validation flags as in
 * nmfmu_pack_x (nmf.py:329-336). */
int nmfmu_pack2d(const float* src, int rows, int cols, int row_inner, int64_t row_outer_stride, int64_t row_inner_stride,
                 int col_inner, int64_t col_outer_stride, int64_t col_inner_stride, int rows_pad, int cols_pad,
                 float* dst_f32, void* dst_hi, void* dst_lo, uint32_t* flags, void* stream);

/* Toeplitz unfold of H (batch, rank, lh): hu [(b,l)][(r,t)] (bl_pad x rp_pad) and hut [(r,t)][(b,l)]. */
int nmfmu_conv_unfold(const float* h, int batch, int rank, int lh, int taps, void* hu_hi, void* hu_lo, void* hut_hi,
                      void* hut_lo, int bl_pad, int rp_pad, void* stream);

/* out[r] = sum over outer o and inner i of src[o][r][i]: the closed-form beta == 1 denominators (nmf.py:122-131).
 * part: rank * 128 floats of scratch (deterministic two-stage sum). */
int nmfmu_rank_sums(const float* src, int outer, int rank, int inner, float* part, float* out, void* stream);

/* nmf.py:78-92 for W (channels, rank, taps) in place; num/den fp32 [c_pad][rp_pad]; kl_den[rank] or den.
 * (This entry and nmfmu_conv_apply_pack_w below are the un-fused forms: kept for bindings written against earlier ABI
 * versions; the Python host calls nmfmu_conv_apply_pack_w_sums, whose optional operands make it a superset.) */
int nmfmu_conv_apply_w(float* w, int channels, int rank, int taps, const float* num, const float* den,
                       const float* kl_den, int rp_pad, float l1, float l2, float gamma, void* stream);

/* nmfmu_conv_apply_w (when update != 0) fused with the re-packing of W into both GEMM operand layouts:
 * Wm [c_pad][rp_pad] and WmT [rp_pad][c_pad] bf16 planes (hi[, lo]; padding zero).  update == 0 only packs.
 * PRECONDITION of update != 0: the same plane buffers (and tile-sum buffer, in the _sums form) have been through ONE
 * update == 0 call before -- channel tiles that are padding only are skipped by the update pass and rely on the zeros
 * the pack-only pass wrote there. */
int nmfmu_conv_apply_pack_w(float* w, int channels, int rank, int taps, const float* num, const float* den,
                            const float* kl_den, int c_pad, int rp_pad, float l1, float l2, float gamma, int update,
                            void* wm_hi, void* wm_lo, void* wmt_hi, void* wmt_lo, void* stream);

/* Folds y[(r,t)][(b,l)] (fp32 [rp_pad][bl_pad]) along the taps, neg[b][r][j] = sum_t y[(r,t)][(b,j+t)], then
 * nmf.py:78-92 for H (batch, rank, lh) in place. */
int nmfmu_conv_fold_apply_h(float* h, int batch, int rank, int lh, int taps, const float* y_num, const float* y_den,
                            const float* kl_den, int bl_pad, float l1, float l2, float gamma, void* stream);
/* The same update from the per-tile diagonal sums of NMFMU_EPI_FOLD GEMMs (p_num / p_den) instead of Y: saves writing
 * and re-reading 4 * R*T * B*L bytes per GEMM.  Deterministic (fixed gather order). */
/* The same two kernels with the beta == 1 denominators (nmf.py:122-131) fused in instead of nmfmu_rank_sums launches:
 *   nmfmu_conv_apply_pack_w_sums     takes num as num_slabs split-K partials [slab][c_pad][rp_pad] (nmfmu_gemm_desc.k_split),
 *                                    sum_{b,j} H[b][r][j] as kl_den (finished) or as kl_hpart[rank][n_hparts]
 *                                    partials, and leaves wcol[c_pad/64][rp_pad/64][2] = sums of W per 64 x 64 tile and
 *                                    rank (taps >= 64: at most two ranks per tile);
 *   nmfmu_conv_fold_parts_apply_h_sums takes sum_{c,t} W[c][r][t] as kl_den or as kl_wcol (c_tiles = c_pad / 64) and
 *                                    leaves hsum_part[rank][nmfmu_fold_hsum_parts(batch, lh)] partial sums of the new H. */
int nmfmu_conv_apply_pack_w_sums(float* w, int channels, int rank, int taps, const float* num, const float* den,
                                 const float* kl_den, const float* kl_hpart, int n_hparts, float* wcol, int num_slabs,
                                 int c_pad, int rp_pad, float l1, float l2, float gamma, int update, int precision,
                                 void* wm_hi, void* wm_lo, void* wmt_hi, void* wmt_lo, void* stream);
int nmfmu_fold_hsum_parts(int batch, int lh);
int nmfmu_conv_fold_parts_apply_h_sums(float* h, int batch, int rank, int lh, int taps, const float* p_num,
                                       const float* p_den, const float* kl_den, const float* kl_wcol, int c_tiles,
                                       int rp_pad, float* hsum_part, int bl_pad, float l1, float l2, float gamma,
                                       void* stream);
/* ... and for an EPI_FOLD GEMM that ran with the tail-round split (nmfmu_gemm_desc.tail_rows / k_split; m_pad = the GEMM's):
 * the superset of the two entries above (kl_wcol / hsum_part may be NULL). */
int nmfmu_conv_fold_parts_apply_h_tail(float* h, int batch, int rank, int lh, int taps, const float* p_num,
                                       const float* p_den, const float* kl_den, const float* kl_wcol, int c_tiles,
                                       int rp_pad, float* hsum_part, int bl_pad, float l1, float l2, float gamma, int m_pad,
                                       int tail_rows, int k_split, void* stream);
/* ... and rewriting the window tables of the new H in the same launch (ABI 5; replaces the nmfmu_conv_tables call that
 * would follow).  A table entry spans eight consecutive j, so blocks recompute a halo of their neighbours' elements and
 * need the OLD values while the neighbours overwrite theirs: h_old is a copy of h that this launch only reads, h_next a
 * second buffer that receives the new values beside h itself; the caller swaps the two every iteration (and refreshes
 * h_old from h whenever h was changed by anything else).  The tables must have been built by nmfmu_conv_tables[_f16]
 * once: entries whose windows lie outside [0, lh) are never touched.  hsum_part holds
 * nmfmu_fold_hsum_parts_tables(batch, lh) partial sums per rank.  rev_lo / fwd_lo: NMFMU_PREC_BF16X3 only. */
int nmfmu_fold_hsum_parts_tables(int batch, int lh);
int nmfmu_conv_fold_parts_apply_h_tables(float* h, const float* h_old, float* h_next, int batch, int rank, int lh, int taps,
                                         const float* p_num, const float* p_den, const float* kl_den, const float* kl_wcol,
                                         int c_tiles, int rp_pad, float* hsum_part, int bl_pad, float l1, float l2,
                                         float gamma, int m_pad, int tail_rows, int k_split, int precision, void* rev_hi,
                                         void* rev_lo, void* fwd_hi, void* fwd_lo, void* stream);
size_t nmfmu_fold_part_bytes(int m_pad, int n_pad);
int nmfmu_fold_parts_supported(int batch, int rank, int lh, int taps);
int nmfmu_conv_fold_parts_apply_h(float* h, int batch, int rank, int lh, int taps, const float* p_num, const float* p_den,
                                  const float* kl_den, int bl_pad, float l1, float l2, float gamma, void* stream);

/* NMF2D / NMF3D (nmf.py:782-942): the same two steps with ndim = 2 or 3 shift axes (lh[ndim], taps[ndim] outermost
 * first; ndim = 1 is NMFD).  Flattened, (b,l) has batch * prod(lh + taps - 1) rows and (r,t) rank * prod(taps) columns;
 * everything else of the NMFD sequence (pack2d, gemm, rank_sums, conv_apply_w with taps = prod(taps)) is shared. */
int nmfmu_convnd_unfold(const float* h, int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                        void* hu_hi, void* hu_lo, void* hut_hi, void* hut_lo, int bl_pad, int rp_pad, void* stream);
int nmfmu_convnd_fold_apply_h(float* h, int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                              const float* y_num, const float* y_den, const float* kl_den, int bl_pad, float l1,
                              float l2, float gamma, void* stream);

/* ---- sparse-COO targets (nmf.py:351-398, 602-638), beta in {1, 2} ---------------------------------------------
 * V is handed over as CSR over the owner axis of the half-step: rowptr[owner_rows + 1], colidx / vals[nnz] (int32
 * indices; rows of V for the H half-step, rows of V^T for the W half-step).  Factors are the plain fp32 masters.
 *   nmfmu_sp_partial : num[row][:] = sum over the row's entries of g(v, <owner[row], panel[col]>) * panel[col][:]
 *                      (g = v / (s + eps) for beta 1, v for beta 2), num is [owner_rows][r_pad], later passed to
 *                      nmfmu_mu_apply as a single slab together with kl_den (beta 1) or den (beta 2)
 *   nmfmu_gram       : gram = f^T f (rank x rank);  nmfmu_rowmat : den[row][:] = owner[row] @ gram  (beta 2)
 *   nmfmu_sp_loss_neg: *out = sum_nnz v log(s + eps) (beta 1) or v s (beta 2), the data-dependent term of the loss
 *                      the reference tracks on sparse targets; part: (owner_rows + 3) / 4 doubles of scratch
 * Other beta: NMFMU_ERR_UNSUPPORTED (their positive term is a dense N x C pass in the reference too). */
int nmfmu_sp_partial(const int32_t* rowptr, const int32_t* colidx, const float* vals, int owner_rows, const float* owner,
                     const float* panel, int rank, float beta, float* num, int r_pad, void* stream);
int nmfmu_sp_loss_neg(const int32_t* rowptr, const int32_t* colidx, const float* vals, int owner_rows, const float* owner,
                      const float* panel, int rank, float beta, double* part, double* out, void* stream);
size_t nmfmu_gram_part_bytes(int rank);   /* scratch of nmfmu_gram */
int nmfmu_gram(const float* f, int rows, int rank, float* part, float* gram, void* stream);
int nmfmu_rowmat(const float* owner, int rows, int rank, const float* gram, float* den, int r_pad, void* stream);

/* ---- autograd on sparse-COO targets: V_norm + pos - neg and its factor gradients, beta in {1, 2} (additive entries) --------
 * Built on SEGMENTS, not whole owner rows: the host cuts every CSR row (H side, forward) and every CSC column (W side) into
 * runs of at most `chunk` stored entries and one wave takes one run, so a few rows with thousands of entries do not set
 * the run time.
 *   seg   int32 [n_seg][4] = (owner row, p_begin, p_end, slot), in row order.  slot < 0: the row's only segment (a row without
 *         entries has one empty segment: every owner row belongs to exactly one writer).  slot >= 0: the row is split; the
 *         segment's partial row is stored to ws[slot][r_pad]; the slots of a row are consecutive and in segment order
 *   multi int32 [n_multi][3] = (owner row, first slot, number of segments) of the split rows
 *   nmfmu_sp_div_backward_ws : floats of `ws` = (sum of `segments` over multi) * r_pad -- a pure function of the counts
 *   nmfmu_sp_div_forward     : *out = sum over the stored entries of v log(s + eps) (beta 1) | v s (beta 2),
 *                              s = <owner[row], panel[colidx[p]]>; accumulated in double per wave, per workgroup, then in
 *                              block order.  part: (n_seg + 3) / 4 doubles of scratch.  s_out (may be NULL): s[p] for
 *                              every stored entry, in the order of colidx (what the beta == 1 backward reads)
 *   nmfmu_sp_div_backward    : out[row][:] = up[0] * (pos - sum over the row's entries of g * panel[idx[p]][:]),
 *                              g = vals[p] / (s[q] + eps) (beta 1; q = perm ? perm[p] : p) | vals[p] (beta 2; s, perm unused).
 *                              One call per side: the H side takes the CSR list (perm NULL), the W side the CSC list with
 *                              vals in CSC order and perm[p] = the CSR position of CSC entry p.  pos: a vector [rank]
 *                              (pos_plane == 0; beta 1: the panel's column sums, nmfmu_rank_sums) or a plane [rows][r_pad]
 *                              (pos_plane != 0; beta 2: nmfmu_rowmat of the owner and the panel's Gram matrix).  up: the 0-dim
 *                              incoming gradient, read on the device.  out is [owner rows][r_pad]; every padded column is
 *                              written (0).  Entries accumulate in storage order, a split row's partials in segment order:
 *                              plain stores only, no atomics -- a repeated call is bitwise identical.
 * Other beta: NMFMU_ERR_UNSUPPORTED.  rank <= 256. */
int64_t nmfmu_sp_div_backward_ws(int n_multi_segments, int r_pad);
int nmfmu_sp_div_forward(const int32_t* seg, int n_seg, const int32_t* colidx, const float* vals, const float* owner,
                         const float* panel, int rank, float beta, float* s_out, double* part, double* out, void* stream);
int nmfmu_sp_div_backward(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                          const float* vals, const int32_t* perm, const float* s, const float* panel, int rank, float beta,
                          const float* pos, int pos_plane, const float* up, float* ws, float* out, int r_pad, void* stream);

/* ---- missing-data NMF: a sparse target fitted over its STORED entries only, every beta (additive entries) ---------------------
 * The unstored entries are unknown, not zero: both contractions of the multiplicative update run over the stored set,
 *   s_p = <owner[row], panel[idx[p]]>,  num[row] = sum_p g_neg(v_p, s_p) panel[idx[p]],  den[row] = sum_p g_pos(s_p) panel[idx[p]]
 * with g_neg / g_pos = output_neg / output_pos of nmf.py:61-74 (beta 2: v, s; beta 1: v / (s + eps), 1; beta 0: v / (s + eps)^2,
 * 1 / (s + eps); otherwise v (s + eps)^(beta - 2), (s + eps)^(beta - 1)).  seg / multi are the segment lists of
 * nmfmu_sp_div_backward; one call per side: the H side takes the CSR list, the W side the CSC list with vals in CSC order.
 * Entries accumulate in storage order, a split row's partial [num | den] rows (ws[slot][2 r_pad]) in segment order: plain
 * stores only, no atomics -- a repeated call is bitwise identical.
 *   nmfmu_sp_masked_ws    : floats of `ws` = (sum of `segments` over multi) * 2 * r_pad -- a pure function of the counts
 *   nmfmu_sp_masked_terms : num, den [owner rows][r_pad]; every padded column is written (0); a row without entries gets zeros.
 *                           den - num is the gradient of the masked loss with respect to the owner.
 *   nmfmu_sp_masked_step  : the same terms, then nmf.py:78-92 in place on the owner's fp32 master [owner rows][rank]:
 *                           f *= ((relu(num) + eps) / (relu(den) + eps + l1 + l2 f))^gamma.  owner != panel.
 *   nmfmu_sp_masked_loss  : *out = metrics.beta_div(s, v, beta) over the stored entries (seg: the CSR list, owner = H), with the
 *                           reference's eps conventions per branch (metrics.py:22, 39, 57, 85-96).  The terms that hold s are
 *                           summed in double per wave, per workgroup, then in block order; v_term carries the terms of v alone,
 *                           formed by the caller in float64: beta 2: 0; beta 1: sum v log(v + eps) - sum v; beta 0:
 *                           -sum log(v + eps) - nnz; otherwise sum v'^beta (v' = v + eps when beta < 0, else v).
 *                           part: (n_seg + 3) / 4 doubles of scratch.
 * Null pointers, n_seg <= 0, rank <= 0, r_pad != nmfmu_pad_rank(rank): NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both
 * before any device work. */
int64_t nmfmu_sp_masked_ws(int n_multi_segments, int r_pad);
int nmfmu_sp_masked_terms(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                          const float* vals, const float* owner, const float* panel, int rank, float beta, float* ws,
                          float* num, float* den, int r_pad, void* stream);
int nmfmu_sp_masked_step(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* idx,
                         const float* vals, float* owner, const float* panel, int rank, float beta, float l1, float l2,
                         float gamma, float* ws, int r_pad, void* stream);
int nmfmu_sp_masked_loss(const int32_t* seg, int n_seg, const int32_t* colidx, const float* vals, const float* owner,
                         const float* panel, int rank, float beta, double v_term, double* part, double* out, void* stream);

/* ---- weighted NMF on a dense target: dense per-entry weights or a dense mask, every beta (additive entries) -------------------
 * L = sum_ij m_ij d_beta(v_ij | y_ij), y = H W^T, m >= 0.  V and M are row-major [n][c] fp32 with the row stride ld (floats).
 * side 0 is the H half (owner = H [n][rank], panel = W [c][rank], contraction over the columns of V), side 1 the W half
 * (owner = W, panel = H, V and M walked along their columns in place: no transposed copy exists).  Both seeds of nmf.py:61-74
 * are multiplied by m:
 *   num[i][r] = sum_k (m g_neg(v, y))(i, k) panel[k][r],   den[i][r] = sum_k (m g_pos(y))(i, k) panel[k][r]
 * (g_neg / g_pos as listed for the missing-data entries above).  Where m == 0 the entry is selected away, not multiplied:
 * V may hold NaN, Inf or a negative value there.  One fused exact-fp32 MFMA kernel (v_mfma_f32_32x32x2_f32: y over the full
 * padded rank, the elementwise seeds in LDS, both accumulators in registers; y and m g never reach HBM).  The contraction
 * is cut into parts of whole 32-step stages: nsplit == 0 takes nmfmu_wmu_nsplit(owner rows, contraction, r_pad), a pure
 * function of the shape; nsplit > 0 asks for that many (no empty part, only the last one short).  The parts' planes go to
 * ws [part][num | den][owner rows][r_pad] with plain stores and a second kernel adds them in part order: no atomics, no
 * fences -- a repeated call is bitwise identical whatever ws held.  16-byte loads of V and M when ld % 4 == 0 and both bases
 * are 16-byte aligned, scalar loads otherwise.
 *   nmfmu_wmu_ws         : floats of `ws` = parts * 2 * rows * r_pad -- a pure function of its four arguments (0 if one is bad)
 *   nmfmu_wmu_terms      : num, den [owner rows][r_pad]; every element is written, the padded columns with 0.  den - num is
 *                          the gradient of the weighted loss with respect to the owner.
 *   nmfmu_wmu_step       : the same terms, then nmf.py:78-92 in place on the owner's fp32 master [owner rows][rank]:
 *                          f *= ((relu(num) + eps) / (relu(den) + eps + l1 + l2 f))^gamma, applied by the second kernel once
 *                          every part of every row tile is done (each reads the owner).  owner != panel.
 *   nmfmu_wmu_loss       : *out = sum_ij m_ij (the term of metrics.beta_div at (i, j)), the reference's eps conventions per
 *                          branch (metrics.py:22, 39, 57, 85-96).  The terms that hold y are summed in double per lane, per
 *                          wave, per workgroup, then in block order; v_term carries sum m (the terms of v alone), formed by
 *                          the caller in float64 as for nmfmu_sp_masked_loss.  part: nmfmu_wmu_loss_parts(n, c) doubles.
 * Null pointers, n, c, rank <= 0, ld < c, side not 0 / 1, r_pad != nmfmu_pad_rank(rank), nsplit < 0: NMFMU_ERR_ARG; rank > 256:
 * NMFMU_ERR_UNSUPPORTED -- both before any device work. */
int nmfmu_wmu_nsplit(int rows, int contraction, int r_pad);
int64_t nmfmu_wmu_ws(int rows, int contraction, int r_pad, int nsplit);
int nmfmu_wmu_terms(const float* V, const float* M, int64_t ld, int n, int c, int side, const float* owner,
                    const float* panel, int rank, int r_pad, float beta, int nsplit, float* ws, float* num, float* den,
                    void* stream);
int nmfmu_wmu_step(const float* V, const float* M, int64_t ld, int n, int c, int side, float* owner, const float* panel,
                   int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit, float* ws, void* stream);
int nmfmu_wmu_loss_parts(int n, int c);
int nmfmu_wmu_loss(const float* V, const float* M, int64_t ld, int n, int c, const float* H, const float* W, int rank,
                   float beta, double v_term, double* part, double* out, void* stream);

/* ---- batched NMF: `batch` independent problems of one shape per launch, each stopped on its own (additive entries) ------------
 * Problem b: V_b [n][c] fp32, row stride ld, at V + b * v_batch_stride floats (v_batch_stride == 0: ONE target shared by every
 * problem -- restarts), H_b [n][rank] and W_b [c][rank] contiguous fp32 masters, the factors of the batch stored
 * [batch][rows][rank].  The unweighted update of nmf.py:61-92 per problem on the tile arithmetic of the nmfmu_wmu entries
 * (exact fp32 MFMA, y over the full padded rank, both contractions in registers; side 0: owner = H, side 1: owner = W with V
 * walked along its columns in place; 16-byte loads of V when ld % 4 == 0, v_batch_stride % 4 == 0 and V is 16-byte aligned).
 * The contraction is cut into parts by nmfmu_bmu_nsplit(owner rows, contraction, r_pad) == nmfmu_wmu_nsplit of the same
 * arguments: THE BATCH DOES NOT ENTER, so the bits of a problem do not depend on how many others are fitted alongside it.
 * ws is [problem][part][num | den][owner rows][r_pad], written with plain stores and added in part order by a second kernel:
 * no atomics, a repeated call is bitwise identical whatever ws held.  The problem index is the slow part of grid.x; a batch
 * whose grid.x would pass 2^31 - 1 workgroups is refused with NMFMU_ERR_UNSUPPORTED (the 65 535 limit of y / z never sees it).
 * active: NULL (every problem) or int32 [batch] on the device; every kernel leaves at once for a problem whose flag is 0 --
 * neither its factors, its slice of ws, its partials nor its `out` are touched.
 *   nmfmu_bmu_ws         : floats of `ws` = batch * parts * 2 * rows * r_pad (0 if an argument is bad)
 *   nmfmu_bmu_terms      : num, den [batch][owner rows][r_pad]; every element of an active problem is written, the padded
 *                          columns with 0.  den - num is the gradient of the problem's loss with respect to its owner.
 *   nmfmu_bmu_step       : the same terms, then nmf.py:78-92 in place on the owners.  owner != panel.
 *   nmfmu_bmu_loss       : out[b] = metrics.beta_div(H_b W_b^T, V_b, beta) in float64.  The terms that hold y are summed in
 *                          double per lane, per wave, per workgroup (part: batch * nmfmu_bmu_loss_parts(n, c) doubles), then per
 *                          problem in block order; v_term [batch] (device) carries the terms of v alone, as
 *                          nmfmu_bmu_v_term forms them.
 *   nmfmu_bmu_v_term     : out[b] = the sum over V_b of the terms of metrics.beta_div that hold v alone (beta 2: 0; beta 1:
 *                          v log(v + eps) - v; beta 0: -log(v + eps) - 1; otherwise v'^beta, v' = v + eps when beta < 0), every
 *                          term and the sum in double: one workgroup per problem, strided lanes, then a tree -- a function of
 *                          the problem's own entries alone.  Once per fit; a shared target is one problem (batch = 1).
 *   nmfmu_bmu_judge      : the stop rule of nmf.py:402-407 in double, one thread per active problem: loss = sqrt(2 div[b]) (NaN
 *                          when div[b] < 0: such a problem never stops); if (previous[b] - loss) / loss_init[b] < tol the
 *                          problem stops: n_iter[b] = iteration + 1, active[b] = 0; otherwise previous[b] = loss.  *n_active =
 *                          the number of problems still active.  One workgroup, no atomics.
 * Null pointers (active may be NULL except for the judge), batch, n, c, rank <= 0, ld < c, v_batch_stride < 0, side not 0 / 1,
 * r_pad != nmfmu_pad_rank(rank), owner == panel, nsplit < 0, iteration < 0: NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED --
 * both before any device work. */
int nmfmu_bmu_nsplit(int rows, int contraction, int r_pad);
int64_t nmfmu_bmu_ws(int batch, int rows, int contraction, int r_pad, int nsplit);
int nmfmu_bmu_terms(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, int side, const float* owner,
                    const float* panel, int rank, int r_pad, float beta, int nsplit, const int32_t* active, float* ws,
                    float* num, float* den, void* stream);
int nmfmu_bmu_step(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, int side, float* owner,
                   const float* panel, int rank, int r_pad, float beta, float l1, float l2, float gamma, int nsplit,
                   const int32_t* active, float* ws, void* stream);
int nmfmu_bmu_loss_parts(int n, int c);
int nmfmu_bmu_loss(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, const float* H, const float* W,
                   int rank, float beta, const double* v_term, const int32_t* active, double* part, double* out,
                   void* stream);
int nmfmu_bmu_v_term(const float* V, int64_t v_batch_stride, int64_t ld, int batch, int n, int c, float beta, double* out,
                     void* stream);
int nmfmu_bmu_judge(int batch, const double* div, const double* loss_init, double* previous, double tol, int iteration,
                    int32_t* active, int64_t* n_iter, int32_t* n_active, void* stream);

/* ---- batched NMF with per-problem weights and a per-problem regulariser (additive entries) -------------------------------------
 * The nmfmu_bmu entries with dense weights: problem b reads M_s [n][c] fp32, V's row stride ld, at M + s * m_batch_stride floats,
 * s = m_index[b] when m_index (int32 [batch] on the device, values validated by the caller) is given, else s = b;
 * m_batch_stride == 0: one weight matrix for every problem.  Cross-validation shares K fold masks among K x starts x alphas
 * problems through m_index and the target through v_batch_stride == 0: nothing of size batch x n x c exists.  The arithmetic is
 * the nmfmu_wmu entries' per problem -- both seeds multiplied by m, an entry with m == 0 SELECTED away (V may hold NaN, Inf or
 * a negative value there), the same tile, part order and apply: problem b of nmfmu_bwmu_terms / _step is bitwise
 * nmfmu_wmu_terms / _step on (V_b, M_b) with the same nsplit.  A problem's bits do not depend on the batch, its position in
 * it, or whether V or M are shared or indexed.  16-byte loads of V and M when ld, both batch strides and both bases allow,
 * scalar loads otherwise.  ws, the split and the loss partials are nmfmu_bmu_ws / nmfmu_bmu_nsplit / nmfmu_bmu_loss_parts'
 * (neither the batch nor the weights enter the split); nmfmu_bmu_judge serves unchanged.  An inactive problem is not touched.
 *   reg (nmfmu_bwmu_step) : NULL, or fp32 [batch][2] on the device: problem b's (l1, l2), replacing the scalars -- one launch
 *                           sweeps the regulariser.
 *   M == NULL             : the unweighted kernels: bitwise the nmfmu_bmu entries (reg still honoured).
 *   nmfmu_bwmu_loss       : out[b] = sum_ij m_ij (the term of metrics.beta_div at (i, j)) in float64, summed as nmfmu_bmu_loss.
 *   nmfmu_bwmu_v_term     : out[b] = sum m (the terms of metrics.beta_div that hold v alone) over problem b's weighted entries,
 *                           every term, the product and the sum in double, in nmfmu_bmu_v_term's fixed order: a function of
 *                           (V_b, M_b) alone.
 * The argument errors of the nmfmu_bmu entries, and m_batch_stride < 0 or m_index given with M == NULL: NMFMU_ERR_ARG -- before
 * any device work. */
int nmfmu_bwmu_terms(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                     int64_t ld, int batch, int n, int c, int side, const float* owner, const float* panel, int rank, int r_pad,
                     float beta, int nsplit, const int32_t* active, float* ws, float* num, float* den, void* stream);
int nmfmu_bwmu_step(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                    int64_t ld, int batch, int n, int c, int side, float* owner, const float* panel, int rank, int r_pad,
                    float beta, float l1, float l2, const float* reg, float gamma, int nsplit, const int32_t* active, float* ws,
                    void* stream);
int nmfmu_bwmu_loss(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                    int64_t ld, int batch, int n, int c, const float* H, const float* W, int rank, float beta,
                    const double* v_term, const int32_t* active, double* part, double* out, void* stream);
int nmfmu_bwmu_v_term(const float* V, int64_t v_batch_stride, const float* M, int64_t m_batch_stride, const int32_t* m_index,
                      int64_t ld, int batch, int n, int c, float beta, double* out, void* stream);

/* ---- PLCA's EM update (plca.py:248-290) -----------------------------------------------------------------------------
 * With G = Vn / (H diag(Z) W^T + eps) the factor "gradients" are (G^T H) * Z, (G W) * Z and Z.grad[r] = sum W * (G^T H);
 * nmfmu_mu_partial delivers the unscaled numerators G^T H / G W when the step's panel struct carries the image of the
 * Z-scaled factor as p1 (reconstruction) and of the unscaled factor as p2.  part: nmfmu_plca_part_bytes() of scratch.
 *   nmfmu_plca_em        f *= relu(num * z_old) (skipped when update == 0); colsum_out = column sums of the result;
 *                        zgrad_out (may be NULL) = sum_rows f_old * num
 *   nmfmu_plca_normalize f /= divider[r]; when alpha != 1: f += (float)(alpha - 1.0), clamped below at eps; colsum_out =
 *                        column sums.  alpha is a double so that the constant is the reference's: the subtraction in double,
 *                        one rounding to fp32 (the same in nmfmu_plca_z and nmfmu_plca3)
 *   nmfmu_plca_scale     f /= colsum[r] */
size_t nmfmu_plca_part_bytes(int rows, int r_pad);
int nmfmu_plca_em(float* f, int rows, int rank, int r_pad, const float* num, int nslab, int rows_pad, const float* z_old,
                  int update, float* part, float* colsum_out, float* zgrad_out, void* stream);
int nmfmu_plca_normalize(float* f, int rows, int rank, int r_pad, const float* divider, double alpha, float* part,
                         float* colsum_out, void* stream);
int nmfmu_plca_scale(float* f, int rows, int rank, const float* colsum, void* stream);
/* plca.py:253-260 in one launch: prior[r] = z[r] * relu(zgrad[r]); z <- prior (+ alpha - 1, clamped below at eps when
 * alpha != 1), then z /= sum(z).  rank <= 256. */
int nmfmu_plca_z(float* z, const float* zgrad, int rank, double alpha, float* prior, void* stream);

/* ---- PLCA on a sparse-COO target: the E-step over the STORED entries only (additive entries) ----------------------------------
 * Where Vn is zero, G = Vn / (H diag(Z) W^T + eps) is zero and adds nothing to G W, G^T H or Z.grad: both unscaled numerators of
 * an EM iteration are sums over the stored set, exactly.  seg / multi are the segment lists of nmfmu_sp_div_backward; vals_n are
 * the stored values divided by their total, in CSR order; the factors are the fp32 masters [rows][rank].  One reconstruction
 * feeds every update of the iteration (plca.py:252): g is formed once, on the H side, and the W side reads it back.
 *   nmfmu_sp_plca_estep  : H side, the CSR list.  Per stored entry p of row i, j = colidx[p]:
 *                          s_p = sum_r (owner[i][r] * z[r]) * panel[j][r] (the row scaled once per segment; fixed-order butterfly),
 *                          g_p = vals_n[p] / (s_p + eps), g_out[p] = g_p (one float per stored entry, CSR order, written once),
 *                          num[i][:] = sum_p g_p * panel[j][:]  = (G W)[i].  owner = H, panel = W, z [rank].
 *   nmfmu_sp_plca_gather : W side, the CSC list.  num[j][:] = sum_p g[perm[p]] * panel[rowidx[p]][:] = (G^T H)[j]; perm[p] = the
 *                          CSR position of CSC entry p; panel = H.  No dot product, no cross-lane reduction, no divide.
 * num is [owner rows][r_pad]: every padded column is written (0), a row without entries gets zeros -- the single slab
 * nmfmu_plca_em reads (nslab = 1, rows_pad = rows).  Entries accumulate in storage order, a split row's partial rows
 * (ws[slot][r_pad]; the size rule is nmfmu_sp_div_backward_ws) in segment order: plain stores only, no atomics -- a repeated
 * call is bitwise identical.
 * Null pointers, n_seg <= 0, rank <= 0, r_pad != nmfmu_pad_rank(rank): NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both
 * before any device work. */
int nmfmu_sp_plca_estep(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* colidx,
                        const float* vals_n, const float* owner, const float* z, const float* panel, int rank, float* g_out,
                        float* ws, float* num, int r_pad, void* stream);
int nmfmu_sp_plca_gather(const int32_t* seg, int n_seg, const int32_t* multi, int n_multi, const int32_t* rowidx,
                         const int32_t* perm, const float* g, const float* panel, int rank, float* ws, float* num, int r_pad,
                         void* stream);

/* ---- scoring a fitted model without the N x C product (additive entries; scoring.py) ---------------------
 * H [N][rank] and W [C][rank] are fp32 masters; a score is s_ij = <H[i], W[j]>.
 *   nmfmu_score_pairs : out[p] = s at (rows[p], cols[p]), p < n; the pairs may repeat and come in any order.  The caller
 *                       answers for 0 <= rows[p] < N and 0 <= cols[p] < C.  n == 0 launches nothing.
 *   nmfmu_topk        : for each of the n_rows requested rows (row_ids, or rows 0 .. n_rows - 1 when it is NULL) the k largest
 *                       scores over the admissible columns, score descending and equal scores by ascending column; a row with
 *                       fewer than k admissible columns ends in (-inf, -1).  out_val / out_idx are [n_rows][k].  The stored
 *                       columns of row i of a CSR pattern -- ex_colidx[ex_rowptr[i] .. ex_rowptr[i + 1]), ascending -- are
 *                       inadmissible.  The columns are cut into nsplit ranges of whole 128-column tiles; with nsplit > 1 the
 *                       ranges' lists go to ws and a second kernel merges them.  Exact-fp32 MFMA; the result does not depend
 *                       on nsplit.
 *   nmfmu_topk_ws     : bytes of ws (0 for nsplit == 1): n_rows * nsplit * k * 8 -- a pure function of its arguments.
 * Null pointers (row_ids, ex_rowptr and, for nsplit == 1, ws may be NULL), sizes < 1, rank <= 0, k < 1, nsplit < 1:
 * NMFMU_ERR_ARG; rank > 256 or k > 128: NMFMU_ERR_UNSUPPORTED -- both before any device work.  No atomics: a repeated call is
 * bitwise identical. */
int nmfmu_score_pairs(const int32_t* rows, const int32_t* cols, int64_t n, const float* H, int N, const float* W, int C,
                      int rank, float* out, void* stream);
int64_t nmfmu_topk_ws(int n_rows, int k, int nsplit);
int nmfmu_topk(const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C, int rank, int k,
               const int32_t* ex_rowptr, const int32_t* ex_colidx, int nsplit, void* ws, float* out_val, int32_t* out_idx,
               void* stream);

/* ---- full-ranking evaluation without the n_rows x C score matrix (additive entries; scoring.py) ---------
 * Scores, the order and the exclusion pattern are nmfmu_topk's.  The held-out pattern is a CSR over the n_rows REQUESTED rows
 * (row_ids, or rows 0 .. n_rows - 1 when it is NULL): ho_colidx[ho_rowptr[r] .. ho_rowptr[r + 1]), ascending, are the held-out
 * columns of requested row r; n_pairs = ho_rowptr[n_rows] is read on the device.  ex_rowptr / ex_colidx are indexed by the
 * original row, as in nmfmu_topk, and may be NULL.  For every pair e = (i, c):
 *   out_score[e] = the score tile's fp32 value of (i, c), the bits nmfmu_topk returns for that row and column;
 *   out_rank[e]  = the number of admissible columns j != c of row i with s_ij > s_ic, or s_ij == s_ic and j < c (0-based); -1
 *                  when the exclusion pattern stores (i, c) itself;
 *   out_admissible[r] = C - (stored columns of the row in the exclusion pattern).
 * Three launches on `stream`: pass 0 extracts the scores and sets the -1 flags, pass 1 counts per (pair, split) into ws, pass 2
 * adds the nsplit partial counts.  Counts are integers: the result does not depend on nsplit or on the form of the count.
 *   nmfmu_rank_pairs : the three passes in order, every row choosing the form of its count (the per-lane scan above 24 held-out
 *                      pairs, one ballot per threshold below).  A requested row with an empty held-out range writes nothing but
 *                      its out_admissible; the entry does not learn n_pairs on the host, so a caller without pairs does not call.
 *   nmfmu_rank_pass  : one of the passes alone (pass 0 / 1 / 2), for timing them apart; form 0 = as nmfmu_rank_pairs, 1 = the
 *                      ballot form for every row, 2 = the scan form for every row, form > 2 = the scan form above `form`
 *                      held-out pairs (pass 1 reads it; for measuring where the two forms cross).
 *   nmfmu_rank_ws    : bytes of ws: n_pairs * nsplit * 4 (0 when an argument is < 1) -- a pure function of its arguments.
 * Null pointers (row_ids and ex_rowptr may be NULL), sizes < 1, rank <= 0, nsplit < 1, a pass outside 0 .. 2, form < 0:
 * NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both before any device work.  No atomics: a repeated call is bitwise
 * identical. */
int64_t nmfmu_rank_ws(int64_t n_pairs, int n_rows, int nsplit);
int nmfmu_rank_pairs(const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C, int rank,
                     const int32_t* ho_rowptr, const int32_t* ho_colidx, const int32_t* ex_rowptr, const int32_t* ex_colidx,
                     int nsplit, void* ws, float* out_score, int32_t* out_rank, int32_t* out_admissible, void* stream);
int nmfmu_rank_pass(int pass, int form, const float* H, int N, const int32_t* row_ids, int n_rows, const float* W, int C,
                    int rank, const int32_t* ho_rowptr, const int32_t* ho_colidx, const int32_t* ex_rowptr,
                    const int32_t* ex_colidx, int nsplit, void* ws, float* out_score, int32_t* out_rank,
                    int32_t* out_admissible, void* stream);

/* ---- source separation: per-group soft masks of a fitted model (additive entries; separation.py) ----------
 * With Y_g the reconstruction from the components of group g alone, D = sum_{g < groups} Y_g^power in ascending g (power == 1:
 * the one reconstruction over all components), every output plane s holds  v * (Y_g^power / (D + eps))  for the group g with
 * slot[g] == s.  v_kind 0: no mixture (v = 1, fp32 planes); 1: V real fp32 [n][ldv]; 2: V complex64 read as interleaved floats
 * (ldv in complex elements), planes complex64 -- the real mask multiplies both parts.  slot [groups] (HOST) maps a group to its
 * output plane, -1 for none; at most one group per plane is the caller's business.  Every element of every mapped plane is
 * written; Y_g and D are never stored.
 *   nmfmu_separate        : dense models on one fused exact-fp32 MFMA kernel (the tile of nmfmu_reconstruct).  Hp [n][cols] and
 *                           Wp [c][cols] are the factors with the components sorted by group and every group padded with zero
 *                           columns to an even count; gstart [groups + 1] (HOST) are the groups' first columns: gstart[0] == 0,
 *                           gstart[groups] == cols, ascending, every entry even (an empty group has equal neighbours).  Plane s is
 *                           out + s * n * ld (elements), row stride ld.  tables_dev: nmfmu_separate_tables_bytes(groups) bytes on
 *                           the device that the CALLER has filled with gstart [groups + 1] followed by slot [groups]: the
 *                           kernel reads that copy, the library validates the host arrays (read only during the call) and
 *                           copies nothing.  16-byte loads of the factors when cols % 4 == 0 and Hp, Wp are 16-byte aligned,
 *                           scalar otherwise; V and out must be aligned to their element (8 bytes for v_kind 2), else
 *                           NMFMU_ERR_ARG.  groups <= nmfmu_separate_max_rank() and cols <= twice that, else
 *                           NMFMU_ERR_UNSUPPORTED.
 *   nmfmu_separate_planes : the planes Y_g are given: element i of plane g at Y[g * y_stride + i * y_elem], y_elem 1 or 2 (2: the
 *                           planes sit in the real slots of a complex output).  D: NULL, or the denominator plane [n] to use
 *                           instead of the sum.  Output plane s is out + s * out_stride (elements).  An input plane may be the
 *                           output plane of its own group (same element positions).  slot_dev: groups * 4 bytes on the device
 *                           that the CALLER has filled with slot (the kernel reads it; the host array is what is validated).
 *                           16-byte accesses when every base is 16-byte aligned and the strides are multiples of four floats.
 *   nmfmu_separate_accumulate : D[i] += Y[i * y_elem]^power for i < n, with the very operation the two kernels above use for their
 *                           own sums (power == 2: one fused multiply-add), so a denominator accumulated plane by plane in
 *                           ascending g from a zero plane has the bits of the one nmfmu_separate_planes forms itself.
 * Null pointers, sizes < 1, ld / ldv below c, y_stride below n * y_elem, out_stride below n, power <= 0 or not a number, eps < 0, an
 * unknown v_kind or y_elem, a boundary table that is not as described, a slot outside [-1, planes): NMFMU_ERR_ARG -- before any
 * device work.  No atomics: a repeated call is bitwise identical, and a plane's bits do not depend on the other slots. */
int nmfmu_separate_max_rank(void);
int64_t nmfmu_separate_tables_bytes(int groups);
int nmfmu_separate(const float* Hp, int n, const float* Wp, int c, int cols, const int32_t* gstart, const int32_t* slot,
                   int groups, int planes, void* tables_dev, const float* V, int v_kind, int64_t ldv, float power, float eps,
                   float* out, int64_t ld, void* stream);
int nmfmu_separate_planes(const float* Y, int groups, int64_t y_stride, int y_elem, const float* D, const float* V, int v_kind,
                          int64_t n, float power, float eps, const int32_t* slot, int planes, void* slot_dev, float* out,
                          int64_t out_stride, void* stream);
int nmfmu_separate_accumulate(const float* Y, int y_elem, int64_t n, float power, float* D, void* stream);

/* ---- fold-in: new rows against a fixed W, all iterations in one launch (additive entries; fold_in.py) ----
 * The new rows come as CSR (rowptr [n_rows + 1], colidx / vals [nnz], int32 indices below n_cols); H [n_rows][rank] holds the
 * start H0 on entry and the result on return; W [n_cols][rank] is read only.  Per row, with S its stored columns, max_iter times
 *   s_j = <h, W[j]>,  h *= ((relu(num) + eps) / (den' + l1 + l2 h))^gamma                                        (nmf.py:78-92)
 *   NMFMU_FOLD_MISSING, any beta : num = sum_S g_neg(v_j, s_j) W[j], den' = relu(sum_S g_pos(s_j) W[j]) + eps -- g as in
 *                                  nmfmu_sp_masked_step; aux is not read (may be NULL)
 *   NMFMU_FOLD_ZERO, beta 1      : num = sum_S v_j / (s_j + eps) W[j], den' = aux[r], the column sums of W as they are
 *                                  (nmf.py:128-131; nmfmu_rank_sums(W, n_cols, rank, 1, ..))
 *   NMFMU_FOLD_ZERO, beta 2      : num = sum_S v_j W[j] (formed once), den' = relu(sum_q h[q] aux[q][r]) + eps, aux = W^T W
 *                                  [rank][rank] (nmfmu_gram)
 * A row stops after iteration k when max_r |h_k[r] - h_{k-1}[r]| <= tol * max_r h_k[r] (fp32; tol == 0: never) and
 * n_iter_rows[row] (may be NULL) receives its iteration count.  order (may be NULL): int32 [n_rows], the rows in the order they
 * are handed out -- longest first balances the launch; it does not change any result.  block / long_rows (0 = default): stored
 * entries per LDS block (clamped to nmfmu_fold_in_block(rank), what the LDS holds) and the count above which a row takes a whole
 * workgroup (default nmfmu_fold_in_block(rank): what one wave keeps resident).  A row's result is bitwise independent of block, of order and of the other rows of the call; plain
 * stores only, no atomics -- a repeated call is bitwise identical.
 * Null pointers (aux in zero mode included), rank <= 0, n_rows < 0, n_cols <= 0, max_iter < 0, tol < 0, block < 0, long_rows < 0
 * or an unknown mode: NMFMU_ERR_ARG; rank > 256, or zero mode with beta not in {1, 2}: NMFMU_ERR_UNSUPPORTED; n_rows == 0 or
 * max_iter == 0: NMFMU_OK without a launch, H untouched -- all before any device work. */
#define NMFMU_FOLD_MISSING 0
#define NMFMU_FOLD_ZERO 1
int nmfmu_fold_in_block(int rank);   /* the default (and largest) block of a rank; 0 outside 1 .. 256 */
int nmfmu_fold_in(const int32_t* rowptr, const int32_t* colidx, const float* vals, int n_rows, float* H, const float* W,
                  int n_cols, int rank, float beta, int mode, const float* aux, float l1, float l2, float gamma,
                  int max_iter, float tol, int32_t* n_iter_rows, const int32_t* order, int block, int long_rows,
                  void* stream);

/* ---- fold-in by coordinate descent, beta == 2 (additive entries; fold_in.py) --------------------------
 * nmfmu_fold_in_cd: the new rows as for nmfmu_fold_in (CSR; H holds H0 on entry and the result on return; W read only), every
 * iteration of every row in ONE launch, for the objective of a row h
 *   1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 + l1 sum h + l2/2 |h|^2,   0 <= omega <= 1,   y_j = <h, W[j]>
 * -- omega = 0: the stored entries only ('missing', nmfmu_sp_ccd_sweep's recurrence); 0 < omega < 1: nmfmu_sp_wccd_sweep's;
 * omega = 1: every unstored entry an observed zero ('zero', HALS on the row).  gram [rank][rank] = W^T W, SYMMETRIC as nmfmu_gram
 * writes it (coordinate k reads its row k only); may be NULL iff omega == 0.  With c = 1.0f - omega (fp32), per row, once:
 *   d_k = sum_e W[j_e][k]^2,  D_k = fma(c, d_k, omega * gram[k][k])  (omega == 0: D_k = d_k),  omega == 1: n_k = sum_e v_e W[j_e][k]
 * and max_iter times
 *   t_e = fma(-c, s_e, v_e),  s_e = sum_k h[k] W[j_e][k]   (k ascending, one fused multiply-add chain from 0; formed anew from h
 *                                                           in every iteration)
 *   for k = 0 .. rank-1:  n = sum_e t_e W[j_e][k]  (omega == 1: n_k),   q = sum_j h[j] gram[k][j]   (omega == 0: none)
 *                         h' = max(eps, (fma(h[k], D_k, fma(-omega, q, n)) - l1) / ((D_k + l2) + eps)),   eps = 2^-23
 *                              (omega == 0: fma(h[k], D_k, n) - l1 above the same denominator)
 *                         t_e = fma(-(c * (h' - h[k])), W[j_e][k], t_e) for every e;   h[k] = h'
 * A row stops after iteration k when max_r |h_k[r] - h_{k-1}[r]| <= tol * max_r h_k[r] (fp32; tol == 0: never); n_iter_rows
 * (may be NULL) receives the count.  A row without entries: omega == 0 leaves it untouched (count 1 with tol > 0, else max_iter),
 * omega > 0 sweeps it.  There is no initial scaling: H is used as it comes.
 * Arithmetic: fp32.  A row of at most long_rows entries (0 = nmfmu_fold_in_cd_long_rows(rank)) is worked by one wave, a longer
 * one by the NW = 4 waves of its workgroup: wave w owns the entries [w per, (w + 1) per), per = ceil(count / NW), local entry i on
 * lane i mod 64 as slot i / 64.  d, n, n_k: per-lane fused multiply-add chains over the slots in ascending order from 0, an xor
 * butterfly 32 .. 1 per wave, the waves' totals added in wave order.  q: lane l runs fma(h[l + 64 m], gram[k][l + 64 m], q)
 * for m = 0 .. 3 from 0 (coordinates beyond the rank left out), then the same butterfly.  block (0 = nmfmu_fold_in_cd_block(rank),
 * also the largest value): the largest share per whose W rows are staged in LDS once per row; above it W[j_e][k] is gathered
 * from W at every use -- the same floats.  A row whose share exceeds the wave's LDS (more than 7100 .. 9400 entries, by the rank) keeps no
 * residuals and forms t_e from h as it stands for every coordinate.  order as for nmfmu_fold_in.  A row's bits depend on its
 * entries, its row of H, W, gram, omega, l1, l2, max_iter, tol and long_rows alone -- not on block, order or the other rows;
 * plain vector stores, no atomics: a repeated call is bitwise identical.
 * Null rowptr / colidx / vals / H / W, H == W, gram NULL with omega > 0, rank <= 0, n_rows < 0, n_cols <= 0, max_iter < 0, tol < 0,
 * block < 0, long_rows < 0, omega outside [0, 1] or not a number: NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED; n_rows == 0
 * or max_iter == 0: NMFMU_OK without a launch, H untouched -- all before any device work. */
int nmfmu_fold_in_cd_block(int rank);       /* the default (and largest) staged share of a rank; 0 outside 1 .. 256 */
int nmfmu_fold_in_cd_long_rows(int rank);   /* the default count above which a row takes the workgroup: min(block, 128) */
int nmfmu_fold_in_cd(const int32_t* rowptr, const int32_t* colidx, const float* vals, int n_rows, float* H, const float* W,
                     int n_cols, int rank, const float* gram, float omega, float l1, float l2, int max_iter, float tol,
                     int32_t* n_iter_rows, const int32_t* order, int block, int long_rows, void* stream);

/* ---- HALS: coordinate descent for beta == 2 (additive entry; hals.py) ---------------------------------
 * nmfmu_hals_sweep: one Gauss-Seidel pass over the rank on f [rows][rank], in place, every row on its own.  With
 * a [rows][lda] = X_owner @ panel (lda >= rank elements per row: nmfmu_sp_partial writes r_pad, nmfmu_reconstruct_backward
 * rank) and gram [rank][rank] = panel^T panel (nmfmu_gram), for r = 0 .. rank-1 in this order
 *   s         = sum_{j != r} f[row][j] gram[j][r]                  (j < r: the values this pass already wrote)
 *   f[row][r] = max(eps, ((a[row][r] - l1) - s) / ((gram[r][r] + l2) + eps)),   eps = 2^-23
 * -- the exact minimiser of 1/2 |X - owner panel^T|^2 + l1 sum f + l2/2 |f|^2 along the coordinate, floored at eps (not 0:
 * a factor can be handed on to the multiplicative update, which never leaves an exact zero); the eps in the denominator
 * covers a panel column that is all floor.  gram must be SYMMETRIC (a Gram matrix is, and nmfmu_gram writes it so bit for
 * bit): coordinate r reads its row r.
 * Arithmetic: fp32; term j of s goes to accumulator j mod 4 by fused multiply-add in increasing j (the own term as an exact
 * +0), s = (acc0 + acc1) + (acc2 + acc3).  One lane per row, one 64-lane workgroup per 64 rows with the rows in LDS: a row's
 * bits depend on that row of f and a, on gram, l1 and l2 alone -- not on rows, the launch geometry or the other rows; plain
 * vector stores, no atomics: a repeated call is bitwise identical.  a and gram are only read; of f only [rows][rank] is
 * written.
 * Null pointers, rows <= 0, rank <= 0, lda < rank: NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both before any
 * device work. */
int nmfmu_hals_sweep(float* f, int rows, int rank, const float* a, int64_t lda, const float* gram, float l1, float l2,
                     void* stream);

/* ---- CCD: coordinate descent over the STORED entries, beta == 2 (additive entries; ccd.py) -------------
 * nmfmu_sp_ccd_sweep: one pass over the rank on owner [n_rows][rank], in place, for a target whose unstored entries are
 * MISSING.  rowptr / idx / vals: the owner side's CSR (H) or CSC (W) arrays; idx holds rows of panel [n_panel][rank].  Every
 * owner row i with stored entries e (panel row j_e, value v_e), on its own:
 *   r_e = v_e - sum_k owner[i][k] panel[j_e][k]                       (k ascending, one fused multiply-add chain from 0)
 *   for k = 0 .. rank-1:  d = sum_e panel[j_e][k]^2,  n = sum_e r_e panel[j_e][k]
 *                         f' = max(eps, (fma(owner[i][k], d, n) - l1) / ((d + l2) + eps)),   eps = 2^-23
 *                         r_e = fma(-(f' - owner[i][k]), panel[j_e][k], r_e) for every e;   owner[i][k] = f'
 * -- the exact minimiser of 1/2 sum_e (v_e - <owner[i], panel[j_e]>)^2 + l1 sum f + l2/2 |f|^2 along the coordinate, floored
 * at eps.  A row without entries is not touched.
 * Arithmetic: fp32.  A row of at most wg_rows entries (0: nmfmu_sp_ccd_limit()) is worked by one wave, a longer one by a
 * workgroup of NW = nmfmu_sp_ccd_wg_waves() waves (two launches over the same list; which one takes a row is a function of
 * its count and wg_rows).  Rows are taken in the order of `order` (int32 [n_rows], NULL: 0 .. n_rows-1; longest first keeps
 * the launches short, no result depends on it).  With NW waves on a row (1 or 16), entry e belongs to lane e mod 64 of wave
 * (e / 64) mod NW; d and n are per-lane fused multiply-add chains over the lane's entries in ascending e, then an xor
 * butterfly 32 .. 1 per wave, then the waves' totals added in wave order.
 * limit: a row of at most limit NW entries keeps its residuals in registers (0: nmfmu_sp_ccd_limit() = 512, also the largest
 * value); a longer row keeps them in its slice scratch[rowptr[i] .. rowptr[i + 1]) of scratch [nnz floats], which no other
 * row touches.  lds_rows: a one-wave row of at most min(lds_rows, nmfmu_sp_ccd_lds_rows(rank)) entries copies its panel rows
 * to LDS once; the other rows gather panel[j_e][k] from panel_t [rank][n_panel], a transposed copy this entry writes first
 * (one more small launch), or from panel itself when panel_t is NULL.  The same operations in the same order wherever the
 * residuals and the panel values live: a row's bits depend on that row of owner, its entries, panel, l1, l2 and wg_rows
 * alone -- not on limit, lds_rows, panel_t, order or the other rows.  Plain vector stores, no atomics: a repeated call is
 * bitwise identical.  panel, idx, vals are only read.
 * Null rowptr / idx / vals / owner / panel / scratch, owner == panel, n_rows < 0, n_panel <= 0, rank <= 0, limit outside
 * 0 .. 512, lds_rows < 0, wg_rows < 0: NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both before any device work. */
int nmfmu_sp_ccd_limit(void);          /* 512: entries per row whose residuals stay in registers */
int nmfmu_sp_ccd_wg_waves(void);       /* 16: waves of the workgroup that takes a row of more than wg_rows entries */
int nmfmu_sp_ccd_lds_rows(int rank);   /* entries per row whose panel rows fit the LDS stage; 0 outside rank 1 .. 256 */
int nmfmu_sp_ccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, int n_rows,
                       float* owner, const float* panel, int n_panel, int rank, float l1, float l2, float* scratch,
                       float* panel_t, int limit, int lds_rows, int wg_rows, void* stream);

/* ---- weighted CCD: unstored entries are zeros of confidence omega, beta == 2 (additive entry; wccd.py)
 * nmfmu_sp_wccd_sweep: one pass over the rank on owner [n_rows][rank], in place, for the objective
 *   1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 + l1 sum f + l2/2 |f|^2,   0 < omega < 1,   y = <owner[i], panel[j]>.
 * rowptr / idx / vals / order / scratch / limit / wg_rows as for nmfmu_sp_ccd_sweep; gram [rank][rank] = panel^T panel, SYMMETRIC
 * as nmfmu_gram writes it (coordinate k reads its row k only).  With c = 1.0f - omega (fp32), every owner row i with stored
 * entries e (panel row j_e, value v_e), on its own -- a row WITHOUT entries too (the Gram term acts on it; it is a one-wave row):
 *   t_e = fma(-c, s_e, v_e),  s_e = sum_k owner[i][k] panel[j_e][k]    (k ascending, one fused multiply-add chain from 0)
 *   for k = 0 .. rank-1:  d = sum_e panel[j_e][k]^2,  n = sum_e t_e panel[j_e][k],  q = sum_j owner[i][j] gram[k][j]
 *                                                                  (j < k: the values this pass wrote, j >= k: the old ones)
 *                         D  = fma(c, d, omega * gram[k][k])
 *                         f' = max(eps, (fma(owner[i][k], D, fma(-omega, q, n)) - l1) / ((D + l2) + eps)),   eps = 2^-23
 *                         t_e = fma(-(c * (f' - owner[i][k])), panel[j_e][k], t_e) for every e;   owner[i][k] = f'
 * -- the exact minimiser of the objective along the coordinate, floored at eps.
 * Arithmetic: fp32.  d and n: as in nmfmu_sp_ccd_sweep (per-lane chains over the lane's entries in ascending e, xor butterfly
 * 32 .. 1 per wave, the waves' totals added in wave order).  q: lane l runs fma(owner[i][l + 64 m], gram[k][l + 64 m], q) for
 * m = 0 .. 3 from 0 (coordinates beyond the rank left out), then the same butterfly; with 16 waves on a row every wave
 * computes q itself, with identical bits.  panel[j_e][k] is gathered from the row-major panel.  The same operations in the
 * same order wherever the residuals live: a row's bits depend on that row of owner, its entries, panel, gram, omega, l1, l2
 * and wg_rows alone -- not on limit, order or the other rows.  Plain vector stores, no atomics: a repeated call is bitwise
 * identical.  panel, gram, idx, vals are only read.
 * Null rowptr / idx / vals / owner / panel / gram / scratch, owner == panel, n_rows < 0, n_panel <= 0, rank <= 0, limit outside
 * 0 .. 512, wg_rows < 0, omega outside (0, 1) or not finite: NMFMU_ERR_ARG; rank > 256: NMFMU_ERR_UNSUPPORTED -- both before
 * any device work. */
int nmfmu_sp_wccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, int n_rows,
                        float* owner, const float* panel, int n_panel, int rank, const float* gram, float omega, float l1,
                        float l2, float* scratch, int limit, int wg_rows, void* stream);

/* ---- shift-invariant PLCA (SIPLCA / SIPLCA2 / SIPLCA3, plca.py:376-606) on the NMFD GEMM path ----------------------
 * Same EM update as PLCA with W (C, R, *T), H (B, R, *Lh): factors are addressed [outer][rank][inner], the unscaled
 * numerator as num[o * num_pitch + r * inner + i].
 *   nmfmu_conv_pack_w_scaled : Wm / WmT planes of W * scale[r] (the reconstruction operand W * Z); W is not modified
 *   nmfmu_convnd_fold        : out[b][r][j] = sum_t y[(r,t)][(b, j + t)]  (the fold of nmfmu_convnd_fold_apply_h alone)
 *   nmfmu_plca3              : mode 0 em (vec = z_old), 1 normalize (vec = divider, alpha), 2 scale (vec = colsum);
 *                              part: nmfmu_plca3_part_bytes(rank) of scratch */
int nmfmu_conv_pack_w_scaled(float* w, int channels, int rank, int taps, const float* scale, int c_pad, int rp_pad,
                             void* wm_hi, void* wm_lo, void* wmt_hi, void* wmt_lo, void* stream);
int nmfmu_convnd_fold(float* out, int batch, int rank, int ndim, const int32_t* lh, const int32_t* taps, const float* y,
                      int bl_pad, void* stream);
/* The two small kernels around the window-operand GEMM (NMFMU_OPS_A_WIN), F = nmfmu_gemm_desc.win_fold (>= 1):
 *   nmfmu_conv_pack_wk:      Wk[r F + d][((to TQ + q) CK + ck) 64 + c'] = w[c = 64 ck + c'][r][to taps_last + F q + d]
 *                            (CK = ceil(channels / 64), TQ = taps_last / F; taps = the product over the shift axes, innermost
 *                            last), planes [rows_pad][k_pad] zero padded
 *   nmfmu_conv_apply_h_rows: h (batch, rank, lh_outer, lh_last) in place by nmf.py:78-92 from num / den
 *                            [(b, jo, j')][ld], j' < lh_last + F - 1 (den NULL: beta == 1, kl_den[r] = sum_{c,t} W[c][r][t]) */
int nmfmu_conv_pack_wk(const float* w, int channels, int rank, int taps, int taps_last, int fold, int rows_pad, int k_pad,
                       int precision, void* wk_hi, void* wk_lo, void* stream);
int nmfmu_conv_apply_h_rows(float* h, int batch, int rank, int lh_outer, int lh_last, int fold, const float* num,
                            const float* den, const float* kl_den, int ld, float l1, float l2, float gamma, void* stream);
/* (ABI 8) The same two with their neighbours riding along -- four launches less per iteration of NMF2D / NMF3D / NMFD with a
 * short kernel (beta == 1, taps >= 64 in total, rank <= 256):
 *   nmfmu_conv_apply_pack_w_wk    = nmfmu_conv_apply_pack_w_sums (update, Wm / WmT planes, kl_hpart in, wcol out) + the Wk planes
 *                                   of nmfmu_conv_pack_wk from the same tile (their zero padding is NOT rewritten: run
 *                                   nmfmu_conv_pack_wk once on these buffers first);
 *   nmfmu_conv_apply_h_rows_sums  = nmfmu_conv_apply_h_rows for beta == 1 with sum_{c,t} W[c][r][t] finished in the kernel from
 *                                   the tile sums kl_wcol [c_tiles][rp_pad / 64][2] (nmfmu_conv_apply_pack_w_sums / _wk), and
 *                                   sum_{b,j} of the NEW h left as hsum_part[r][nmfmu_conv_h_rows_parts()] partials (fixed order)
 *                                   -- what kl_hpart / n_hparts of the next W update take. */
int nmfmu_conv_apply_pack_w_wk(float* w, int channels, int rank, int taps, const float* num, const float* den,
                               const float* kl_den, const float* kl_hpart, int n_hparts, float* wcol, int num_slabs,
                               int c_pad, int rp_pad, float l1, float l2, float gamma, int update, int precision,
                               void* wm_hi, void* wm_lo, void* wmt_hi, void* wmt_lo, int taps_last, int fold, int wk_rows_pad,
                               int wk_k_pad, void* wk_hi, void* wk_lo, void* stream);
int nmfmu_conv_h_rows_parts(int batch, int rank, int lh_outer, int lh_last);
int nmfmu_conv_apply_h_rows_sums(float* h, int batch, int rank, int lh_outer, int lh_last, int fold, const float* num,
                                 const float* kl_wcol, int c_tiles, int rp_pad, int taps, int ld, float l1, float l2, float gamma,
                                 float* hsum_part, void* stream);
/* ... and the sum alone: out (batch, rank, lh_outer, lh_last) = the folded numerator (shift-invariant PLCA's own update) */
int nmfmu_conv_rows_fold(float* out, int batch, int rank, int lh_outer, int lh_last, int fold, const float* num, int ld,
                         void* stream);
/* slabs[0][i] += slabs[1][i] + .. + slabs[nslab-1][i], fixed order: the partials of a split-K NMFMU_EPI_F32 launch
 * (k_split slabs of m_pad * n_ld floats) for a consumer that takes one slab.  slab_elems a multiple of 4. */
int nmfmu_slab_sum(float* slabs, int64_t slab_elems, int nslab, void* stream);
size_t nmfmu_plca3_part_bytes(int rank);
int nmfmu_plca3(int mode, float* f, int outer, int rank, int inner, const float* num, int64_t num_pitch, const float* vec,
                double alpha, int update, float* part, float* colsum_out, float* zgrad_out, void* stream);

/* ---- the collective of the column-sharded path ----------------------------------------------
 * One process (or host thread) per GPU, or one process driving several: the H half-step sums ONE packed fp32 buffer
 * [numerators (owner.rows_pad x r_pad) | denominators] over the ranks between nmfmu_mu_partial + nmfmu_slab_reduce and
 * nmfmu_mu_apply(..., nslab = 1); relu / eps / regularisers are applied after the sum, as on the unsharded matrix
 * (nmf.py:78-92).  RCCL is resolved at run time (dlopen): NMFMU_ERR_UNSUPPORTED when it is not installed.  RCCL errors
 * come back as 10000 + ncclResult_t.  (The Python host side of this repository uses torch.distributed, backend "nccl" =
 * RCCL, for the same exchange.) */
typedef struct nmfmu_comm nmfmu_comm;
int nmfmu_comm_available(void);                                   /* 1 when librccl could be loaded                      */
int nmfmu_comm_unique_id(void* id128);                            /* rank 0: 128 bytes to hand to every rank out of band */
int nmfmu_comm_init_rank(nmfmu_comm** comm, int nranks, const void* id128, int rank); /* current device = this rank's GPU */
int nmfmu_comm_init_all(nmfmu_comm** comms, int ndev, const int* devices);  /* one process, ndev GPUs (devices may be NULL) */
int nmfmu_comm_nranks(const nmfmu_comm* comm);
int nmfmu_comm_allreduce_sum_f32(nmfmu_comm* comm, float* buf, size_t count, void* stream);  /* in place, asynchronous */
/* one host thread driving ndev devices: the ndev all-reduces of one exchange inside ncclGroupStart / End */
int nmfmu_comm_allreduce_sum_f32_multi(nmfmu_comm* const* comms, float* const* bufs, size_t count, void* const* streams,
                                       int ndev);
int nmfmu_comm_destroy(nmfmu_comm* comm);
/* The column-sharded H half-step in one host call: nmfmu_mu_partial -> nmfmu_slab_reduce into xbuf =
 * [numerator owner_rows_pad x r_pad | beta == 1: the panel shard's column sums, r_pad floats; else the denominator,
 * owner_rows_pad x r_pad] -> ONE all-reduce of the whole buffer -> nmfmu_mu_apply(nslab = 1) -- enqueued back to back on
 * `stream`; relu / eps / regularisers are applied after the sum, as nmf.py:78-92 does on the unsharded matrix. */
int nmfmu_mu_step_allreduce(const nmfmu_step* st, nmfmu_comm* comm, float* xbuf, void* stream);

/* ---- instrumentation ------------------------------------------------------------------------------------------
 * hipEvent-based timers on the caller's stream (bench.py uses them to time the dominant kernel live). */
int nmfmu_timer_create(int n_events, void** timer);
int nmfmu_timer_record(void* timer, int idx, void* stream);
int nmfmu_timer_elapsed_ms(void* timer, int idx_from, int idx_to, float* ms); /* synchronises on idx_to */
int nmfmu_timer_destroy(void* timer);

/* ---- self-test probes (used by tests only; they validate the hardware assumptions the kernels rest on) ------ */
int nmfmu_probe_mfma(const uint16_t* a /*32x16 bf16 row-major*/, const uint16_t* b /*16x32*/, float* d /*32x32*/,
                     void* stream);
int nmfmu_probe_lds_dma(const uint32_t* src, uint32_t* dst, int n_dwords /* multiple of 1024 */, void* stream);
/* The zero-overhead ceiling of the fused MU step, measured in the run that quotes it (bench.py: roofline.ceiling_tflops):
 * every wave issues 32 MFMAs (32x32x16; f16 != 0: fp16, else bf16) per tile on fixed fragments read once from `operands`
 * (a REAL 16-bit factor image of >= 64 KiB, so that the matrix pipe sees the MU step's value distribution -- the clock the
 * power limit leaves follows the data) and streams kib_per_tile KiB (0, 1, 2, 4 or 8) per wave and tile from `stream_src`
 * by non-temporal LDS-DMA, never read back, at most three tiles in flight; no LDS reads, no VALU, no barriers.
 * kib_per_tile = 4 is the rank-128 MU step (256 flop per X byte).  grid workgroups of `waves` (4 or 8) waves, `tiles`
 * tiles each: stream_src holds grid * waves * tiles * kib_per_tile KiB, out grid * waves * 64 floats (a sink).  Flops =
 * grid * waves * tiles * 32 * 32768.  Asynchronous on `stream`; time it with events.  Not used by the product path. */
int nmfmu_ubench_mfma_hbm(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile,
                          int waves, int tiles, int grid, float* out, void* stream);
/* The same loop with its own clocks (ABI 9): `tiles` may exceed what stream_src holds -- the stream wraps after wrap_tiles
 * tiles per wave (0 = never) -- and every wave writes {shader cycles, 100 MHz ticks, start tick, end tick} of its tile loop
 * to stamps[4 * (workgroup * waves + wave) ..] (NULL = no stamps; grid * waves * 4 uint64).  The two waves of a SIMD do not
 * share the matrix pipe evenly, so the busy fraction is taken over a workgroup's span: 32 cycles x MFMAs per SIMD /
 * ((max end - min start) x clock), clock = cycles / ticks of any wave. */
int nmfmu_ubench_mfma_hbm2(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile,
                           int waves, int tiles, int wrap_tiles, int grid, float* out, uint64_t* stamps, void* stream);
/* Diagnostic hook of the ping-pong kernel (nmfmu_pp.h), live only in libraries built with -DNMFMU_DEBUG_HOOKS
 * (NMFMU_ERR_UNSUPPORTED otherwise): with a device buffer of >= (64 + 5 * workgroups) uint64 registered, every
 * workgroup records clock stamps at kernel entry, loop start, loop end and exit (tools/pp_timeline.py).  buf = NULL
 * unregisters.  Not used by the product path. */
int nmfmu_debug_set_buffer(void* buf);

#ifdef __cplusplus
}
#endif
#endif /* NMFMU_H_ */
