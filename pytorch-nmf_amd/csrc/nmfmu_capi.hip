// C ABI (include/nmfmu.h) over the HIP kernels.  Thin: argument checks, grid sizing, dispatch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/nmfmu.h"
#include "nmfmu_aux.h"
#include "nmfmu_fused.h"
#include "nmfmu_pp.h"
#include "nmfmu_sp.h"
#include "nmfmu_sp2.h"
#include "nmfmu_sp128.h"

// A/B build switches (tools/sp_bitcompare.py, pp_timeline.py, xb_timeline.py build with them); each is read in one place below
#ifndef NMFMU_SP
#define NMFMU_SP 1   // 0 = padded rank 256, beta == 1, fp16 stays on the four-wave kernel
#endif
#ifndef NMFMU_SP2
#define NMFMU_SP2 1  // 0 = padded rank 128, beta in {0, 0.5, 1.5, generic}, fp16 stays on the four-wave kernel
#endif
#ifndef NMFMU_PP_F16R
#define NMFMU_PP_F16R 1   // 0 = the 3-byte target stays on the four-wave kernel at beta == 1 as well
#endif
#ifndef NMFMU_FUSE_APPLY_TWO_ACC
#define NMFMU_FUSE_APPLY_TWO_ACC 1   // 0 = beta != 1 always goes through slabs + the apply kernel
#endif

using namespace nmfmu;

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool is_f16(int precision) {   // fp16 operand images
  return precision == NMFMU_PREC_F16 || precision == NMFMU_PREC_F16X || precision == NMFMU_PREC_F16R;
}
inline bool x_is_f32(int precision) { return precision == NMFMU_PREC_BF16X3 || precision == NMFMU_PREC_F16X; }
inline bool valid_block_rows(int block_rows) { return block_rows == 128 || block_rows == 256; }
inline int workgroups(int owner_rows_pad, int block_rows, int nsplit) { return (owner_rows_pad / block_rows) * nsplit; }
// the stages whose caller promises that nobody reads the factors' transposed images (include/nmfmu.h)
inline bool one_image_stage(int stage) {
  return stage == NMFMU_STAGE_DMA_LDSTR || stage == NMFMU_STAGE_DMA_SP128 || stage == NMFMU_STAGE_DMA_SP128_RB0;
}

// Diagnostic builds only (make EXTRA=-DNMFMU_DEBUG_HOOKS): NMFMU_FORCE_NSPLIT overrides the contraction split and
// nmfmu_debug_set_buffer registers the clock-stamp buffer of the pipelined kernels (tools/pp_timeline.py) and of the streaming
// kernel (tools/xb_timeline.py).  The product library reads no environment variable and keeps no global state.
#ifdef NMFMU_DEBUG_HOOKS
void* g_pp_debug = nullptr;
void* debug_buffer() { return g_pp_debug; }
int debug_set_buffer(void* buf) {
  g_pp_debug = buf;
  return NMFMU_OK;
}
int forced_nsplit() {   // (read once)
  static const int forced = [] { const char* v = std::getenv("NMFMU_FORCE_NSPLIT"); return v && *v ? std::atoi(v) : 0; }();
  return forced;
}
#else
void* debug_buffer() { return nullptr; }
int debug_set_buffer(void*) { return NMFMU_ERR_UNSUPPORTED; }
int forced_nsplit() { return 0; }
#endif

// Which kernel serves a dense half-step, and everything the rest of this file needs to know about that choice.
enum Kernel { kFused, kPP, kSP, kSP2, kSP128 };   // four-wave fused | eight-wave ping-pong | nmfmu_sp.h | nmfmu_sp2.h | nmfmu_sp128.h
struct Selection {
  int stage_err;   // the stage does not go with this step: refused before the step's arguments are looked at
  int err;         // no kernel serves the combination: refused after they are
  int mode;        // the mode the kernel runs in (kModeMU of a split panel: kModeMU2)
  Kernel kernel;
  bool rb0;        // kSP128: its RB = 0 schedule (A/B arm)
  bool trl;        // kPP: the instance that builds the transposed panel tile in LDS
  int group;       // the tile loop runs in groups of this many tiles: tiles_per_split is rounded up to it
  int wg_per_cu;   // workgroups a CU holds (the split rule fills the chip once)
  bool owner_p2;   // the owner's transposed image is written (false: nobody reads it, epilogue and apply kernel skip it)
};

// Pure: a function of its arguments and of which instances the kernel units hold.
Selection select_kernel(int r_pad, int precision, float beta, int block_rows, int stage, int mode, bool riding_loss) {
  const int kind = nmfmu_beta_kind(beta);
  const bool kl = kind == NMFMU_BETA_KL, f16 = precision == NMFMU_PREC_F16;
  // ping-pong kernel: beta == 1, one operand plane (bf16 or fp16; fp16 with the 3-byte target), padded rank <= 128 ...
  const bool pp = kl && r_pad <= 128 && (f16 || precision == NMFMU_PREC_BF16 || (NMFMU_PP_F16R && precision == NMFMU_PREC_F16R));
  // ... of those, the ones with the instance that builds the transposed panel tile in LDS (NMFMU_STAGE_DMA_LDSTR) ...
  const bool pp_trl = pp && pp_trl_available(r_pad, is_f16(precision) ? kOpF16 : kOpBf16, kModeMU);
  // ... and of those, the ones NMFMU_STAGE_DMA_SP128 moves to the software-pipelined kernel with 64 owner rows per wave
  const bool sp128 = pp_trl && f16 && sp128_available(r_pad, kOpF16, kModeMU);
  // one wave per SIMD, software-pipelined, fp16 operands and target: beta == 1 at padded rank 256 (configs[4]'s shard), and
  // the two-accumulator sibling for beta != 1 and != 2 at padded rank 128 (configs[2]'s beta < 1 legs)
  const bool sp = NMFMU_SP && kl && r_pad == 256 && f16;
  const bool sp2 = NMFMU_SP2 && (kind == NMFMU_BETA_IS || kind == NMFMU_BETA_GEN) && r_pad == 128 && f16;
  const bool one_image = one_image_stage(stage), sp128_stage = one_image && stage != NMFMU_STAGE_DMA_LDSTR;

  Selection s{};
  s.mode = mode, s.kernel = kFused, s.group = 1, s.wg_per_cu = block_rows == 128 ? 2 : 1;
  s.owner_p2 = !one_image && !(stage == NMFMU_STAGE_DMA_NOP2 && sp);
  if (stage != NMFMU_STAGE_DMA && stage != NMFMU_STAGE_DMA_SPLIT && stage != NMFMU_STAGE_DMA_NOP2 && !one_image) {
    s.stage_err = NMFMU_ERR_UNSUPPORTED;   // (register staging: no longer built)
  } else if (one_image && mode != kModeLoss && (mode != kModeMU || block_rows != 256 || !pp_trl)) {
    s.stage_err = NMFMU_ERR_UNSUPPORTED;   // one panel image: the ping-pong kernel's MU half-step only (the loss reads p1 alone anyway)
  } else if (sp128_stage && !sp128) {
    s.stage_err = NMFMU_ERR_UNSUPPORTED;
  } else if (stage == NMFMU_STAGE_DMA_SPLIT && mode == kModeMU && precision != NMFMU_PREC_BF16X3) {
    // split panel (PLCA: p1 = the Z-scaled factor, p2 = the unscaled one): the instantiation that stages BOTH images
    if (kl && block_rows == 128) s.mode = kModeMU2;
    else s.stage_err = NMFMU_ERR_UNSUPPORTED;
  }
  if (block_rows == 256) {   // the eight-wave ping-pong kernel; both half-steps (the apply is fused there as well)
    if (mode == kModeDen || !pp) s.err = NMFMU_ERR_UNSUPPORTED;
    s.kernel = kPP, s.group = 2;   // its tile loop is unrolled by two
    s.trl = one_image && mode != kModeLoss;
    if (sp128_stage && mode == kModeMU && !riding_loss) {   // (the loss-carrying half-step stays on the ping-pong kernel)
      s.kernel = kSP128, s.group = 4, s.rb0 = stage == NMFMU_STAGE_DMA_SP128_RB0;   // ring slot = tile & 3
    }
  } else if (s.mode == kModeMU && (sp || sp2)) {
    s.kernel = sp ? kSP : kSP2, s.group = 4, s.wg_per_cu = 1;   // ring slot = tile & 3; one 512-register workgroup per CU
  } else if (r_pad != 32 && r_pad != 64 && r_pad != 128 && r_pad != 256) {
    s.err = NMFMU_ERR_UNSUPPORTED;
  }
  return s;
}

// The apply kernel's side of the one-image promise (see nmfmu.h): NMFMU_OK, or the code a one-image stage is refused with on
// a step whose half-step could not keep it; *writes_p2: the owner's transposed images are written.  The apply kernel serves
// every one-image stage alike, so the question is put for NMFMU_STAGE_DMA_LDSTR, not for the half-step's own kernel.
int apply_image_rule(const nmfmu_step* st, bool* writes_p2) {
  const bool one_image = one_image_stage(st->stage);
  const Selection sel = select_kernel(st->r_pad, st->precision, st->beta, st->block_rows,
                                      one_image ? NMFMU_STAGE_DMA_LDSTR : st->stage, kModeMU, false);
  *writes_p2 = sel.owner_p2;
  return one_image ? sel.stage_err : NMFMU_OK;
}

// beta -> kernel branch (nmfmu_fused.h: BetaKind): the public kinds plus the two rsqrt special cases of the generic one
int kernel_beta_kind(float beta) {
  if (beta == 0.5f) return kSqrt;
  if (beta == 1.5f) return kSqrt3;
  return nmfmu_beta_kind(beta);
}

// "The workgroup owns whole rows": unsplit contraction, so a kernel that can may apply the update in its epilogue.
// outputs: the caller also gave everything that epilogue writes (nmfmu_colsum_nparts asks about the split alone)
bool owns_whole_rows(const nmfmu_step* st, bool outputs) {
  return st->nsplit == 1 && (!outputs || (st->owner.f && st->owner.p2_hi && st->owner.colsum && st->owner.colsum_part));
}

struct GramRef {   // Gram matrix of the panel (nmfmu_gram_panel): its 16-bit images with per-row scales
  const void* hi;
  const void* lo;
  const float* scale;
};

int fused_dispatch(const nmfmu_step* st, int mode, float* loss_part, int M, int K, hipStream_t s,
                   const float* fuse_kl_den = nullptr, bool fuse_apply = false, const GramRef* gm = nullptr) {
  if (!st || !st->owner.p1_hi || !st->panel.p1_hi) return NMFMU_ERR_ARG;
  if (!st->xp && (mode == kModeMU || mode == kModeXB)) return NMFMU_ERR_ARG;   // (the denominator-only pass and the loss may run without a target)
  if (st->owner.rows_pad % kRowPad || st->panel.rows_pad % kRowPad) return NMFMU_ERR_ARG;
  if (!valid_block_rows(st->block_rows)) return NMFMU_ERR_ARG;
  const Selection sel = select_kernel(st->r_pad, st->precision, st->beta, st->block_rows, st->stage, mode,
                                      /*riding loss*/ mode == kModeMU && loss_part != nullptr);
  if (sel.stage_err) return sel.stage_err;
  mode = sel.mode;
  if (st->r_pad != pad_rank(st->rank) || st->nsplit < 1) return NMFMU_ERR_ARG;
  const bool x3 = st->precision == NMFMU_PREC_BF16X3;
  if (x3 && (!st->owner.p1_lo || !st->panel.p1_lo)) return NMFMU_ERR_ARG;
  const int kind = nmfmu_beta_kind(st->beta);
  if (st->precision == NMFMU_PREC_F16R && kind == NMFMU_BETA_EUC) return NMFMU_ERR_UNSUPPORTED;   // the target is an operand there: F16X
  FusedArgs a{};
  a.xp = st->xp;
  a.p1_hi = static_cast<const uint16_t*>(st->panel.p1_hi), a.p1_lo = static_cast<const uint16_t*>(st->panel.p1_lo);
  a.p2_hi = static_cast<const uint16_t*>(st->panel.p2_hi), a.p2_lo = static_cast<const uint16_t*>(st->panel.p2_lo);
  a.a1_hi = static_cast<const uint16_t*>(st->owner.p1_hi), a.a1_lo = static_cast<const uint16_t*>(st->owner.p1_lo);
  a.slab_num = st->slab_num, a.slab_den = st->slab_den, a.loss_part = loss_part;
  a.M = M, a.K = K, a.M_pad = st->owner.rows_pad;
  a.ktiles = st->panel.rows_pad / kBK, a.nsplit = st->nsplit;
  a.tiles_per_split = ((a.ktiles + st->nsplit - 1) / st->nsplit + sel.group - 1) / sel.group * sel.group;
  a.beta = st->beta;
  a.status = st->status;
  a.cs_owner = st->owner.colsum;   // fp16 operands, beta < 1: typical S -> scale of Gn / Gp (nmfmu_fused.h)
  a.cs_panel = st->panel.colsum;
  if (fuse_apply) {  // nsplit == 1: apply in the epilogue
    a.fuse_apply = 1;
    a.rank = st->rank;
    a.f = st->owner.f;
    a.kl_den = fuse_kl_den;
    a.o1_hi = static_cast<uint16_t*>(st->owner.p1_hi), a.o1_lo = static_cast<uint16_t*>(st->owner.p1_lo);
    a.o2_hi = sel.owner_p2 ? static_cast<uint16_t*>(st->owner.p2_hi) : nullptr, a.o2_lo = static_cast<uint16_t*>(st->owner.p2_lo);
    a.colsum_part = st->owner.colsum_part;
    a.l1 = st->l1, a.l2 = st->l2, a.gamma = st->gamma;
  }
  if (mode == kModeMU2) {
    if (!a.slab_num || !a.p2_hi || fuse_apply) return NMFMU_ERR_ARG;
  } else if (mode == kModeXB) {   // beta == 2 without reconstruction: numerator slabs only (or the fused apply with the Gram images)
    if (kind != kEuc || x3 || st->block_rows != 128) return NMFMU_ERR_UNSUPPORTED;
    if (!a.p2_hi || (!fuse_apply && !a.slab_num)) return NMFMU_ERR_ARG;
    if (fuse_apply && (!gm || st->r_pad > 128)) return NMFMU_ERR_ARG;
    if (gm) {   // denominator in the kernel: fused apply, or ONE denominator slab, its rank tiles shared out over the row block's first workgroups
      if (!gm->hi || !gm->lo || !gm->scale || (!fuse_apply && !a.slab_den)) return NMFMU_ERR_ARG;
      a.gram_hi = static_cast<const uint16_t*>(gm->hi), a.gram_lo = static_cast<const uint16_t*>(gm->lo);
      a.gram_scale = gm->scale;
    } else {
      a.slab_den = nullptr;   // numerator slabs only (nmfmu_xb_partial)
    }
  } else if (mode == kModeMU || mode == kModeDen) {
    if (!a.slab_num || !a.p2_hi || (x3 && !a.p2_lo)) return NMFMU_ERR_ARG;
    if (mode == kModeMU && kind != kKL && !a.slab_den) return NMFMU_ERR_ARG;
    if (mode == kModeDen && (kind != kGen || st->block_rows != 128)) return NMFMU_ERR_UNSUPPORTED;
  } else if (!loss_part) {
    return NMFMU_ERR_ARG;
  }
  if (sel.err || (sel.kernel == kPP && !st->xp)) return NMFMU_ERR_UNSUPPORTED;   // (the ping-pong kernel's loss pass needs the target)
  const int grid = workgroups(st->owner.rows_pad, st->block_rows, st->nsplit);
  // clock stamps (nmfmu_step.stamps) of the pipelined kernels' MU half-step; diagnostic builds: the registered buffer there
  // and on the streaming kernel
  const bool stamped = mode == kModeMU && (sel.kernel == kPP || sel.kernel == kSP128 || sel.kernel == kSP);
  a.debug = stamped ? st->stamps : nullptr;
  if (debug_buffer() && (stamped || (sel.kernel == kFused && mode == kModeXB))) a.debug = debug_buffer();
  const int opt = is_f16(st->precision) ? kOpF16 : kOpBf16, kk = kernel_beta_kind(st->beta);
  switch (sel.kernel) {
    case kSP128: return sel.rb0 ? launch_sp128_rb0(st->r_pad, kOpF16, a, grid, s) : launch_sp128(st->r_pad, kOpF16, a, grid, s);
    case kPP:
      return launch_pp(st->r_pad, opt, mode, a, grid, s, st->precision == NMFMU_PREC_F16R,
                       /*riding loss*/ mode == kModeMU && loss_part != nullptr, sel.trl);
    case kSP: return launch_sp(st->r_pad, kOpF16, a, grid, s);
    case kSP2: return launch_sp2(st->r_pad, kk, a, grid, s);
    case kFused: break;
  }
  switch (st->r_pad) {
    case 32: return launch_fused_r32(kk, st->precision, mode, a, grid, s);
    case 64: return launch_fused_r64(kk, st->precision, mode, a, grid, s);
    case 128: return launch_fused_r128(kk, st->precision, mode, a, grid, s);
    default: return launch_fused_r256(kk, st->precision, mode, a, grid, s);
  }
}

struct Timer {
  std::vector<hipEvent_t> ev;
};

}  // namespace

// (nmfmu_aux.h) apply_image_rule for the apply stages that live in other units (nmfmu_ard.hip)
int nmfmu::apply_writes_p2(const nmfmu_step* st, bool* writes_p2) { return apply_image_rule(st, writes_p2); }

extern "C" {

int nmfmu_abi_version(void) { return NMFMU_ABI_VERSION; }
int nmfmu_abi_check(int compiled_against) { return compiled_against == NMFMU_ABI_VERSION ? NMFMU_OK : NMFMU_ERR_ARG; }
int nmfmu_pad_rows(int rows) { return rows <= 0 ? NMFMU_ERR_ARG : pad_rows(rows); }
int nmfmu_pad_rank(int rank) {
  const int r = pad_rank(rank);
  return r < 0 ? NMFMU_ERR_UNSUPPORTED : r;
}
int nmfmu_beta_kind(float beta) {
  if (beta == 1.f) return NMFMU_BETA_KL;
  if (beta == 2.f) return NMFMU_BETA_EUC;
  if (beta == 0.f) return NMFMU_BETA_IS;
  return NMFMU_BETA_GEN;
}
int nmfmu_supported(int r_pad, int precision) {
  if (r_pad != 32 && r_pad != 64 && r_pad != 128 && r_pad != 256) return 0;
  if (precision == NMFMU_PREC_BF16) return 1;
  if (precision == NMFMU_PREC_BF16X3) return r_pad <= 128;  // 4 image planes x 2 stages must fit 160 KiB of LDS
  if (precision == NMFMU_PREC_F16) return 1;                // ping-pong kernel (beta == 1, r_pad <= 128), else four-wave
  if (precision == NMFMU_PREC_F16X) return 1;               // four-wave kernel: fp16 operands, fp32 target
  if (precision == NMFMU_PREC_F16R) return 1;               // as F16 with a 3-byte target (beta != 2): ping-pong / four-wave kernel
  return 0;
}

int nmfmu_block_rows(int r_pad, int precision, float beta) {
  // 256-row tiles where the eight-wave ping-pong kernel serves the MU half-step (beta == 1, one operand plane, padded rank
  // <= 128).  Everything else: 128-row tiles (the four-wave kernels; two workgroups per CU where the registers allow).
  return select_kernel(r_pad, precision, beta, 256, NMFMU_STAGE_DMA, kModeMU, false).err ? 128 : 256;
}

int nmfmu_step_block_rows(int owner_rows_pad, int panel_rows_pad, int r_pad, int precision, float beta, int num_cu) {
  (void)num_cu;
  const int block_rows = nmfmu_block_rows(r_pad, precision, beta);
  if (block_rows == 128 && (owner_rows_pad <= 0 || panel_rows_pad <= 0)) return NMFMU_ERR_ARG;   // (not looked at for the ping-pong kernel)
  return block_rows;
}

int nmfmu_kernel_family(int r_pad, int precision, float beta) {
  const Kernel k = select_kernel(r_pad, precision, beta, nmfmu_block_rows(r_pad, precision, beta), NMFMU_STAGE_DMA, kModeMU, false).kernel;
  return k == kPP ? NMFMU_KERNEL_PP : (k == kSP || k == kSP2) ? NMFMU_KERNEL_SP : NMFMU_KERNEL_FUSED;
}

int nmfmu_pp_lds_transpose_supported(int r_pad, int precision, float beta) {
  return select_kernel(r_pad, precision, beta, 256, NMFMU_STAGE_DMA_LDSTR, kModeMU, false).stage_err ? 0 : 1;
}

// The split rule.  wg_per_cu == 2 (four-wave kernel on 128-row tiles: both wave slots of every SIMD) or 1 (256-row tiles);
// pipelined: a one-wave-per-SIMD kernel, one 512-register workgroup per CU -- as many splits as fill the chip ONCE (whole
// rounds when the row blocks alone exceed it), each at least two groups of four tiles
static int split_rule(int owner_rows_pad, int panel_rows_pad, int block_rows, int num_cu, int wg_per_cu, bool pipelined) {
  if (owner_rows_pad <= 0 || panel_rows_pad <= 0 || !valid_block_rows(block_rows)) return NMFMU_ERR_ARG;
  const int mblocks = owner_rows_pad / block_rows, ktiles = panel_rows_pad / kBK;
  if (const int forced = pipelined ? 0 : forced_nsplit(); forced > 0) return std::min(forced, std::max(1, ktiles));
  int ns = (wg_per_cu * std::max(num_cu, 1) + mblocks - 1) / mblocks;
  if (ns > 8 && !pipelined) ns = (ns + 7) / 8 * 8;   // same-chunk workgroups then share an XCD (block b runs on XCD b % 8)
  ns = std::min(ns, std::max(1, ktiles / (pipelined ? 8 : 4)));   // at least 4 tiles per workgroup to amortise prologue/epilogue
  return std::max(ns, 1);
}

int nmfmu_choose_nsplit(int owner_rows_pad, int panel_rows_pad, int block_rows, int num_cu) {
  return split_rule(owner_rows_pad, panel_rows_pad, block_rows, num_cu, block_rows == 128 ? 2 : 1, false);
}

int nmfmu_choose_nsplit_for(int owner_rows_pad, int panel_rows_pad, int r_pad, int precision, float beta, int block_rows, int num_cu) {
  const Selection sel = select_kernel(r_pad, precision, beta, block_rows, NMFMU_STAGE_DMA, kModeMU, false);
  return split_rule(owner_rows_pad, panel_rows_pad, block_rows, num_cu, sel.wg_per_cu, sel.kernel == kSP || sel.kernel == kSP2);
}

size_t nmfmu_xp_bytes(int owner_rows_pad, int panel_rows_pad, int precision) {
  return (size_t)owner_rows_pad * (size_t)panel_rows_pad * (x_is_f32(precision) ? 4 : (precision == NMFMU_PREC_F16R ? 3 : 2));
}
size_t nmfmu_image_bytes(int rows_pad, int r_pad) { return (size_t)rows_pad * (size_t)r_pad * 2; }
size_t nmfmu_slab_bytes(int owner_rows_pad, int r_pad, int nsplit) {
  return (size_t)nsplit * (size_t)owner_rows_pad * (size_t)r_pad * 4;
}
size_t nmfmu_colsum_part_bytes(int rows_pad, int r_pad) { return (size_t)(rows_pad / 16) * (size_t)r_pad * 4; }

int nmfmu_pack_x(const float* v, int64_t ld, int rows, int cols, int transpose, int precision, int block_rows, void* xp,
                 int owner_rows_pad, int panel_rows_pad, uint32_t* flags, void* stream) {
  if (!v || !xp || rows <= 0 || cols <= 0 || !valid_block_rows(block_rows)) return NMFMU_ERR_ARG;
  const int m = transpose ? cols : rows, k = transpose ? rows : cols;
  if (owner_rows_pad != pad_rows(m) || panel_rows_pad != pad_rows(k)) return NMFMU_ERR_ARG;
  const int fmt = x_is_f32(precision) ? 1 : (precision == NMFMU_PREC_F16 ? 2 : (precision == NMFMU_PREC_F16R ? 3 : 0));
  return launch_pack_x(v, ld, rows, cols, transpose != 0, fmt, xp, owner_rows_pad, panel_rows_pad, flags,
                       block_rows / 128, S(stream));
}

static int pack_factor_common(const nmfmu_factor* fac, int rank, int r_pad, int precision, const float* scale,
                              void* stream) {
  if (!fac || !fac->f || !fac->p1_hi || !fac->p2_hi || !fac->colsum || !fac->colsum_part) return NMFMU_ERR_ARG;
  if (r_pad != pad_rank(rank) || fac->rows_pad != pad_rows(fac->rows)) return NMFMU_ERR_ARG;
  const bool x3 = precision == NMFMU_PREC_BF16X3;
  if (x3 && (!fac->p1_lo || !fac->p2_lo)) return NMFMU_ERR_ARG;
  ApplyArgs a{};
  a.f = fac->f;
  a.p1_hi = fac->p1_hi, a.p1_lo = fac->p1_lo, a.p2_hi = fac->p2_hi, a.p2_lo = fac->p2_lo;
  a.colsum_part = fac->colsum_part, a.colsum = fac->colsum;
  a.rows = fac->rows, a.rank = rank, a.rows_pad = fac->rows_pad;
  a.gamma = 1.f;
  a.scale = scale;
  a.skip_colsum = scale != nullptr;   // the scaled packing serves PLCA's EM, which reads no column sums of the images' factor
  a.f16 = is_f16(precision);
  return launch_apply(r_pad, a, x3, /*pack_only=*/true, S(stream));
}

int nmfmu_pack_factor(const nmfmu_factor* fac, int rank, int r_pad, int precision, void* stream) {
  return pack_factor_common(fac, rank, r_pad, precision, nullptr, stream);
}

int nmfmu_pack_factor_scaled(const nmfmu_factor* fac, int rank, int r_pad, int precision, const float* scale,
                             void* stream) {
  if (!scale) return NMFMU_ERR_ARG;
  return pack_factor_common(fac, rank, r_pad, precision, scale, stream);
}

static int partial_sums(const nmfmu_step* st, int mode, void* stream) {
  if (!st) return NMFMU_ERR_ARG;
  if (!nmfmu_supported(st->r_pad, st->precision)) return NMFMU_ERR_UNSUPPORTED;
  return fused_dispatch(st, mode, nullptr, st->owner.rows, st->panel.rows, S(stream));
}
int nmfmu_mu_partial(const nmfmu_step* st, void* stream) { return partial_sums(st, kModeMU, stream); }
int nmfmu_den_partial(const nmfmu_step* st, void* stream) { return partial_sums(st, kModeDen, stream); }

// A complete MU half-step (phase 0), its fused launch alone (1) or what follows that launch (2).  xlogs_part: the launch is
// the kernel instance that also accumulates the riding loss
static int mu_step_common(const nmfmu_step* st, const float* kl_den, int phase, float* xlogs_part, void* stream) {
  const bool kl = nmfmu_beta_kind(st->beta) == NMFMU_BETA_KL;
  // apply in the fused kernel's epilogue (nmf.py:78-92) when the workgroup owns whole rows: beta == 1 (closed-form denominators)
  // on both kernels, beta != 1 (two accumulator sets) on the four-wave kernel in the single-plane precisions up to rank pad 128
  const bool fuse = owns_whole_rows(st, true) && (kl || (NMFMU_FUSE_APPLY_TWO_ACC && st->precision != NMFMU_PREC_BF16X3 && st->r_pad <= 128));
  int e = 0;
  if (phase != 2) e = fused_dispatch(st, kModeMU, xlogs_part, st->owner.rows, st->panel.rows, S(stream), kl_den, fuse);
  if (e || phase == 1) return e;
  // what is left: the column-sum finalize, or the whole apply
  return fuse ? launch_colsum_finalize(st->owner.colsum_part, workgroups(st->owner.rows_pad, st->block_rows, 1), st->r_pad,
                                       st->owner.colsum, S(stream))
              : nmfmu_mu_apply(st, nullptr, nullptr, 0, kl ? kl_den : nullptr, stream);
}

int nmfmu_mu_step(const nmfmu_step* st, const float* kl_den, int phase, void* stream) {
  if (!st || phase < 0 || phase > 2) return NMFMU_ERR_ARG;
  if (!nmfmu_supported(st->r_pad, st->precision)) return NMFMU_ERR_UNSUPPORTED;
  // (a split panel -- images of two different matrices -- belongs to nmfmu_mu_partial: PLCA's EM reads the slabs; a complete
  // MU half-step of ONE panel matrix has nothing to split, and the fused-apply epilogue stages p1 only)
  if (st->stage == NMFMU_STAGE_DMA_SPLIT) return NMFMU_ERR_ARG;
  if (nmfmu_beta_kind(st->beta) == NMFMU_BETA_KL && !kl_den) return NMFMU_ERR_ARG;
  return mu_step_common(st, kl_den, phase, nullptr, stream);
}

int nmfmu_colsum_nparts(const nmfmu_step* st) {
  if (!st || !valid_block_rows(st->block_rows)) return NMFMU_ERR_ARG;
  // fused apply: one partial per workgroup tile; otherwise one per apply-kernel stripe
  return owns_whole_rows(st, false) ? workgroups(st->owner.rows_pad, st->block_rows, 1) : st->owner.rows_pad / apply_stripe_rows(st->owner.rows_pad);
}

int nmfmu_pack_nparts(int rows_pad) { return rows_pad <= 0 ? NMFMU_ERR_ARG : rows_pad / apply_stripe_rows(rows_pad); }

int nmfmu_colsum_finalize(const nmfmu_factor* fac, int nparts, int r_pad, void* stream) {
  if (!fac || !fac->colsum || !fac->colsum_part || nparts <= 0) return NMFMU_ERR_ARG;
  return launch_colsum_finalize(fac->colsum_part, nparts, r_pad, fac->colsum, S(stream));
}

int nmfmu_slab_reduce(const nmfmu_step* st, float* num_out, float* den_out, void* stream) {
  if (!st || !num_out || !st->slab_num) return NMFMU_ERR_ARG;
  const int64_t plane = (int64_t)st->owner.rows_pad * st->r_pad;
  int e = launch_slab_reduce(st->slab_num, st->nsplit, plane, num_out, S(stream));
  if (e) return e;
  if (den_out) {
    if (!st->slab_den) return NMFMU_ERR_ARG;
    e = launch_slab_reduce(st->slab_den, st->nsplit, plane, den_out, S(stream));
  }
  return e;
}

static int apply_common(const nmfmu_step* st, const float* num, const float* den, int nslab, const float* kl_den,
                        int trainer, float ortho, float* grad, void* stream, int den_nslab = 0, int skip_colsum = 0) {
  if (!st || !st->owner.f) return NMFMU_ERR_ARG;
  const bool kl = nmfmu_beta_kind(st->beta) == NMFMU_BETA_KL;
  ApplyArgs a{};
  a.f = st->owner.f;
  a.num = num ? num : st->slab_num;
  a.den = num ? den : st->slab_den;
  a.nslab = num ? nslab : st->nsplit;
  a.kl_den = kl ? kl_den : nullptr;
  if (!a.num || a.nslab < 1) return NMFMU_ERR_ARG;
  a.den_nslab = den_nslab;
  a.skip_colsum = skip_colsum;
  if (kl ? !a.kl_den : !a.den) return NMFMU_ERR_ARG;
  a.p1_hi = st->owner.p1_hi, a.p1_lo = st->owner.p1_lo, a.p2_hi = st->owner.p2_hi, a.p2_lo = st->owner.p2_lo;
  a.colsum_part = st->owner.colsum_part, a.colsum = st->owner.colsum;
  a.rows = st->owner.rows, a.rank = st->rank, a.rows_pad = st->owner.rows_pad;
  a.l1 = st->l1, a.l2 = st->l2, a.gamma = st->gamma;
  a.trainer = trainer, a.ortho = ortho, a.grad = grad;
  a.f16 = is_f16(st->precision);
  a.status = st->status;
  if (!a.p1_hi || !a.p2_hi || !a.colsum || !a.colsum_part) return NMFMU_ERR_ARG;
  bool writes_p2 = true;
  if (const int e = apply_image_rule(st, &writes_p2)) return e;
  if (!writes_p2) a.p2_hi = a.p2_lo = nullptr;   // nobody reads the transposed images where the stage promises so
  return launch_apply(st->r_pad, a, st->precision == NMFMU_PREC_BF16X3, /*pack_only=*/false, S(stream));
}

int nmfmu_mu_apply(const nmfmu_step* st, const float* num, const float* den, int nslab, const float* kl_den, void* stream) {
  return apply_common(st, num, den, nslab, kl_den, 0, 0.f, nullptr, stream);
}

int nmfmu_trainer_apply(const nmfmu_step* st, const float* num, const float* den, int nslab, const float* kl_den,
                        float ortho, float* grad, void* stream) {
  if (!(ortho >= 0.f)) return NMFMU_ERR_ARG;
  return apply_common(st, num, den, nslab, kl_den, 1, ortho, grad, stream);
}

int nmfmu_xb_supported(int r_pad, int precision, float beta) {
  if (nmfmu_beta_kind(beta) != NMFMU_BETA_EUC) return 0;
  if (r_pad != 32 && r_pad != 64 && r_pad != 128 && r_pad != 256) return 0;
  if (precision == NMFMU_PREC_F16X) return r_pad <= 128;   // (three fp32 X buffers + rank-256 accumulators: no registers)
  return precision == NMFMU_PREC_BF16 || precision == NMFMU_PREC_F16;
}

int nmfmu_xb_partial(const nmfmu_step* st, void* stream) {
  if (!st) return NMFMU_ERR_ARG;
  if (!nmfmu_xb_supported(st->r_pad, st->precision, st->beta)) return NMFMU_ERR_UNSUPPORTED;
  return fused_dispatch(st, kModeXB, nullptr, st->owner.rows, st->panel.rows, S(stream));
}

int nmfmu_xb_step(const nmfmu_step* st, const void* g_hi, const void* g_lo, const float* g_scale, int phase, void* stream) {
  if (!st || !g_hi || !g_lo || !g_scale || phase < 0 || phase > 2) return NMFMU_ERR_ARG;
  if (!nmfmu_xb_supported(st->r_pad, st->precision, st->beta)) return NMFMU_ERR_UNSUPPORTED;
  // the workgroup owns whole rows (unsplit contraction): numerator, denominator (owner fragments x Gram image) and
  // nmf.py:78-92 in the kernel's epilogue; otherwise nsplit numerator slabs + ONE denominator slab (written by the first
  // min(nsplit, r_pad / 32) workgroups of every row block, one 32-rank tile each, the same MFMA product) + the apply kernel
  const bool fuse = owns_whole_rows(st, true) && st->r_pad <= 128;
  if (!fuse && !st->slab_den) return NMFMU_ERR_ARG;
  const GramRef gm{g_hi, g_lo, g_scale};
  int e = 0;
  if (phase != 2) e = fused_dispatch(st, kModeXB, nullptr, st->owner.rows, st->panel.rows, S(stream), nullptr, fuse, &gm);
  if (e || phase == 1 || fuse) return e;
  // (no column-sum finalize on this path: beta == 2 reads neither the closed-form denominators nor the fp16 scale)
  return apply_common(st, nullptr, nullptr, 0, nullptr, 0, 0.f, nullptr, stream, /*den_nslab=*/1, /*skip_colsum=*/1);
}

int nmfmu_mu_step_allreduce(const nmfmu_step* st, nmfmu_comm* comm, float* xbuf, void* stream) {
  // The column-sharded H half-step of SURVEY 8(e) as ONE host call: partial sums -> slab reduction into the packed buffer
  // [numerator M_pad x R_PAD | panel column sums R_PAD (beta == 1) or denominator M_pad x R_PAD] -> ONE RCCL all-reduce
  // -> apply -- all enqueued back to back on the caller's stream, so the host never returns to its interpreter between
  // the kernel and the collective (the torch.distributed route costs a Python / c10d round trip and two stream hops there).
  if (!st || !comm || !xbuf) return NMFMU_ERR_ARG;
  const bool kl = nmfmu_beta_kind(st->beta) == NMFMU_BETA_KL;
  const size_t plane = (size_t)st->owner.rows_pad * st->r_pad;
  const size_t tail = kl ? (size_t)st->r_pad : plane;
  if (kl && !st->panel.colsum) return NMFMU_ERR_ARG;
  int e = nmfmu_mu_partial(st, stream);
  if (e) return e;
  e = nmfmu_slab_reduce(st, xbuf, kl ? nullptr : xbuf + plane, stream);
  if (e) return e;
  if (kl) {
    hipError_t he = hipMemcpyAsync(xbuf + plane, st->panel.colsum, st->r_pad * sizeof(float), hipMemcpyDeviceToDevice, S(stream));
    if (he != hipSuccess) return (int)he;
  }
  e = nmfmu_comm_allreduce_sum_f32(comm, xbuf, plane + tail, stream);
  if (e) return e;
  return nmfmu_mu_apply(st, xbuf, kl ? nullptr : xbuf + plane, 1, kl ? xbuf + plane : nullptr, stream);
}

int nmfmu_loss_part_count(int owner_rows_pad, int block_rows, int nsplit) {
  return valid_block_rows(block_rows) ? workgroups(owner_rows_pad, block_rows, nsplit) : NMFMU_ERR_ARG;
}

int nmfmu_loss(const nmfmu_step* st, float* loss_part, double* out, void* stream) {
  if (!st || !out) return NMFMU_ERR_ARG;
  if (!nmfmu_supported(st->r_pad, st->precision)) return NMFMU_ERR_UNSUPPORTED;
  int e = fused_dispatch(st, kModeLoss, loss_part, st->owner.rows, st->panel.rows, S(stream));
  if (e) return e;
  return launch_sum_finalize_f32(loss_part, workgroups(st->owner.rows_pad, st->block_rows, st->nsplit), out, S(stream));
}

int nmfmu_loss_checkpoint(const nmfmu_step* st, float* loss_part, double* out2, const float* fa, float* fa_snap, int64_t na,
                          const float* fb, float* fb_snap, int64_t nb, void* stream) {
  if (!st || !loss_part || !out2 || !fa || !fa_snap || !fb || !fb_snap || na < 0 || nb < 0 || (na & 3) || (nb & 3)) return NMFMU_ERR_ARG;
  if (!nmfmu_supported(st->r_pad, st->precision)) return NMFMU_ERR_UNSUPPORTED;
  int e = fused_dispatch(st, kModeLoss, loss_part, st->owner.rows, st->panel.rows, S(stream));
  if (e) return e;
  return launch_checkpoint(loss_part, workgroups(st->owner.rows_pad, st->block_rows, st->nsplit), st->status, out2, fa, fa_snap, na, fb,
                           fb_snap, nb, S(stream));
}

int nmfmu_riding_loss_supported(const nmfmu_step* st) {
  // the half-steps whose kernel can carry the loss term: beta == 1 on the ping-pong kernel with fp16 operands (either target
  // width); unsplit contraction (fused apply) or split (partial sums + apply kernel) alike
  if (!st || !st->xp || !is_f16(st->precision)) return 0;
  const Selection sel = select_kernel(st->r_pad, st->precision, st->beta, st->block_rows, st->stage, kModeMU, true);
  if (sel.kernel != kPP || sel.err || st->stage == NMFMU_STAGE_DMA_SPLIT || st->nsplit < 1 || !st->slab_num) return 0;
  return st->owner.f && st->owner.colsum ? 1 : 0;
}
int nmfmu_riding_loss_part_count(const nmfmu_step* st) {
  return nmfmu_riding_loss_supported(st) ? 16 * workgroups(st->owner.rows_pad, st->block_rows, st->nsplit) : NMFMU_ERR_UNSUPPORTED;
}
int nmfmu_target_sums_nparts(void) { return 1024; }
int nmfmu_target_sums(const float* v, int64_t ld, int rows, int cols, double* part, double* out4, void* stream) {
  if (!v || !part || !out4 || rows <= 0 || cols <= 0 || ld < cols) return NMFMU_ERR_ARG;
  return launch_target_sums(v, ld, rows, cols, part, nmfmu_target_sums_nparts(), out4, S(stream));
}
int nmfmu_mu_step_with_loss(const nmfmu_step* st, const float* kl_den, float* xlogs_part, const double* target_sums,
                            double* out2, void* stream) {
  if (!st || !kl_den || !xlogs_part || !target_sums || !out2) return NMFMU_ERR_ARG;
  if (!nmfmu_riding_loss_supported(st)) return NMFMU_ERR_UNSUPPORTED;
  const int e = mu_step_common(st, kl_den, 0, xlogs_part, stream);
  if (e) return e;
  return launch_riding_finish(xlogs_part, nmfmu_riding_loss_part_count(st) / 2, target_sums,
                              (double)st->owner.rows_pad * (double)st->panel.rows_pad, st->status, out2, S(stream));
}

int nmfmu_beta_div(const float* x, const float* y, int64_t n, float beta, double* part, double* out, void* stream) {
  if (!x || !y || !part || !out || n < 0) return NMFMU_ERR_ARG;
  return launch_beta_div(x, y, n, beta, nmfmu_beta_kind(beta), part, out, S(stream));
}

int nmfmu_mu_terms(const float* s, const float* v, int64_t n, float beta, float* gn, float* gp, void* stream) {
  if (!s || !v || !gn || !gp || n <= 0) return NMFMU_ERR_ARG;
  return launch_mu_terms(s, v, n, beta, nmfmu_beta_kind(beta), gn, gp, S(stream));
}

int nmfmu_trainer_update(float* f, int rows, int cols, const float* neg, const float* pos, float l1, float l2, float ortho,
                         float gamma, float* grad, void* stream) {
  if (!f || !neg || !pos || rows <= 0 || cols <= 0 || !(ortho >= 0.f)) return NMFMU_ERR_ARG;
  return launch_trainer_update(f, rows, cols, neg, pos, l1, l2, ortho, gamma, grad, S(stream));
}

int nmfmu_norms(const float* x, int64_t n, double* part, double* out, void* stream) {
  if (!x || !part || !out || n <= 0) return NMFMU_ERR_ARG;
  return launch_norms(x, n, part, out, S(stream));
}

int nmfmu_reconstruct(const float* owner, int m, const float* panel, int k, int rank, float* out, int64_t ld,
                      void* stream) {
  if (!owner || !panel || !out || m <= 0 || k <= 0 || rank <= 0 || ld < k) return NMFMU_ERR_ARG;
  return launch_reconstruct(owner, m, panel, k, rank, out, ld, S(stream));
}

int64_t nmfmu_reconstruct_backward_ws(int m, int k, int rank, int want_owner, int want_panel, int* splits) {
  if (m <= 0 || k <= 0 || rank <= 0) return NMFMU_ERR_ARG;
  return backward_ws_floats(m, k, rank, want_owner != 0, want_panel != 0, splits);
}

int nmfmu_reconstruct_backward(const float* g, int64_t ld, int m, int k, const float* owner, const float* panel, int rank,
                               float* grad_owner, float* grad_panel, float* ws, void* stream) {
  if (!g || m <= 0 || k <= 0 || rank <= 0 || ld < k) return NMFMU_ERR_ARG;
  if ((grad_owner && !panel) || (grad_panel && !owner)) return NMFMU_ERR_ARG;
  if (!ws && backward_ws_floats(m, k, rank, grad_owner != nullptr, grad_panel != nullptr, nullptr) > 0) return NMFMU_ERR_ARG;
  return launch_reconstruct_backward(g, ld, m, k, owner, panel, rank, grad_owner, grad_panel, ws, S(stream));
}

int64_t nmfmu_conv_backward_ws(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps, int want_h,
                               int want_w, int* splits) {
  const int64_t n = conv_backward_ws_floats(batch, channels, rank, ndim, lh, taps, want_h != 0, want_w != 0, splits);
  return n < 0 ? NMFMU_ERR_ARG : n;
}

int nmfmu_conv_backward(const float* g, const float* w, const float* h, int batch, int channels, int rank, int ndim,
                        const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* ws, void* stream) {
  if (!g || (!grad_h && !grad_w) || (grad_h && !w) || (grad_w && !h)) return NMFMU_ERR_ARG;
  const int64_t n = conv_backward_ws_floats(batch, channels, rank, ndim, lh, taps, grad_h != nullptr, grad_w != nullptr, nullptr);
  if (n < 0 || (n > 0 && !ws)) return NMFMU_ERR_ARG;
  return launch_conv_backward(g, w, h, batch, channels, rank, ndim, lh, taps, grad_h, grad_w, ws, S(stream));
}

int64_t nmfmu_plca_backward_ws(int m, int k, int rank, int want_h, int want_w, int want_z, int* info) {
  if (m <= 0 || k <= 0 || rank <= 0) return NMFMU_ERR_ARG;
  return plca_backward_ws_floats(m, k, rank, want_h != 0, want_w != 0, want_z != 0, info);
}

int nmfmu_plca_backward(const float* g, int64_t ld, int m, int k, const float* h, const float* w, const float* z, int rank,
                        float* grad_h, float* grad_w, float* grad_z, float* ws, void* stream) {
  if (!g || !h || !w || !z || m <= 0 || k <= 0 || rank <= 0 || ld < k) return NMFMU_ERR_ARG;
  if (!grad_h && !grad_w && !grad_z) return NMFMU_ERR_ARG;
  if (!ws && plca_backward_ws_floats(m, k, rank, grad_h != nullptr, grad_w != nullptr, grad_z != nullptr, nullptr) > 0)
    return NMFMU_ERR_ARG;
  return launch_plca_backward(g, ld, m, k, h, w, z, rank, grad_h, grad_w, grad_z, ws, S(stream));
}

int64_t nmfmu_conv_plca_backward_ws(int batch, int channels, int rank, int ndim, const int32_t* lh, const int32_t* taps,
                                    int want_h, int want_w, int want_z, int* info) {
  const int64_t n = conv_plca_backward_ws_floats(batch, channels, rank, ndim, lh, taps, want_h != 0, want_w != 0, want_z != 0, info);
  return n < 0 ? NMFMU_ERR_ARG : n;
}

int nmfmu_conv_plca_backward(const float* g, const float* w, const float* h, const float* z, int batch, int channels, int rank,
                             int ndim, const int32_t* lh, const int32_t* taps, float* grad_h, float* grad_w, float* grad_z,
                             float* ws, void* stream) {
  if (!g || !w || !h || !z || (!grad_h && !grad_w && !grad_z)) return NMFMU_ERR_ARG;
  const int64_t n = conv_plca_backward_ws_floats(batch, channels, rank, ndim, lh, taps, grad_h != nullptr, grad_w != nullptr,
                                                 grad_z != nullptr, nullptr);
  if (n < 0 || (n > 0 && !ws)) return NMFMU_ERR_ARG;
  return launch_conv_plca_backward(g, w, h, z, batch, channels, rank, ndim, lh, taps, grad_h, grad_w, grad_z, ws, S(stream));
}

int nmfmu_beta_div_grad(const float* x, const float* y, int64_t n, float beta, const float* upstream, float* gx,
                        void* stream) {
  if (!x || !y || !upstream || !gx || n < 0) return NMFMU_ERR_ARG;
  if (n == 0) return NMFMU_OK;
  return launch_beta_div_grad(x, y, n, beta, nmfmu_beta_kind(beta), upstream, gx, S(stream));
}

int nmfmu_timer_create(int n_events, void** timer) {
  if (n_events <= 0 || !timer) return NMFMU_ERR_ARG;
  Timer* t = new (std::nothrow) Timer;
  if (!t) return NMFMU_ERR_ARG;
  t->ev.resize(n_events);
  for (auto& e : t->ev) {
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return (int)r;
  }
  *timer = t;
  return NMFMU_OK;
}
int nmfmu_timer_record(void* timer, int idx, void* stream) {
  Timer* t = static_cast<Timer*>(timer);
  if (!t || idx < 0 || idx >= (int)t->ev.size()) return NMFMU_ERR_ARG;
  return (int)hipEventRecord(t->ev[idx], S(stream));
}
int nmfmu_timer_elapsed_ms(void* timer, int idx_from, int idx_to, float* ms) {
  Timer* t = static_cast<Timer*>(timer);
  if (!t || !ms || idx_from < 0 || idx_to < 0 || idx_from >= (int)t->ev.size() || idx_to >= (int)t->ev.size())
    return NMFMU_ERR_ARG;
  hipError_t r = hipEventSynchronize(t->ev[idx_to]);
  if (r != hipSuccess) return (int)r;
  return (int)hipEventElapsedTime(ms, t->ev[idx_from], t->ev[idx_to]);
}
int nmfmu_timer_destroy(void* timer) {
  Timer* t = static_cast<Timer*>(timer);
  if (!t) return NMFMU_ERR_ARG;
  for (auto& e : t->ev) hipEventDestroy(e);
  delete t;
  return NMFMU_OK;
}

int nmfmu_ubench_mfma_hbm(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile,
                          int waves, int tiles, int grid, float* out, void* stream) {
  if (!operands || operand_bytes < 65536 || !out || (waves != 4 && waves != 8) || tiles <= 0 || grid <= 0) return NMFMU_ERR_ARG;
  if (kib_per_tile != 0 && !stream_src) return NMFMU_ERR_ARG;
  const int rc = launch_ubench_mfma_hbm(operands, operand_bytes, f16, stream_src, kib_per_tile, waves, tiles, grid, out, S(stream));
  return rc == -2 ? NMFMU_ERR_UNSUPPORTED : rc;
}

int nmfmu_ubench_mfma_hbm2(const void* operands, size_t operand_bytes, int f16, const void* stream_src, int kib_per_tile,
                           int waves, int tiles, int wrap_tiles, int grid, float* out, uint64_t* stamps, void* stream) {
  if (!operands || operand_bytes < 65536 || !out || (waves != 4 && waves != 8) || tiles <= 0 || grid <= 0 || wrap_tiles < 0)
    return NMFMU_ERR_ARG;
  if (kib_per_tile != 0 && !stream_src) return NMFMU_ERR_ARG;
  const int rc = launch_ubench_mfma_hbm(operands, operand_bytes, f16, stream_src, kib_per_tile, waves, tiles, grid, out, S(stream),
                                        wrap_tiles, reinterpret_cast<unsigned long long*>(stamps));
  return rc == -2 ? NMFMU_ERR_UNSUPPORTED : rc;
}

int nmfmu_debug_set_buffer(void* buf) { return debug_set_buffer(buf); }   // (NMFMU_ERR_UNSUPPORTED outside diagnostic builds)

int nmfmu_probe_mfma(const uint16_t* a, const uint16_t* b, float* d, void* stream) {
  if (!a || !b || !d) return NMFMU_ERR_ARG;
  return launch_probe_mfma(a, b, d, S(stream));
}
int nmfmu_probe_lds_dma(const uint32_t* src, uint32_t* dst, int n_dwords, void* stream) {
  if (!src || !dst || n_dwords <= 0 || n_dwords % 1024 || n_dwords > 16384) return NMFMU_ERR_ARG;
  return launch_probe_lds_dma(src, dst, n_dwords, S(stream));
}

}  // extern "C"
