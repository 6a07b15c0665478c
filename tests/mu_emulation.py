"""Float64 emulation of one dense MU half-step that rounds exactly where the kernels round (test-only).

The GPU tests of the dense MU kernels (pp_kernel, sp_kernel, sp2_kernel, fused_kernel) used to compare against
oracle/mu_oracle.py, which computes with unrounded operands, through one relative norm over the whole factor.  This module
reproduces the kernels' rounding points instead, so that what is left between kernel and emulation is fp32 accumulation
order plus one-ulp hardware transcendentals, and every output element can be held to a tight tolerance of its own.

Rounding points, as written in the sources (pytorch-nmf_amd/csrc):

* factor images: ``pack_img`` (nmfmu_fused.h) -- bf16 round-to-nearest-even, or fp16 round-to-nearest-even clamped at
  65504 (the apply kernel's fminf; the fused epilogues convert under MODE.FP16_OVFL, which saturates to the same value
  for the non-negative factors).  bf16x3: hi = bf16(x), lo = bf16(x - hi), products hi*hi + hi*lo + lo*hi (the lo*lo
  term is never formed: nmfmu_fused.h, GEMM1 and GEMM2 with ``X3``).
* stored target: ``pack_x_kernel`` (nmfmu_aux.hip) -- bf16; fp16 clamped at 65504 (pack_img); f16r = the fp32 rounded to
  nearest-even at bit 8 (``round24``); f16x and bf16x3 keep fp32.
* S = A B^T accumulated on top of eps (the accumulator seed); beta == 2 adds none (nmfmu_fused.h ``mu_elem``).  The
  ping-pong kernel's bf16 instance accumulates 2^23 (S + eps) from owner fragments scaled by 2^23 (nmfmu_pp.h ``SCALED``)
  and scales the numerator back by 2^-23: powers of two, exact, so the same emulation serves it.
* Gn / Gp per element (``mu_elem`` / ``mu_elem_scaled``), then rounded to the operand type: fp16 saturating
  (MODE.FP16_OVFL), bf16 RNE; Gn as an fp16 hi + lo pair where ``GNLO`` holds (bf16x3, and f16x at beta == 2, where Gn is
  the fp32 target itself), Gp as a bf16 hi + lo pair in bf16x3.  At beta == 2 with a 16-bit target Gn IS the stored word.
* fp16 operands, beta in {0, 0.5, generic}: both terms carry 2^ki (``FusedCfg::SCALE``), ki from the column sums the
  kernel reads (nmfmu_fused.h:435-447, the same formula in nmfmu_sp2.h:133-147), computed here in fp32 as well.  The
  slabs and the fused epilogue multiply by 2^-ki (exact).
* num = Gn B, den = Gp B; the apply of nmf.py:78-92 (apply_kernel in nmfmu_aux.hip, the fused epilogues): relu + eps on
  both accumulators (the beta == 1 closed form takes the panel's column sums as they are), + l1, + l2 * theta, ratio,
  power gamma.

The four kernel families implement the same arithmetic up to fp32 evaluation order (v_fma_mix_f32 folds the fp16 target
into the ratio, the fused epilogue multiplies by v_rcp_f32 where the apply kernel divides): no family rounds to a
different operand value on purpose, so the emulation has no per-family branch.

The beta == 2 path without the reconstruction (family 'xb': what fit() runs, DenseMU(allow_gram=True)) rounds elsewhere:

* Gram matrix (nmfmu_gram.hip): G = P2^T P2 from the panel's 16-bit transposed image, products exact in fp32, fp32
  accumulation (gram_partial_kernel :23-111, fixed-order sums in gram_finalize_kernel :117-163) -- ``gram_matrix`` is the
  float64 value, the accumulation order is what ``gram_plan`` / ``gram_excess`` allow for.  The tail of gram_finalize_kernel (:166-193) turns
  row r of the fp32 matrix into 16-bit hi / lo images times a power-of-two scale 2^ex[r] (row maximum at [2^9, 2^10)):
  ``gram_images`` mirrors it bit for bit.
* numerator (nmfmu_fused.h:805-880, ``xb_to_ops`` :379-393): X @ P2 with the stored target word as the operand (bf16 /
  f16), or the fp32 target as an fp16 hi + lo pair against the one panel plane (f16x, ``XSPLIT``) -- the beta == 2
  numerator of ``half_step``.
* denominator (nmfmu_fused.h:918-1007): den[m][r] = (sum_q owner[m][q] (G_hi[r][q] + G_lo[r][q])) * scale[r], fp32
  accumulation over 2 * R_PAD / 16 MFMAs, the scale multiplied onto the fp32 accumulator afterwards (:1001-1003).  The
  OWNER operand is its 16-bit row-major image (``load_owner_frags`` :457-467, called at :938), never the fp32 master; the
  Gram operand is the 16-bit image pair; the fp32 Gram matrix is an output of nmfmu_gram_panel that neither route reads
  (nmfmu_capi.hip:435 passes no fp32 matrix).  Both routes -- the fused apply (``den_fused`` :925) and the split one
  (``den_split`` :926, its tiles stored at :1154-1158) -- run these very lines, so they round the owner alike and the
  emulation has NO branch between them.  The apply kernel's ``den_nslab`` branch (nmfmu_aux.hip:204-216) only reads
  that ONE slab (dslab == 1: no sum over splits) and goes on with relu + eps as for every other beta.
* ``nmfmu_xb_partial`` (nmfmu_capi.hip:420-424) passes no Gram images: ``slab_den`` is dropped (:140-141), ``den_split``
  is false, and NOTHING forms a denominator -- the apply kernel has no product of its own (it only sums slabs), so the
  whole of owner @ G is left to the caller, who must fill a denominator slab before nmfmu_mu_apply.
"""
from __future__ import annotations

import numpy as np
import torch

EPS = 1.1920928955078125e-07     # kEps (nmfmu_fused.h) = constants.py:3 of the reference
F16_MAX = 65504.0
KBK = 64                         # contraction columns per tile (nmfmu_layout.h kBK)
ROW_PAD = 256                    # kRowPad

PRECISIONS = ('bf16', 'bf16x3', 'f16', 'f16x', 'f16r')
F16_OPS = ('f16', 'f16x', 'f16r')


# ---- rounding helpers (inputs: values representable in fp32; outputs: float64 arrays) -------------------------------
def _f32(x) -> np.ndarray:
    return np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(np.float32)


def round_bf16(x) -> np.ndarray:
    """v_cvt_pk_bf16_f32: round to nearest even."""
    return torch.from_numpy(_f32(x)).to(torch.bfloat16).double().numpy()


def round_f16_sat(x) -> np.ndarray:
    """fp16, round to nearest even, saturating at +-65504 (pack_img's clamp; MODE.FP16_OVFL in the kernels)."""
    x = np.clip(_f32(x), -F16_MAX, F16_MAX)
    return torch.from_numpy(x).to(torch.float16).double().numpy()


def round24_bits(bits) -> np.ndarray:
    """``round24`` of nmfmu_aux.hip on fp32 bit patterns: nearest-even at bit 8, bits 7..0 cleared; a finite value whose
    rounding would carry into the all-ones exponent is truncated instead (FLT_MAX stays finite)."""
    b = np.asarray(bits, dtype=np.uint64) & 0xffffffff
    r = (b + 0x7f + ((b >> 8) & 1)) & 0xffffffff
    ovf = ((r & 0x7f800000) == 0x7f800000) & ((b & 0x7f800000) != 0x7f800000)
    r = np.where(ovf, b, r)
    return r & 0xffffff00


def round_f16r(x) -> np.ndarray:
    """The 3-byte target of precision 'f16r': the fp32 rounded to its top 24 bits."""
    x = np.ascontiguousarray(_f32(x))
    bits = round24_bits(x.view(np.uint32)).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def round_op(x, precision: str) -> np.ndarray:
    """One 16-bit operand: fp16 (saturating) in the fp16-operand modes, bf16 otherwise."""
    return round_f16_sat(x) if precision in F16_OPS else round_bf16(x)


def split_op(x, precision: str):
    """(hi, lo) of an fp32 value as the kernels form it: hi = op(x), lo = op(x - hi) (x - hi is exact in fp32)."""
    x = _f32(x).astype(np.float64)
    hi = round_op(x, precision)
    return hi, round_op(x - hi, precision)


def factor_image(f, precision: str):
    """(hi, lo or None) of a factor's image planes (pack_img / the lo plane of bf16x3)."""
    if precision == 'bf16x3':
        return split_op(f, 'bf16')
    return round_op(f, precision), None


def stored_target(X, precision: str) -> np.ndarray:
    """The target as pack_x_kernel stores it."""
    if precision == 'bf16':
        return round_bf16(X)
    if precision == 'f16':
        return round_f16_sat(X)
    if precision == 'f16r':
        return round_f16r(X)
    return _f32(X).astype(np.float64)      # f16x, bf16x3: fp32


# ---- the half-step ------------------------------------------------------------------------------------------------
def beta_kind(beta: float) -> str:
    """kernel_beta_kind of nmfmu_capi.hip."""
    beta = float(np.float32(beta))
    return {1.0: 'kl', 2.0: 'euc', 0.0: 'is', 0.5: 'sqrt', 1.5: 'sqrt3'}.get(beta, 'gen')


def scale_exponent(cs_owner, cs_panel, M: int, K: int, beta: float, precision: str) -> int:
    """ki of nmfmu_fused.h:435-447 / nmfmu_sp2.h:133-147 (fp16 operands, negative powers of S): the power of two that
    brings the terms at the typical S = sum_r colsum_A[r] colsum_B[r] / (M K) near 1, in fp32 as the kernel computes it."""
    kind = beta_kind(beta)
    if precision not in F16_OPS or kind not in ('is', 'gen', 'sqrt') or cs_owner is None:
        return 0
    with np.errstate(over='ignore', invalid='ignore'):
        p = np.float32(np.sum(_f32(cs_owner) * _f32(cs_panel), dtype=np.float32))
        styp = np.float32(p / (np.float32(M) * np.float32(K))) + np.float32(EPS)
        if not (styp > 0 and styp < np.float32(3.0e38)):
            return 0
        bexp = np.float32(-1.0 if kind == 'is' else (-0.5 if kind == 'sqrt' else np.float32(beta) - np.float32(1.0)))
        v = np.float32(-np.rint(bexp * np.log2(styp)))
    return int(min(max(v, -40.0), 40.0))


def mu_terms(S, x, beta: float, ki: int = 0):
    """(Gn, Gp) of mu_elem / mu_elem_scaled before rounding (Gp None at beta == 1).  ``S`` already holds eps."""
    kind = beta_kind(beta)
    sc = 2.0 ** ki
    if kind == 'kl':
        return x / S, None
    if kind == 'euc':
        return x, S
    if kind == 'is':
        r = 1.0 / S
        return sc * r * r * x, sc * r
    if kind == 'sqrt':
        r = 1.0 / np.sqrt(S)
        return sc * r * r * r * x, sc * r
    if kind == 'sqrt3':
        r = 1.0 / np.sqrt(S)
        return r * x, S * r
    gp = sc * np.power(S, float(beta) - 1.0)
    return gp / S * x, gp


def rounded_terms(G, precision, split):
    """One elementwise operand set as the MFMA sees it: [hi] or [hi, lo]."""
    if split:
        return list(split_op(G, 'bf16' if precision == 'bf16x3' else precision))
    return [round_op(G, precision)]


def _gemm(lhs, rhs_hi, rhs_lo):
    """The operand-plane products the kernel forms: hi hi, plus hi lo + lo hi where both sides carry a lo plane (bf16x3),
    plus lo hi where only the left one does (f16x at beta == 2: Gn's hi + lo against ONE panel plane, nmfmu_fused.h:776)."""
    out = lhs[0] @ rhs_hi
    if len(lhs) == 2:
        out = out + lhs[1] @ rhs_hi
        if rhs_lo is not None:
            out = out + lhs[0] @ rhs_lo
    return out


# Relative perturbation under which the kernel's fp32 value of a term may differ from the float64 one: S accumulated in fp32
# (~1e-7 relative), v_rcp / v_rsq (1 ulp), v_log + v_exp of the generic branch (~1e-7 |(beta - 1) log2 S|).  A term whose
# rounding to the 16-bit operand changes inside this band is "ambiguous": the emulation cannot know which neighbour the
# kernel took, and the element's check allows the difference of the two for exactly those terms -- nothing else.
AMBIGUITY = 2e-6


def half_step(X, A, B, beta: float, precision: str, *, M=None, K=None, cs_owner=None, cs_panel=None, rounding=True,
              A_img=None, B_img=None, ratio_round=None, x_stored=None, B2=None, B2_img=None):
    """Numerator and denominator of one half-step, float64, [rows of A] x rank.

    X: [m, k] fp32 target rows (V or V^T); A: [m, R] owner rows; B: [k, R] panel.  ``A_img`` / ``B_img`` = (hi, lo or None)
    image planes to use instead of rounding A / B (the tests pass the images read back from the GPU).  M, K: the full
    owner / contraction lengths (ki), default the shapes given.  cs_owner / cs_panel: the column sums the kernel reads
    (ki).  rounding=False: every operand exact (the plain float64 algorithm of mu_oracle).  ``ratio_round(G, split)``:
    replaces the Gn / Gp rounding (seeded-fault tests).  ``x_stored``:
    the target as the kernel holds it, used instead of ``stored_target(X, precision)`` (the convolutive engine keeps fp32
    targets in every precision: tests/conv_emulation.py).  ``B2`` / ``B2_img``: the contraction panel where it is another
    matrix than the reconstruction panel (the split panel of PLCA's EM step, kModeMU2: S = A B^T + eps from ``B`` -- the
    Z-scaled factor -- and num = Gn B2 with the unscaled one); default: ``B`` / ``B_img`` itself, nothing changes.

    Returns a dict: num, den (None at beta == 1), ki, and num_amb / den_amb -- per element, the largest difference that
    the ambiguous terms (AMBIGUITY) can make."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[0] if M is None else M
    K = X.shape[1] if K is None else K
    kind = beta_kind(beta)
    if rounding:
        Ah, Al = A_img if A_img is not None else factor_image(A, precision)
        Bh, Bl = B_img if B_img is not None else factor_image(B, precision)
        x = stored_target(X, precision) if x_stored is None else np.asarray(x_stored, dtype=np.float64)
        Ch, Cl = B2_img if B2_img is not None else ((Bh, Bl) if B2 is None else factor_image(B2, precision))
    else:
        Ah, Al, Bh, Bl, x = (np.asarray(A, np.float64), None, np.asarray(B, np.float64), None, X)
        Ch, Cl = (Bh if B2 is None else np.asarray(B2, np.float64)), None
    S = _gemm([Ah] if Al is None else [Ah, Al], Bh.T, None if Bl is None else Bl.T)
    if kind != 'euc':
        S = S + EPS
    ki = scale_exponent(cs_owner, cs_panel, M, K, beta, precision) if rounding else 0
    gn, gp = mu_terms(S, x, beta, ki)
    unsc = 2.0 ** -ki
    out = {'ki': ki, 'num_amb': 0.0, 'den_amb': 0.0, 'den': None}
    if not rounding:
        out['num'] = gn @ Ch
        out['den'] = None if gp is None else gp @ Ch
        return out
    rr = ratio_round or (lambda G, split: rounded_terms(G, precision, split))
    Babs = np.abs(Ch)

    def contract(G, split, key):
        ops = rr(G, split)
        res = _gemm(ops, Ch, Cl) * unsc
        if not split:       # (a hi + lo pair holds the term to 2^-16 whichever way hi went)
            flip = np.abs(round_op(G * (1 + AMBIGUITY), precision) - round_op(G * (1 - AMBIGUITY), precision))
            if flip.any():
                out[key + '_amb'] = (flip @ Babs) * unsc
        out[key] = res

    if kind == 'euc' and precision in ('bf16', 'f16'):
        out['num'] = x @ Ch                                   # the stored word is the operand (nmfmu_fused.h:690)
    else:
        contract(gn, precision == 'bf16x3' or (precision == 'f16x' and kind == 'euc'), 'num')
    if gp is not None:
        contract(gp, precision == 'bf16x3', 'den')
    return out


def apply_allowance(theta_new, num, den, amb_num, amb_den, beta: float, gamma: float, kl_den=None, l1=0.0, l2=0.0,
                    theta=None):
    """What the ambiguous terms of num / den can move the updated factor by (first order: d new / new = gamma (d neg / neg
    - d pos / pos))."""
    neg = np.maximum(num, 0.0) + EPS
    a = np.asarray(amb_num) / neg
    if beta_kind(beta) != 'kl':
        pos = np.maximum(den, 0.0) + EPS + l1 + (l2 * theta if l2 > 0 else 0.0)
        a = a + np.asarray(amb_den) / pos
    return np.abs(theta_new) * gamma * a


def apply(theta, num, den, beta: float, gamma: float, l1=0.0, l2=0.0, kl_den=None):
    """nmf.py:78-92 as apply_kernel / the fused epilogues do it: relu + eps, closed-form denominators at beta == 1."""
    theta = np.asarray(theta, dtype=np.float64)
    neg = np.maximum(num, 0.0) + EPS
    if beta_kind(beta) == 'kl':
        pos = np.broadcast_to(np.asarray(kl_den, dtype=np.float64)[:theta.shape[1]], theta.shape)
    else:
        pos = np.maximum(den, 0.0) + EPS
    if l1 > 0:
        pos = pos + l1
    if l2 > 0:
        pos = pos + l2 * theta
    mult = neg / pos
    if gamma != 1:
        mult = np.power(mult, gamma)
    return theta * mult


# ---- beta == 2 without the reconstruction: Gram matrix, its images, the XB half-step ----------------------------------
GRAM_MAX_CHUNKS = 256     # kGramMaxChunks (nmfmu_gram.hip)
GRAM_TILES_PER_CHUNK = 4  # kGramTilesPerChunk
# NMFMU_XB_NSTAGE (nmfmu_fused.h:195-197).  A library built with another value (make EXTRA=-DNMFMU_XB_NSTAGE=3) needs this
# constant edited along with the build flag: the ring claims below describe the kernel only while the two agree.
XB_NSTAGE = 4


def xb_nstage(precision: str) -> int:
    """FusedCfg::NSTAGE of the kModeXB instances (nmfmu_fused.h:198): ring stages of the X / panel streams -- three for the
    fp32 target of 'f16x' (XF32), else NMFMU_XB_NSTAGE."""
    return 3 if precision == 'f16x' else XB_NSTAGE


def gram_matrix(B_img) -> np.ndarray:
    """B_img^T B_img in float64; B_img = the panel's 16-bit image VALUES, padded rows and columns included."""
    B = np.asarray(B_img, dtype=np.float64)
    return B.T @ B


def gram_images(G32, r_pad: int, f16: bool):
    """Bit-exact mirror of the tail of gram_finalize_kernel (nmfmu_gram.hip:166-193) on the fp32 matrix [r_pad, r_pad]:
    row maximum -> frexp -> ex - 10 (ex = 0 for a zero row and for a row whose maximum is not below 3e38), scale = 2^ex,
    hi = round16(v 2^-ex), lo = round16(v 2^-ex - hi).  Returns (hi words, lo words: uint16 [r_pad, r_pad], scale fp32)."""
    G = np.ascontiguousarray(np.asarray(G32, dtype=np.float32).reshape(r_pad, r_pad))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        m = np.fmax.reduce(np.fmax(G, np.float32(0.0)), axis=1)       # fmaxf drops NaN (an all-NaN row fails ``m > 0`` too)
        ok = (m > 0) & (m < np.float32(3.0e38))
        _, ex = np.frexp(np.where(ok, m, np.float32(1.0)))
        ex = np.where(ok, ex.astype(np.int64) - 10, 0)
        down = np.ldexp(np.float32(1.0), -ex).astype(np.float32)
        scale = np.ldexp(np.float32(1.0), ex).astype(np.float32)
        v = torch.from_numpy((G * down[:, None]).astype(np.float32))
        dt = torch.float16 if f16 else torch.bfloat16
        hi = v.to(dt)
        lo = (v - hi.float()).to(dt)
    words = lambda t: t.view(torch.int16).numpy().view(np.uint16).copy()
    return words(hi), words(lo), scale


def image_values(words, f16: bool) -> np.ndarray:
    """float64 values of 16-bit image words."""
    w = torch.from_numpy(np.ascontiguousarray(words).view(np.int16))
    return w.view(torch.float16 if f16 else torch.bfloat16).double().numpy()


def gram_plan(rows: int, r_pad: int) -> dict:
    """Launch arithmetic of nmfmu_gram_panel (nmfmu_gram.hip:217-221) and the summation chain of an element of the fp32 matrix.

    ``n_seq`` = the longest chain of sequential fp32 additions a product passes through: 16 inside its MFMA (K = 16 products
    per instruction; their order is not documented, so the worst one is taken), 4 MFMA accumulations per 64-row tile x
    ``per`` tiles in a chunk's accumulator (:59-65, :80-96), ceil(nchunk / ngrp) additions of chunk partials in one thread
    group of the finalize (:132-149; the rounds of 16 and 8 add in the same order as the single ones), ngrp - 1 additions
    of the groups (:152-157)."""
    ktiles = pad_rows(rows) // KBK
    nchunk = ktiles if ktiles <= GRAM_MAX_CHUNKS else -(-ktiles // GRAM_TILES_PER_CHUNK)
    nchunk = min(nchunk, GRAM_MAX_CHUNKS)
    per = -(-ktiles // nchunk)
    ngrp = 256 // (r_pad // 4)
    tiles = [max(0, min(ktiles, (c + 1) * per) - c * per) for c in range(nchunk)]
    return dict(ktiles=ktiles, nchunk=nchunk, per=per, ngrp=ngrp, tiles=tiles,
                n_seq=16 + 4 * per + -(-nchunk // ngrp) + ngrp - 1)


def gram_excess(G32, ref, n_seq: int) -> float:
    """max over the elements of |G32 - ref| / (n_seq 2^-24 ref): every term of an element is non-negative, so the standard
    bound of a summation tree of depth n_seq holds relative to the element itself.  An element whose reference is zero
    (padding) must be exactly zero; a non-finite element counts as inf.  The check is ``gram_excess(...) <= 1``."""
    G = np.asarray(G32, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = n_seq * 2.0 ** -24 * np.abs(ref)
    diff = np.abs(G - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    return float(np.where(np.isfinite(G), ratio, np.inf).max())


def xb_half_step(X, A_img, B_img, G_hi, G_lo, scale, precision: str, rounding=True):
    """Numerator and denominator of one beta == 2 half-step on the Gram path, float64.

    X: [m, k] fp32 target rows; A_img: [m, q] the owner's 16-bit image values; B_img: [k, q] the panel's; G_hi / G_lo:
    [r, q] values of the Gram image planes (row r = column r of the matrix, carrying 2^-ex[r]); scale: [r] = 2^ex[r].
    num = the beta == 2 numerator of ``half_step`` (stored word, or the fp16 hi + lo pair of 'f16x'); den[m][r] =
    (sum_q A_img[m][q] (G_hi[r][q] + G_lo[r][q])) scale[r] -- the fused and the split epilogue alike (see the header).
    (``half_step`` also forms the reconstruction path's m x k denominator on the way; it is discarded here.)
    rounding=False: the plain algorithm (exact target; pass exact factors and G_hi = gram_matrix, G_lo = 0, scale = 1)."""
    A = np.asarray(A_img, dtype=np.float64)
    B = np.asarray(B_img, dtype=np.float64)
    hs = half_step(X, A, B, 2.0, precision, A_img=(A, None), B_img=(B, None), rounding=rounding)
    G = np.asarray(G_hi, dtype=np.float64) + np.asarray(G_lo, dtype=np.float64)
    den = (A @ G.T) * np.asarray(scale, dtype=np.float64)[None, :]
    return {'num': hs['num'], 'den': den, 'num_amb': hs['num_amb'], 'den_amb': 0.0}


# ---- the contraction split (mirror of nmfmu_capi.hip) ----------------------------------------------------------------
def pad_rows(n: int) -> int:
    return -(-n // ROW_PAD) * ROW_PAD


def pad_rank(r: int) -> int:
    for p in (32, 64, 128, 256):
        if r <= p:
            return p
    raise ValueError(r)


def kernel_family(r_pad: int, precision: str, beta: float, block_rows: int) -> str:
    """Which kernel runs the MU half-step (fused_dispatch): 'pp' (256-row tiles), 'sp', 'sp2' or 'fused'."""
    kind = beta_kind(beta)
    if block_rows == 256:
        return 'pp'
    if kind == 'kl' and r_pad == 256 and precision == 'f16':
        return 'sp'
    if kind in ('is', 'gen', 'sqrt', 'sqrt3') and r_pad == 128 and precision == 'f16':
        return 'sp2'
    return 'fused'


def default_block_rows(r_pad: int, precision: str, beta: float) -> int:
    """nmfmu_step_block_rows: the ping-pong kernel's 256-row tiles where it is eligible."""
    return 256 if beta_kind(beta) == 'kl' and r_pad <= 128 and precision in ('bf16', 'f16', 'f16r') else 128


def choose_nsplit(m_pad: int, k_pad: int, r_pad: int, precision: str, beta: float, block_rows: int, ncu: int,
                  forced=None) -> int:
    """engine.HipBackend.choose_nsplit: the TORCHNMF_AMD_NSPLIT hook, else nmfmu_choose_nsplit_for."""
    if forced:
        return max(1, min(int(forced), k_pad // 64 // 4))
    mblocks, ktiles = m_pad // block_rows, k_pad // KBK
    if kernel_family(r_pad, precision, beta, block_rows) in ('sp', 'sp2'):
        ns = (max(ncu, 1) + mblocks - 1) // mblocks
        return max(min(ns, max(1, ktiles // 8)), 1)
    target = (2 if block_rows == 128 else 1) * max(ncu, 1)
    ns = (target + mblocks - 1) // mblocks
    if ns > 8:
        ns = (ns + 7) // 8 * 8
    return max(min(ns, max(1, ktiles // 4)), 1)


def tiles_per_split(k_pad: int, nsplit: int, family: str):
    """(tiles_per_split before the family's rounding, after it): x2 for pp's unrolled loop, x4 for sp / sp2's groups."""
    raw = -(-(k_pad // KBK) // nsplit)
    if family == 'pp':
        return raw, (raw + 1) & ~1
    if family in ('sp', 'sp2'):
        return raw, (raw + 3) & ~3
    return raw, raw


def split_tiles(k_pad: int, nsplit: int, family: str):
    """Tiles each contraction split works on (0 = an empty workgroup: the kernels' ``nt > 0`` guards)."""
    ktiles = k_pad // KBK
    tps = tiles_per_split(k_pad, nsplit, family)[1]
    return [max(0, min(ks * tps + tps, ktiles) - ks * tps) for ks in range(nsplit)]


# ---- per-element check ---------------------------------------------------------------------------------------------
# Per-element relative tolerances of the emulated-parity tests: the largest error the first MI355X run recorded over the
# whole case matrix (after the ambiguity allowance) with about 3x margin -- bf16 7.5e-7, bf16x3 1.3e-6, f16 7.2e-7,
# f16x 5.7e-7, f16r 4.9e-7.  What is left between kernel and emulation is fp32 accumulation order and one-ulp
# transcendentals; the ambiguous roundings are allowed for separately, term by term.
TOL = {'bf16': 2.5e-6, 'bf16x3': 4e-6, 'f16': 2.5e-6, 'f16x': 2e-6, 'f16r': 1.5e-6}
FLOOR = 1e-6      # near-zero entries are measured against this fraction of their column's largest |ref|


def elem_err(got, ref, allow=0.0) -> np.ndarray:
    """Per element: (|got - ref| - allow)+ / max(|ref|, FLOOR * max |ref| of the column); inf where got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.maximum(np.abs(ref), FLOOR * np.abs(ref).max(axis=0, keepdims=True))
    scale = np.where(scale > 0, scale, 1.0)
    err = np.maximum(np.abs(got - ref) - allow, 0.0) / scale
    return np.where(np.isfinite(got), err, np.inf)


# ---- the case matrix of tests/test_gpu_emulated_parity.py ---------------------------------------------------------------
def half_step_plan(N: int, C: int, R: int, precision: str, beta: float, ncu: int, nsplit=None, block_rows=None,
                   gram=False):
    """{'w': ..., 'h': ...}: the kernel family, tile height, split and per-split tiles each half-step runs with.
    gram: the engine was built with allow_gram -- beta == 2 runs family 'xb' (kModeXB, 128-row tiles; the four-wave
    kernel's split rule, tiles per split not rounded: nmfmu_capi.hip:115)."""
    r_pad = pad_rank(R)
    plan = {}
    for which, (m, k) in (('w', (C, N)), ('h', (N, C))):
        m_pad, k_pad = pad_rows(m), pad_rows(k)
        br = block_rows or default_block_rows(r_pad, precision, beta)
        fam = kernel_family(r_pad, precision, beta, br)
        if gram and beta_kind(beta) == 'euc':
            assert br == 128 and precision in ('bf16', 'f16', 'f16x') and (precision != 'f16x' or r_pad <= 128)
            fam = 'xb'
        ns = choose_nsplit(m_pad, k_pad, r_pad, precision, beta, br, ncu, nsplit)
        plan[which] = dict(M=m, K=k, m_pad=m_pad, k_pad=k_pad, block_rows=br, family=fam, nsplit=ns,
                           tps_raw=tiles_per_split(k_pad, ns, fam)[0], tiles=split_tiles(k_pad, ns, fam), r_pad=r_pad,
                           nstage=xb_nstage(precision))
    return plan


def claim_holds(claim: str, p: dict, R: int) -> bool:
    """Does one half-step's plan ``p`` reach the control flow ``claim`` names?"""
    t = p['tiles']
    live = [x for x in t if x]
    nst, rt = p['nstage'], p['r_pad'] // 32
    xb = p['family'] == 'xb'
    return {
        # family 'xb': the NSTAGE-deep ring of nmfmu_fused.h:805-880 and the denominator tiles of :918-1007 / :1154-1158
        'ring_prologue_short': xb and any(x < nst - 1 for x in live),
        'ring_rem1': xb and any(x % nst == 1 for x in live),
        'ring_rem2': xb and any(x % nst == 2 for x in live),
        'ring_rem3': xb and any(x % nst == 3 for x in live),
        'ring_exact': xb and any(x % nst == 0 for x in live),
        'den_tiles_shared': xb and p['nsplit'] > 1 and min(p['nsplit'], rt) > 1,
        'den_tiles_fewer_splits_than_tiles': xb and 1 < p['nsplit'] < rt,
        'den_more_splits_than_tiles': xb and p['nsplit'] > rt > 1,
        'empty_split_owns_den_tile': xb and any(x == 0 and ks < min(p['nsplit'], rt) for ks, x in enumerate(t)),
        'den_one_tile_owner': xb and p['nsplit'] > 1 and rt == 1,
        'den_one_slab_unsplit': xb and p['r_pad'] == 256 and p['nsplit'] == 1,
        'touched_prefetch': xb and p['nsplit'] == 1 and R == p['r_pad'] == 128 and p['M'] % 128 == 0,
        'empty_split': 0 in t,
        'short_last_split': len([x for x in t if x]) > 1 and 0 < [x for x in t if x][-1] < t[0],
        'odd_tps': p['nsplit'] > 1 and p['tps_raw'] % 2 == 1,
        'fused_apply': p['nsplit'] == 1 and not (xb and p['r_pad'] > 128),
        'split': p['nsplit'] > 1,
        'one_group': t == [4],
        'several_groups': p['nsplit'] == 1 and t[0] > 4,
        'ragged_m': p['M'] % p['block_rows'] != 0,
        'ragged_k': p['K'] % KBK != 0,
        'ragged_r': R < p['r_pad'],
        'm1': p['M'] == 1,
    }[claim]


def heuristic_empty_split_cols(ncu: int, N: int = 2200) -> int:
    """A column count C for which the product's own split of the rank-256 fp16 beta == 1 W half-step (owner C, contraction
    N) leaves an empty split on ``ncu`` CUs -- 9000 on 256 CUs (nsplit 4, tiles [12, 12, 12, 0]), else searched."""
    for C in [9000] + [mb * 128 - 56 for mb in range(2 * max(ncu, 1), 1, -2)]:
        if C > 0 and 0 in half_step_plan(N, C, 256, 'f16', 1.0, ncu)['w']['tiles']:
            return C
    raise ValueError(f'no empty-split shape for {ncu} CUs')


def parity_cases(ncu: int):
    """The case matrix: dicts of family, precision, beta, N, C, R, forced nsplit / block_rows, stage, regularisation,
    target kind, the control-flow claims the case is named for, and the owner rows to sample (None = all)."""
    cases = []

    def add(family, prec, beta, N, C, R, nsplit=None, claims=(), block_rows=None, stage='dma', regs=(0.0, 0.0),
            target='rand', sample=None):
        tag = f'{family}-{prec}-b{beta:g}-{N}x{C}r{R}-ns{nsplit}-{stage}' + (f'-{target}' if target != 'rand' else '') \
            + ('-reg' if regs != (0.0, 0.0) else '')
        cases.append(dict(id=tag, family=family, precision=prec, beta=float(beta), N=N, C=C, R=R, nsplit=nsplit,
                          block_rows=block_rows, stage=stage, regs=regs, target=target, claims=tuple(claims), sample=sample))

    # ping-pong kernel (beta == 1, one operand plane, padded rank <= 128, 256-row tiles)
    for prec in ('bf16', 'f16', 'f16r'):
        add('pp', prec, 1, 1, 300, 1, 1, ('m1', 'fused_apply', 'ragged_r'))
        add('pp', prec, 1, 257, 1100, 33, 4, ('odd_tps', 'split', 'ragged_m', 'ragged_k', 'ragged_r'))
        add('pp', prec, 1, 600, 1000, 100, 1, ('fused_apply', 'ragged_m'), regs=(0.05, 0.05))
        add('pp', prec, 1, 300, 2100, 128, None, ('split',))
    add('pp', 'f16', 1, 300, 1000, 64, 2, ('split',), target='zeros')
    # software-pipelined rank-256 kernel (beta == 1, fp16)
    add('sp', 'f16', 1, 300, 200, 200, None, ('one_group', 'several_groups', 'fused_apply', 'ragged_m', 'ragged_k', 'ragged_r'))
    add('sp', 'f16', 1, 400, 1300, 129, 3, ('split', 'ragged_r'))
    add('sp', 'f16', 1, 300, 1200, 200, 4, ('empty_split', 'short_last_split'))
    add('sp', 'f16', 1, 300, 1200, 256, 4, ('empty_split', 'short_last_split'), stage='nop2')
    add('sp', 'f16', 1, 600, 1000, 256, 1, ('fused_apply',), stage='nop2', regs=(0.05, 0.05))
    add('sp', 'f16', 1, 2200, heuristic_empty_split_cols(ncu), 256, None, ('empty_split',), stage='nop2', sample=64)
    # two-accumulator software-pipelined kernel (padded rank 128, beta not in {1, 2}, fp16)
    for beta in (0.0, 0.5, 1.5, 0.3, 3.0, -1.0):
        add('sp2', 'f16', beta, 300, 1200, 100, 4, ('empty_split', 'short_last_split', 'ragged_r'))
        add('sp2', 'f16', beta, 600, 1000, 128, 1, ('fused_apply',), regs=(0.05, 0.05))
        add('sp2', 'f16', beta, 130, 500, 65, None, ('one_group', 'fused_apply', 'ragged_m', 'ragged_k'))
    add('sp2', 'f16', 0.5, 300, 1200, 128, 2, ('split',), target='zeros')
    # four-wave kernel: beta == 1 on 128-row tiles, then every other beta, every precision it serves
    shapes = [((200, 330, 24), None, ('ragged_m', 'ragged_k', 'ragged_r')),
              ((384, 1100, 64), 3, ('split',)),
              ((520, 700, 100), 1, ('fused_apply', 'ragged_r')),
              ((300, 640, 200), 2, ('split', 'ragged_r'))]
    i = 0
    for beta in (1.0, 0.0, 0.5, 1.5, 0.3, 3.0, -1.0, 2.0):
        for prec in PRECISIONS:
            if prec == 'f16r' and beta == 2.0:
                continue
            for _ in range(len(shapes)):
                (N, C, R), ns, claims = shapes[i % len(shapes)]
                i += 1
                r_pad = pad_rank(R)
                if not (prec == 'bf16x3' and r_pad > 128) and kernel_family(r_pad, prec, beta, 128) == 'fused':
                    break
            add('fused', prec, beta, N, C, R, ns, claims, block_rows=128 if beta == 1.0 else None,
                regs=(0.05, 0.05) if i % 3 == 0 else (0.0, 0.0))
    for beta in (0.0, 0.5):
        for target in ('scale1e-3', 'scale30'):
            add('fused', 'f16', beta, 384, 1100, 64, 3, ('split',), target=target)
    add('fused', 'f16', 0.5, 520, 700, 64, 1, ('fused_apply',), target='zeros')
    return cases


def make_problem(case, seed=None):
    """(V, W0, H0) of a case, fp32 on the CPU."""
    N, C, R = case['N'], case['C'], case['R']
    g = torch.Generator().manual_seed(seed if seed is not None else (N * 7 + C * 3 + R) % 100003)
    V = torch.rand(N, C, generator=g)
    beta = case['beta']
    if case['target'] == 'zeros':
        V = torch.where(torch.rand(N, C, generator=g) < 0.3, torch.zeros(()), V)
    elif beta <= 0:
        V = V + 2.0 ** -7
    W0 = torch.randn(C, R, generator=g).abs() + 0.05
    H0 = torch.randn(N, R, generator=g).abs() + 0.05
    if case['target'].startswith('scale'):
        s = float(case['target'][5:])
        V, W0, H0 = V * s, W0 * s ** 0.5, H0 * s ** 0.5
    if case.get('family') == 'xb':
        # rank columns of unlike magnitude (1, 2, 4, 1, ...): neighbouring rows of the Gram image then carry different
        # power-of-two scales, so a scale applied to the wrong row shows (tests/test_mu_emulation.py, fault (b))
        W0, H0 = W0 * xb_column_scales(R), H0 * xb_column_scales(R)
    if case['target'] == 'fac30':          # factors x 30 (their Gram matrix leaves fp16's range), the target to match
        V, W0, H0 = V * 900.0, W0 * 30.0, H0 * 30.0
    elif case['target'] == 'zero_row':       # an all-zero owner row in either half-step: its numerator is exactly 0
        V[min(3, N - 1), :] = 0.0
        V[:, min(5, C - 1)] = 0.0
    return V, W0, H0


# ---- the case matrices of tests/test_gpu_gram_emulated_parity.py -----------------------------------------------------
def gram_cases():
    """nmfmu_gram_panel: (rows, rank) x {f16, bf16}, with the launch arithmetic each is named for and ``n_seq``, the length
    of the longest sequential fp32 addition chain (``gram_plan``), written out per case."""
    shapes = [  # rows, rank, n_seq, what
        (1, 1, 52, 'one live row, three all-zero tiles'),
        (300, 24, 52, 'padded rank 32: RT = 1, idle waves; finalize with nchunk 8 < ngrp 32'),
        (700, 64, 36, '12 one-tile chunks'),
        (5000, 128, 37, '80 one-tile chunks'),
        (300, 200, 25, 'padded rank 256, one tile per chunk'),
        (16500, 100, 48, '260 tiles -> 65 chunks of 4: the even double-buffer loop'),
        (16500, 256, 52, 'the rank-256 loop with 4 tiles per chunk; finalize with ngrp 4'),
        (66000, 40, 67, '1032 tiles -> 256 chunks of 5 (odd loop), one 2-tile chunk, 49 empty chunks'),
        (82000, 128, 79, '1284 tiles -> 6 per chunk, 42 empty chunks'),
    ]
    cases = []
    for rows, rank, n_seq, what in shapes:
        for prec in ('f16', 'bf16'):
            cases.append(dict(id=f'{rows}x{rank}-{prec}', rows=rows, rank=rank, precision=prec, n_seq=n_seq, scale=1.0,
                              what=what))
    for sc in (200.0, 1e-3):   # Gram entries above 65504 (the row scale must keep hi finite) / far below 1
        cases.append(dict(id=f'5000x128-f16-x{sc:g}', rows=5000, rank=128, precision='f16', n_seq=37, scale=sc,
                          what='range'))
    return cases


def gram_problem(case):
    """The factor of a Gram case, fp32 on the CPU."""
    g = torch.Generator().manual_seed(case['rows'] * 3 + case['rank'])
    return torch.randn(case['rows'], case['rank'], generator=g).abs() * (3.0 * case['scale'])


def xb_column_scales(R: int) -> torch.Tensor:
    return 2.0 ** (torch.arange(R) % 3).float()


XB_PRECISIONS = ('bf16', 'f16', 'f16x')


def xb_cases(ncu: int):
    """beta == 2 on the Gram path (DenseMU(allow_gram=True)): dicts like ``parity_cases``.  The contraction axis is C in the H
    half-step and N in the W half-step; k_pad is a multiple of 256, so tile counts come in fours, and a forced split is
    clipped to ktiles // 4 -- the short axis of a case therefore runs the fused apply on 4 tiles."""
    cases = []

    def add(prec, N, C, R, nsplit, claims, target='rand'):
        regs = (0.05, 0.05) if len(cases) % 3 == 0 else (0.0, 0.0)
        claims = tuple(c for c in claims if not c.startswith('@')) + \
            tuple(c[2:] for c in claims if c.startswith('@' + str(xb_nstage(prec))))
        tag = f'xb-{prec}-{N}x{C}r{R}-ns{nsplit}' + (f'-{target}' if target != 'rand' else '') + ('-reg' if regs[0] else '')
        cases.append(dict(id=tag, family='xb', precision=prec, beta=2.0, N=N, C=C, R=R, nsplit=nsplit, block_rows=None,
                          stage='dma', regs=regs, target=target, claims=claims, sample=None))

    # claims written '@4name' / '@3name' hold at NSTAGE 4 (bf16, f16) / 3 (f16x) only
    for prec in XB_PRECISIONS:
        # unsplit, 4 tiles: the fused apply with the Gram image from global memory (padded rank 32) and through LDS (64, 128)
        for R in (24, 64, 100, 128):
            add(prec, 200, 250, R, 1, ('fused_apply', 'ragged_m', 'ragged_k', '@4ring_exact', '@3ring_rem1')
                + (('ragged_r',) if R in (24, 100) else ()))
        add(prec, 130, 2300, 64, 8, ('ring_prologue_short', 'short_last_split', 'ring_rem1', 'den_tiles_shared',
                                     'den_more_splits_than_tiles', '@3ring_rem2'))                 # [5]*7 + [1]
        add(prec, 130, 2048, 100, 7, ('short_last_split', 'ring_rem2', '@4ring_prologue_short', '@4ring_rem1'))  # [5]*6 + [2]
        add(prec, 130, 1792, 24, 6, ('short_last_split', 'den_one_tile_owner', '@4ring_rem3', '@3ring_exact'))   # [5]*5 + [3]
        add(prec, 130, 2304, 128, 7, ('empty_split', 'den_tiles_shared', '@4ring_rem2', '@3ring_exact'))         # [6]*6 + [0]
        add(prec, 1280, 130, 64, 3, ('short_last_split', '@4ring_rem3', '@4ring_rem2', '@3ring_rem1', '@3ring_exact'))  # [7, 7, 6]
        add(prec, 1100, 300, 24, 4, ('den_one_tile_owner', 'ragged_r'))                            # [5]*4 | [4, 4]: nd = 1
        add(prec, 520, 1100, 128, 2, ('den_tiles_shared', 'den_tiles_fewer_splits_than_tiles'))   # [10, 10] | [6, 6]
        add(prec, 256, 384, 128, 1, ('fused_apply', 'touched_prefetch'))
        add(prec, 129, 385, 100, 1, ('fused_apply', 'ragged_m', 'ragged_r'))                       # owner rows = 1 mod 128
    for prec in ('f16', 'f16x'):
        add(prec, 520, 1100, 128, 4, ('den_tiles_shared',))                                        # [5]*4 | [4, 4, 4]
    for prec in ('bf16', 'f16'):
        add(prec, 1, 1100, 64, 4, ('m1',))                                                         # M = 1, split; K = 1 in the W half-step
        # padded rank 256 (RT = 8): one slab from an unsplit launch, fewer splits than rank tiles, more splits than rank tiles
        add(prec, 300, 640, 200, 1, ('den_one_slab_unsplit', 'ragged_r'))
        add(prec, 300, 1280, 200, 3, ('den_tiles_fewer_splits_than_tiles', 'den_tiles_shared'))   # tiles {0,3,6} {1,4,7} {2,5}
        add(prec, 130, 2304, 200, 9, ('den_more_splits_than_tiles',))                              # [4]*9: ks = 8 owns no tile
        # [6]*6 + [0] with nd = 7: the empty split skips the ring and still forms rank tile 6 of the denominator
        add(prec, 130, 2304, 200, 7, ('empty_split', 'empty_split_owns_den_tile'))
    add('f16x', 1, 300, 24, 1, ('m1', 'fused_apply'))
    add('f16', 520, 1100, 128, 2, ('den_tiles_shared',), target='zeros')
    add('f16', 384, 1100, 64, 3, ('split',), target='zero_row')
    add('f16x', 200, 250, 64, 1, ('fused_apply',), target='zero_row')
    add('f16', 384, 1100, 64, 3, ('split',), target='fac30')
    add('f16', 256, 384, 128, 1, ('fused_apply',), target='fac30')
    return cases


# every claim of family 'xb', and the NSTAGE values it can be reached at
XB_CLAIMS = {'ring_prologue_short': (3, 4), 'ring_rem1': (3, 4), 'ring_rem2': (3, 4), 'ring_rem3': (4,), 'ring_exact': (3, 4),
             'den_tiles_shared': (3, 4), 'den_tiles_fewer_splits_than_tiles': (3, 4), 'den_one_slab_unsplit': (4,),
             'empty_split': (3, 4), 'empty_split_owns_den_tile': (4,), 'short_last_split': (3, 4), 'fused_apply': (3, 4), 'ragged_m': (3, 4), 'ragged_k': (3, 4),
             'ragged_r': (3, 4), 'm1': (3, 4)}


# ---- the dense loss pass (kModeLoss of fused_kernel / pp_kernel), the riding loss, metrics.beta_div -----------------------
# What ``DenseMU.divergence()`` and fit()'s stop rule read.  One workgroup per (row block mb, contraction split ks) writes ONE
# float into loss_part[mb * nsplit + ks] (nmfmu_fused.h:907-914 on four waves, nmfmu_pp.h:818-825 on eight); the fixed-order
# sum_finalize_kernel (nmfmu_aux.hip:403-414) adds them in float64.  The model below gives every partial in float64 from the
# operand images the GPU holds, and a bound of its own:
#
#     |got - ref|  <=  sum over the workgroup's elements i of
#                          U * sum_k c_k |term_k(i)|                  loss_elem's own roundings           (``c_elem``)
#                        + gamma(depth_i) * |l_i|                     the fp32 additions element i passes (``n_chain``, ``tree``)
#                        + gamma(n_seq_S) * |dl/ds (i)| s_i           the fp32 reconstruction              (``err_S``)
#
# with U = 2^-24 and gamma(n) = n U / (1 - n U).  It is the form  U (c_elem + n_chain + tree) sum|terms| + sum |dl/ds| |s|
# err_S  with two replacements that only tighten it: the summation error is taken on |l_i| <= sum_k |term_k(i)|, and element
# i is charged the additions it really passes through, depth_i <= n_chain + tree, not the longest chain.  Every constant is
# counted from the source; none comes from running a kernel.
#
# * c_elem, from loss_elem (nmfmu_fused.h:333-352); a hardware transcendental (v_log_f32, v_exp_f32, v_rcp_f32: one ulp)
#   counts as LOSS_FN = 2 roundings of its own result, the rounded constant kLn2 as one:
#     beta 2   d = s - x, 0.5 d d: d enters twice, one multiply (x 0.5 is exact)                           c = 3 on d^2 / 2
#     beta 1   x ((lx - ls) kLn2) - x + (s - eps), terms x ln(x + eps), x ln s, x, s:
#              the logarithm 2, lx - ls 1, x kLn2 2, x x 1, the two additions that follow 1 each            c = 8 on the two x ln
#              x + eps rounds once: ln(x + eps) moves by U, x ln(x + eps) by U |x|; two additions            c = 3 on x
#              s - eps, the last addition                                                                   c = 2 on s
#     beta 0   xe / s - (lx - ls) kLn2 - 1, xe = x + eps, terms xe / s, ln xe, ln s, 1:
#              xe 1, v_rcp 2, the multiply 1, two subtractions                                              c = 6 on xe / s
#              the logarithm 2, lx - ls 1, x kLn2 2, two subtractions                                       c = 7 on the two ln
#              xe's rounding moves ln xe by U; the last subtraction                                         c = 2 on the 1
#     generic  (t1 + (beta - 1) t2 - beta xb sb1) / (beta (beta - 1)), t1 = exp2(beta log2 xb), sb1 = exp2((beta - 1) log2 s),
#              t2 = sb1 s.  An exponent e = c log2 v carries (2 + 1 [+ 1 where c = beta - 1 is itself rounded]) U |e| and
#              moves exp2 by ln 2 times that; exp2's own ulp 2.  The quotient: beta - 1, the product, the division (one ulp)
#              = 4; the two additions 1 each where a term passes them.
#              t1:  2 + 3 |beta ln xb| + |beta| (xb = x + eps rounds, beta < 0) + 2 + 4
#              t2:  2 + 4 |(beta - 1) ln s| + 3 (x s, x (beta - 1), beta - 1) + 2 + 4
#              t3:  2 + 4 |(beta - 1) ln s| + 3 (two multiplies, xb) + 1 + 4
#              less every operation on the scalar beta that is exact in fp32 for the beta at hand (``_gen_roundings``:
#              beta - 1.f for 0.5, 1.5, 3 and -1, a multiplication by a power of two)
#   Contraction to fused multiply-adds (hipcc's default) only removes roundings.
# * n_chain: a lane adds its 32 elements of every tile to ONE accumulator in the order (tt, d, low / high half of the word)
#   (``elem_pair`` through ``elementwise``, nmfmu_fused.h:658-663, :703-707; nmfmu_pp.h:572-589), masked elements as 0.f:
#   32 x (tiles of the split) additions, element i at slot 32 (t - t0) + (k mod 32) passes the 32 nt - slot that follow.
# * tree: six __shfl_xor levels, then (r0 + r1) + (r2 + r3): 6 + 2 = 8 on four waves, 6 + 3 = 9 on eight.
# * err_S: products of two 16-bit operands are exact in fp32 and all non-negative; a product passes through at most the 16
#   additions inside its MFMA (K = 16; the order is not documented, the worst is taken, as ``gram_plan`` does) and one per
#   MFMA of the chain that follows, R_PAD / 16 of them (three times as many with the lo planes of bf16x3), eps being the
#   seed: n_seq_S = 16 + planes R_PAD / 16 + 1.  The lo x lo product bf16x3 never forms is left out of the float64 S too
#   (``_gemm``), so it needs no allowance; the ping-pong kernel's 2^23 scaling of bf16 is exact.
#   |dl/ds| s:  beta 2: |s - x| s;  beta 1: |s - x|;  beta 0: |1 - xe / s|;  generic: |s^beta - xb s^(beta - 1)|.
# A partial whose bound is zero (an empty split, a split or a row block of padding only) must be exactly 0.0.
LOSS_U = 2.0 ** -24
LOSS_FN = 2.0                 # roundings' worth of a one-ulp hardware transcendental
LOSS_TREE = {'fused': 6 + 2, 'pp': 6 + 3}
LOSS_CAP = 1e-5               # non-vacuity: a case's bound may not exceed this fraction of the partial's sum |terms|
LN2 = float(np.log(2.0))


def _gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * LOSS_U / (1.0 - n * LOSS_U)


def s_chain(r_pad: int, precision: str) -> int:
    """n_seq_S: the longest chain of fp32 additions behind one element of S = owner panel^T + eps (see above)."""
    return 16 + (3 if precision == 'bf16x3' else 1) * (r_pad // 16) + 1


def loss_elem_terms(s, x, beta: float, eps_in_log=True):
    """loss_elem in float64, term by term as the source forms them.  ``s`` already holds eps (none at beta == 2).
    Returns (l, w, sens): the element's loss, sum_k c_k |term_k| (in units of U) and |dl/ds| s."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    beta = float(np.float32(beta))
    kind = beta_kind(beta)
    le = EPS if eps_in_log else 0.0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if kind == 'euc':
            d = s - x
            l = 0.5 * d * d
            return l, 3.0 * np.abs(l), np.abs(d) * np.abs(s)
        if kind == 'kl':
            a1, a2 = x * np.log(x + le), x * np.log(s)
            l = (a1 - a2) - x + (s - EPS)
            w = (2 * LOSS_FN + 4) * (np.abs(a1) + np.abs(a2)) + 3.0 * np.abs(x) + 2.0 * np.abs(s)
            return l, w, np.abs(s - x)
        if kind == 'is':
            xe = x + EPS
            q, lx, ls = xe / s, np.log(x + le), np.log(s)
            l = q - (lx - ls) - 1.0
            w = (LOSS_FN + 4) * np.abs(q) + (LOSS_FN + 5) * (np.abs(lx) + np.abs(ls)) + 2.0
            return l, w, np.abs(1.0 - q)
        # generic branch (0.5 and 1.5 take it too in loss mode: nmfmu_fused.h:659)
        xb = x + EPS if beta < 0 else x
        pos = xb > 0
        xs = np.where(pos, xb, 1.0)
        t1 = np.where(pos, np.power(xs, beta), 0.0)
        sb1 = np.power(s, beta - 1.0)
        t2 = sb1 * s
        den = beta * (beta - 1.0)
        T1, T2, T3 = t1 / den, (beta - 1.0) * t2 / den, -beta * xb * sb1 / den
        l = T1 + T2 + T3
        ex_x = np.abs(beta * np.log(xs))
        ex_s = np.abs((beta - 1.0) * np.log(s))
        r = _gen_roundings(beta)
        w = ((LOSS_FN + (LOSS_FN + r['mul_b']) * ex_x + (abs(beta) if beta < 0 else 0.0) + 2 + r['quot']) * np.abs(T1)
             + (LOSS_FN + (LOSS_FN + r['mul_bm1'] + r['bm1']) * ex_s + 1 + r['mul_bm1'] + r['bm1'] + 2 + r['quot']) * np.abs(T2)
             + (LOSS_FN + (LOSS_FN + r['mul_bm1'] + r['bm1']) * ex_s + r['mul_b'] + 1 + (1 if beta < 0 else 0) + 1 + r['quot'])
             * np.abs(T3))
        return l, w, np.abs(t2 - xb * sb1)


def _gen_roundings(beta: float) -> dict:
    """Which fp32 operations on the scalar beta round at all (counted, 0 or 1 each): beta - 1.f (exact for 0.5, 1.5, 3, -1, not
    for 0.3f), a multiplication by beta or by beta - 1 (exact where that is a power of two), and the quotient's
    beta * (beta - 1.f) plus its division (one ulp = 2)."""
    b = np.float32(beta)
    bm1 = np.float32(b - np.float32(1.0))
    r_bm1 = 0 if float(bm1) == float(b) - 1.0 else 1
    pow2 = lambda v: float(np.frexp(abs(float(v)))[0]) == 0.5
    r_prod = 0 if float(np.float32(b * bm1)) == float(b) * float(bm1) else 1
    return dict(bm1=r_bm1, mul_b=0 if pow2(b) else 1, mul_bm1=0 if pow2(bm1) else 1, quot=r_bm1 + r_prod + LOSS_FN)


def loss_abs_terms(s, x, beta: float):
    """sum_k |term_k| of an element (beta == 1: |x ln(x + eps)| + |x ln s| + |x| + |s|)."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    beta = float(np.float32(beta))
    kind = beta_kind(beta)
    if kind == 'euc':
        return 0.5 * (np.abs(s) + np.abs(x)) ** 2      # d = s - x is formed first: |s| + |x| is what its roundings scale with
    if kind == 'kl':
        return np.abs(x * np.log(x + EPS)) + np.abs(x * np.log(s)) + np.abs(x) + np.abs(s)
    if kind == 'is':
        return np.abs((x + EPS) / s) + np.abs(np.log(x + EPS)) + np.abs(np.log(s)) + 1.0
    xb = x + EPS if beta < 0 else x
    t1 = np.where(xb > 0, np.power(np.where(xb > 0, xb, 1.0), beta), 0.0)
    sb1 = np.power(s, beta - 1.0)
    den = abs(beta * (beta - 1.0))
    return (np.abs(t1) + np.abs((beta - 1.0) * sb1 * s) + np.abs(beta * xb * sb1)) / den


def loss_plan(N: int, C: int, R: int, precision: str, beta: float, ncu: int, nsplit=None, block_rows=None, gram=False):
    """What the loss pass of a DenseMU runs with.  It is launched on ``step_h`` (owner H, contraction over C), so tile height
    and nsplit are those the MU step's family chose; the kernel is pp on 256-row tiles and the four-wave kernel otherwise
    (sp, sp2 and xb have no loss instance: fused_dispatch tests ``mode == kModeMU`` for them, nmfmu_capi.hip:171-183).
    The loss-mode tile rule: tiles_per_split = ceil(ktiles / nsplit), rounded up to even on pp ONLY (nmfmu_capi.hip:124,
    :162) -- not to the four of sp / sp2 -- so ``tiles`` differs from ``mu_tiles`` exactly where the MU family is sp / sp2
    and ceil(ktiles / nsplit) is no multiple of four."""
    p = half_step_plan(N, C, R, precision, beta, ncu, nsplit, block_rows, gram)['h']
    fam = 'pp' if p['block_rows'] == 256 else 'fused'
    tiles = split_tiles(p['k_pad'], p['nsplit'], fam)
    return dict(M=N, K=C, R=R, m_pad=p['m_pad'], k_pad=p['k_pad'], r_pad=p['r_pad'], block_rows=p['block_rows'], family=fam,
                nsplit=p['nsplit'], tiles=tiles, tps=tiles_per_split(p['k_pad'], p['nsplit'], fam)[1],
                mu_family=p['family'], mu_tiles=p['tiles'], nparts=(p['m_pad'] // p['block_rows']) * p['nsplit'],
                tree=LOSS_TREE[fam], s_seq=s_chain(p['r_pad'], precision))


def _padded(a, rows, cols):
    out = np.zeros((rows, cols), dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _recon(A_img, B_img, m_pad, k_pad, seed):
    """A B^T + seed on the padded grid (padded rows of an image are zero: S = seed there)."""
    rk = max(A_img[0].shape[1], B_img[0].shape[1])
    pa = [_padded(a, m_pad, rk) for a in A_img if a is not None]
    pb = [_padded(b, k_pad, rk) for b in B_img if b is not None]
    return _gemm(pa, pb[0].T, pb[1].T if len(pb) == 2 else None) + seed


def loss_partials(X, A_img, B_img, beta: float, precision: str, plan: dict, *, rounding=True, x_stored=None,
                  col_mask=True, m_valid=None, eps_in_log=True, tiles=None):
    """Every partial of the loss pass, float64.  X: [M, K] fp32 target; A_img / B_img = (hi, lo or None) image values of the
    owner (H) and the panel (W), [>= M, >= R] / [>= K, >= R] (the GPU test passes the images read back, padding included;
    rounding=False: the exact factors, an exact target).  Seeded faults: ``col_mask=False`` (the ``k0 < a.K`` test dropped),
    ``m_valid`` (another row count in ``m0 < a.M``), ``eps_in_log=False`` (log(x) for log(x + eps)), ``tiles`` (another tile
    list than the plan's).  Returns a dict of arrays [nparts] -- ref, bound, abs_terms -- and n_chain [nparts]: the element
    count of the longest per-lane chain (32 per tile)."""
    M, K, m_pad, k_pad, br, ns = plan['M'], plan['K'], plan['m_pad'], plan['k_pad'], plan['block_rows'], plan['nsplit']
    kind = beta_kind(beta)
    if rounding:
        x = stored_target(X, precision).reshape(np.asarray(X).shape) if x_stored is None else np.asarray(x_stored, np.float64)
    else:
        x = np.asarray(X, dtype=np.float64)
    xp = _padded(x, m_pad, k_pad)
    S = _recon(A_img, B_img, m_pad, k_pad, 0.0 if kind == 'euc' else EPS)
    l, w, sens = loss_elem_terms(S, xp, beta, eps_in_log)
    at = loss_abs_terms(S, xp, beta)
    mv = M if m_valid is None else m_valid
    ok = (np.arange(m_pad)[:, None] < mv) & ((np.arange(k_pad)[None, :] < K) | (not col_mask))
    tl = plan['tiles'] if tiles is None else tiles
    tps = plan['tps']
    nparts = plan['nparts']
    ref, bound, abs_terms = np.zeros(nparts), np.zeros(nparts), np.zeros(nparts)
    n_chain = np.zeros(nparts, dtype=np.int64)
    cols = np.arange(k_pad)
    for mb in range(m_pad // br):
        rows = slice(mb * br, (mb + 1) * br)
        for ks in range(ns):
            nt = tl[ks]
            i = mb * ns + ks
            n_chain[i] = 32 * nt
            if nt == 0:
                continue
            t0 = ks * tps
            c = slice(t0 * KBK, (t0 + nt) * KBK)
            m = ok[rows, c]
            depth = 32 * nt - (32 * (cols[c] // KBK - t0) + cols[c] % 32) + plan['tree']
            lv = np.where(m, l[rows, c], 0.0)
            ref[i] = lv.sum()
            if rounding:
                e = LOSS_U * w[rows, c] + _gamma(depth)[None, :] * (np.abs(lv) + LOSS_U * w[rows, c]) \
                    + _gamma(plan['s_seq']) * sens[rows, c]
                abs_terms[i] = np.where(m, at[rows, c], 0.0).sum()
                bound[i] = np.where(m, e, 0.0).sum() + 2.0 ** -50 * abs_terms[i]
    return dict(ref=ref, bound=bound, abs_terms=abs_terms, n_chain=n_chain)


def partial_excess(got, ref, bound) -> np.ndarray:
    """Per partial |got - ref| / bound; a partial whose bound is zero must equal its reference (0.0) exactly; a value that
    is not finite counts as inf.  The check is ``partial_excess(...).max() <= 1``."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    diff = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


# The riding loss (PPCfg::LACC, nmfmu_pp.h:91-97): the W half-step that follows a checkpoint (owner W, contraction over N)
# accumulates, per lane, four chains of  la += x log2 s  (ONE fused multiply-add: the product is not rounded) and of
# ls += s over EVERY element of its tiles, padding included (x = 0, s = eps there): elements 2d .. 2d + 3 of S^T tile tt go to
# chains 0 .. 3 (:618-636, :687-704), eight elements per chain and tile; then (la0 + la1) + (la2 + la3), six __shfl_xor levels
# (:804-808), one pair per wave at [16 wg + 2 wave].  Wave w owns the rows 256 mb + 32 w .. + 31 and all tiles of the split.
# x is the stored target (the fp16 half of the word, or the 24-bit value of 'f16r').
#   la: the logarithm 2 U |x log2 s|; element i passes 8 nt - slot additions of its chain, 2 + 6 after it; S moves
#       x log2 s by gamma(n_seq_S) |x| / ln 2.
#   ls: the additions alike; S itself gamma(n_seq_S) s.
RIDING_TREE = 2 + 6


def riding_plan(N: int, C: int, R: int, precision: str, ncu: int, nsplit=None):
    p = half_step_plan(N, C, R, precision, 1.0, ncu, nsplit, None)['w']
    assert p['family'] == 'pp' and precision in ('f16', 'f16r')
    tps = tiles_per_split(p['k_pad'], p['nsplit'], 'pp')[1]
    return dict(M=C, K=N, R=R, m_pad=p['m_pad'], k_pad=p['k_pad'], r_pad=p['r_pad'], nsplit=p['nsplit'], tiles=p['tiles'],
                tps=tps, nwg=(p['m_pad'] // 256) * p['nsplit'], s_seq=s_chain(p['r_pad'], precision),
                n_all=p['m_pad'] * p['k_pad'])


def riding_partials(Xt, A_img, B_img, precision: str, plan: dict, x_stored=None):
    """The 8 pairs per workgroup, float64: ref [nwg, 8, 2] = (sum x log2 s, sum s) and bound [nwg, 8, 2].  Xt: [C, N] fp32 (the
    target transposed: the W half-step's rows are columns of V); A_img / B_img: image values of W and of H BEFORE the update."""
    m_pad, k_pad, ns, tps = plan['m_pad'], plan['k_pad'], plan['nsplit'], plan['tps']
    x = stored_target(Xt, precision).reshape(np.asarray(Xt).shape) if x_stored is None else np.asarray(x_stored, np.float64)
    xp = _padded(x, m_pad, k_pad)
    S = _recon((A_img[0], None), (B_img[0], None), m_pad, k_pad, EPS)
    xl = xp * np.log2(S)
    ref = np.zeros((plan['nwg'], 8, 2))
    bound = np.zeros((plan['nwg'], 8, 2))
    cols = np.arange(k_pad)
    gs = _gamma(plan['s_seq'])
    for mb in range(m_pad // 256):
        for ks in range(ns):
            nt = plan['tiles'][ks]
            if nt == 0:
                continue
            t0 = ks * tps
            c = slice(t0 * KBK, (t0 + nt) * KBK)
            kk = cols[c] % 32                                     # 16 tt + e
            slot = 8 * (cols[c] // KBK - t0) + 4 * (kk // 16) + (kk % 16) // 4
            depth = _gamma(8 * nt - slot + RIDING_TREE)[None, :]
            for wv in range(8):
                r = slice(mb * 256 + 32 * wv, mb * 256 + 32 * wv + 32)
                i = mb * ns + ks
                ref[i, wv, 0] = xl[r, c].sum()
                ref[i, wv, 1] = S[r, c].sum()
                bound[i, wv, 0] = ((LOSS_FN * LOSS_U + depth) * np.abs(xl[r, c]) + gs * np.abs(xp[r, c]) / LN2).sum() \
                    + 2.0 ** -50 * np.abs(xl[r, c]).sum()
                bound[i, wv, 1] = ((depth + gs) * S[r, c]).sum()
    return dict(ref=ref, bound=bound)


def riding_total(V, A_img, B_img, precision: str, plan: dict, x_stored=None, n_all=None):
    """(ref, bound) of the value riding_finish_kernel leaves (nmfmu_aux.hip:520-538): ref = the float64 KL of metrics.py:22
    between the fp32 target V [N, C] and the reconstruction of the images.  The kernel's value is
        A - ln 2 sum x' log2 s - C + (sum s - n_all eps)
    A = sum x ln(x + eps) and C = sum x from target_sums_kernel on the fp32 target (per element in fp32: x + eps moves the
    term by U |x|, the logarithm 2, x kLn2 2, x x 1; summed in float64), the two sums from the pairs (``riding_partials``),
    x' the STORED target.  sum s runs over all n_all = m_pad k_pad processed elements, each padded one exactly eps (its fp32
    accumulator is the seed), so sum s - n_all eps = sum over the valid elements of (s - eps).  x' != x moves the value by
    sum (x - x') ln s exactly: allowed as sum |x - x'| |ln s| from the data (<= 2^-17 sum |x ln s| for 'f16r'; zero for an
    fp16-exact target in 'f16').  ``n_all``: seeded fault (another count than the plan's)."""
    V = np.asarray(V, dtype=np.float64)
    Xt = V.T
    M, K = plan['M'], plan['K']
    xs = stored_target(Xt, precision).reshape(Xt.shape) if x_stored is None else np.asarray(x_stored, np.float64)
    S = _recon((A_img[0], None), (B_img[0], None), plan['m_pad'], plan['k_pad'], EPS)[:M, :K]
    a = Xt * np.log(Xt + EPS)
    ref = float((a - Xt * np.log(S) - Xt + (S - EPS)).sum())
    rp = riding_partials(Xt, A_img, B_img, precision, plan, x_stored=xs)
    bound = float(LOSS_U * (5.0 * np.abs(a) + np.abs(Xt)).sum() + LN2 * rp['bound'][..., 0].sum() + rp['bound'][..., 1].sum()
                  + (np.abs(Xt - xs) * np.abs(np.log(S))).sum()
                  + 2.0 ** -50 * (np.abs(a).sum() + np.abs(Xt).sum() + LN2 * np.abs(rp['ref'][..., 0]).sum()
                                  + rp['ref'][..., 1].sum()))
    kernel_value = float(a.sum() - LN2 * rp['ref'][..., 0].sum() - Xt.sum()
                         + (rp['ref'][..., 1].sum() - (plan['n_all'] if n_all is None else n_all) * EPS))
    return dict(ref=ref, bound=bound, kernel_value=kernel_value)


def beta_div_bound(x, y, beta: float):
    """(ref, bound) of metrics.beta_div(x, y, beta) on plain arrays (beta_div_kernel, nmfmu_aux.hip:558-572): s = x + eps is
    one fp32 addition (none at beta == 2), loss_elem runs in fp32 (``loss_elem_terms``' weights), the sum in float64, the
    result is rounded to fp32 once.  ref is the float64 sum of the same elements."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    s = x if beta_kind(beta) == 'euc' else x + EPS
    l, w, sens = loss_elem_terms(s, y, beta)
    ref = float(l.sum())
    at = float(loss_abs_terms(s, y, beta).sum())
    return ref, float(LOSS_U * (w + sens).sum() + LOSS_U * abs(ref) + 2.0 ** -50 * at)


def loss_cases(ncu: int):
    """The case matrix of tests/test_gpu_loss_emulated_parity.py: dicts like ``parity_cases`` plus ``gram`` (the engine is
    built with allow_gram) and ``fitted`` (V = fp32(H0 W0^T): the loss cancels completely)."""
    cases = []

    def add(group, prec, beta, N, C, R, nsplit=None, block_rows=None, stage='dma', target='rand', gram=False, fitted=False):
        tag = f'{group}-{prec}-b{beta:g}-{N}x{C}r{R}-ns{nsplit}' + (f'-{target}' if target != 'rand' else '') \
            + ('-fitted' if fitted else '')
        cases.append(dict(id=tag, group=group, family=group, precision=prec, beta=float(beta), N=N, C=C, R=R, nsplit=nsplit,
                          block_rows=block_rows, stage=stage, target=target, gram=gram, fitted=fitted))

    # ping-pong loss kernel
    for prec in ('bf16', 'f16', 'f16r'):
        add('pp', prec, 1, 1, 300, 1, 1)
        add('pp', prec, 1, 257, 1100, 33, 4)                # [6, 6, 6, 2]: odd raw tiles per split; the last split is padding only
        add('pp', prec, 1, 300, 2100, 128, None)
        add('pp', prec, 1, 300, 1000, 64, 2, target='zeros')
    add('pp', 'f16', 1, 257, 1700, 33, 6)                   # [6, 6, 6, 6, 4, 0]: an empty loss split
    # four-wave loss kernel: the shape rotation of ``parity_cases``; a case whose bound exceeds LOSS_CAP of sum |terms| takes the
    # shape's shortened contraction (LOSS_SHAPES), beta == 3 the shortest one throughout
    i = 0
    for beta in (1.0, 0.0, 0.5, 1.5, 0.3, 3.0, -1.0, 2.0):
        for prec in PRECISIONS:
            if prec == 'f16r' and beta == 2.0:
                continue
            for _ in range(len(LOSS_SHAPES)):
                k = i % len(LOSS_SHAPES)
                i += 1
                if not (prec == 'bf16x3' and pad_rank(LOSS_SHAPES[k][0][2]) > 128):
                    break
            if beta == 3.0:
                k = 0
            full, ns, short, short_betas = LOSS_SHAPES[k]
            N, C, R = short if beta in short_betas else full
            add('fused', prec, beta, N, C, R, ns, block_rows=128 if beta == 1.0 else None)
    for beta in (1.0, 0.5, 2.0):
        for prec in ('f16', 'bf16x3'):
            add('fused', prec, beta, 200, 330, 24, None, block_rows=128 if beta == 1.0 else None, target='zeros')
    add('fused', 'f16x', 1.0, 200, 330, 24, None, block_rows=128, target='zero_row')
    add('fused', 'bf16', 0.5, 100, 2304, 24, 7)             # [6] * 6 + [0]: an empty loss split, and a row block of padding only
    # the MU step is not the four-wave kernel, the loss is
    add('sp', 'f16', 1, 300, 1200, 256, 4, stage='nop2')    # MU [8, 8, 4, 0], loss [5, 5, 5, 5]
    add('sp', 'f16', 1, 300, 200, 200, None)                # MU [4], loss [4]
    for beta in (0.5, 0.0):
        add('sp2', 'f16', beta, 300, 1200, 100, 4)          # MU [8, 8, 4, 0], loss [5, 5, 5, 5]
    for prec in ('f16', 'f16x'):
        add('xb', prec, 2, 384, 700, 64, 3, gram=True)      # MU [4, 4, 4] = loss (1100 columns, [7, 7, 6], exceed the cap)
    # a fitted state: the loss cancels completely
    add('pp', 'f16r', 1, 257, 1100, 33, 4, fitted=True)
    add('fused', 'f16x', 2, 384, 700, 64, 3, fitted=True)
    return cases


# shapes of the four-wave rotation -- ``parity_cases``' four: (N, C, R), forced split, the same with a contraction short enough
# for LOSS_CAP (four tiles per split), and the betas that need it (tests/test_mu_emulation.py computes the cap for every case)
LOSS_SHAPES = [((200, 330, 24), None, (200, 250, 24), (3.0,)),
               ((384, 1100, 64), 3, (384, 700, 64), (1.5, 3.0, 2.0)),
               ((520, 700, 100), 1, (520, 250, 100), (1.0, 0.5, 1.5, 3.0, -1.0, 2.0)),
               ((300, 640, 200), 2, (300, 500, 200), (1.5, 3.0, 2.0))]


def loss_problem(case):
    """(V, W0, H0) of a loss case: ``make_problem``'s, or the fitted state V = fp32(H0 W0^T) on its factors."""
    V, W0, H0 = make_problem(case)
    if case.get('fitted'):
        V = (H0.double() @ W0.double().t()).float()
    return V, W0, H0


RIDING_CASES = [dict(id=f'{prec}-{N}x{C}r{R}-ns{ns}' + (f'-{target}' if target != 'rand' else ''), precision=prec, beta=1.0, N=N,
                     C=C, R=R, nsplit=ns, target=target, family='pp')
                for prec in ('f16', 'f16r')
                for (N, C, R, ns, target) in ((257, 1100, 33, 4, 'rand'), (300, 1000, 64, None, 'zeros'), (1, 300, 1, None, 'rand'))]


def riding_problem(case):
    """``make_problem``'s data; precision 'f16' is specified for targets fp16 holds exactly (DenseMU's admission test), so its
    target is rounded to fp16 once here -- zeros stay zeros."""
    V, W0, H0 = make_problem(case)
    if case['precision'] == 'f16':
        V = V.half().float()
    return V, W0, H0


def host_images(F, precision: str):
    """(hi, lo or None) image values of a factor, rounded on the host (the CPU tests; the GPU tests read them back)."""
    return factor_image(np.asarray(F, dtype=np.float64), precision)
