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
              A_img=None, B_img=None, ratio_round=None, x_stored=None):
    """Numerator and denominator of one half-step, float64, [rows of A] x rank.

    X: [m, k] fp32 target rows (V or V^T); A: [m, R] owner rows; B: [k, R] panel.  ``A_img`` / ``B_img`` = (hi, lo or None)
    image planes to use instead of rounding A / B (the tests pass the images read back from the GPU).  M, K: the full
    owner / contraction lengths (ki), default the shapes given.  cs_owner / cs_panel: the column sums the kernel reads
    (ki).  rounding=False: every operand exact (the plain float64 algorithm of mu_oracle).  ``ratio_round(G, split)``:
    replaces the Gn / Gp rounding (seeded-fault tests).  ``x_stored``:
    the target as the kernel holds it, used instead of ``stored_target(X, precision)`` (the convolutive engine keeps fp32
    targets in every precision: tests/conv_emulation.py).

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
    else:
        Ah, Al, Bh, Bl, x = (np.asarray(A, np.float64), None, np.asarray(B, np.float64), None, X)
    S = _gemm([Ah] if Al is None else [Ah, Al], Bh.T, None if Bl is None else Bl.T)
    if kind != 'euc':
        S = S + EPS
    ki = scale_exponent(cs_owner, cs_panel, M, K, beta, precision) if rounding else 0
    gn, gp = mu_terms(S, x, beta, ki)
    unsc = 2.0 ** -ki
    out = {'ki': ki, 'num_amb': 0.0, 'den_amb': 0.0, 'den': None}
    if not rounding:
        out['num'] = gn @ Bh
        out['den'] = None if gp is None else gp @ Bh
        return out
    rr = ratio_round or (lambda G, split: rounded_terms(G, precision, split))
    Babs = np.abs(Bh)

    def contract(G, split, key):
        ops = rr(G, split)
        res = _gemm(ops, Bh, Bl) * unsc
        if not split:       # (a hi + lo pair holds the term to 2^-16 whichever way hi went)
            flip = np.abs(round_op(G * (1 + AMBIGUITY), precision) - round_op(G * (1 - AMBIGUITY), precision))
            if flip.any():
                out[key + '_amb'] = (flip @ Babs) * unsc
        out[key] = res

    if kind == 'euc' and precision in ('bf16', 'f16'):
        out['num'] = x @ Bh                                   # the stored word is the operand (nmfmu_fused.h:690)
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
def half_step_plan(N: int, C: int, R: int, precision: str, beta: float, ncu: int, nsplit=None, block_rows=None):
    """{'w': ..., 'h': ...}: the kernel family, tile height, split and per-split tiles each half-step runs with."""
    r_pad = pad_rank(R)
    plan = {}
    for which, (m, k) in (('w', (C, N)), ('h', (N, C))):
        m_pad, k_pad = pad_rows(m), pad_rows(k)
        br = block_rows or default_block_rows(r_pad, precision, beta)
        fam = kernel_family(r_pad, precision, beta, br)
        ns = choose_nsplit(m_pad, k_pad, r_pad, precision, beta, br, ncu, nsplit)
        plan[which] = dict(M=m, K=k, m_pad=m_pad, k_pad=k_pad, block_rows=br, family=fam, nsplit=ns,
                           tps_raw=tiles_per_split(k_pad, ns, fam)[0], tiles=split_tiles(k_pad, ns, fam), r_pad=r_pad)
    return plan


def claim_holds(claim: str, p: dict, R: int) -> bool:
    """Does one half-step's plan ``p`` reach the control flow ``claim`` names?"""
    t = p['tiles']
    return {
        'empty_split': 0 in t,
        'short_last_split': len([x for x in t if x]) > 1 and 0 < [x for x in t if x][-1] < t[0],
        'odd_tps': p['nsplit'] > 1 and p['tps_raw'] % 2 == 1,
        'fused_apply': p['nsplit'] == 1,
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
    return V, W0, H0
