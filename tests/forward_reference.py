"""References and per-element checkers of the forward (reconstruct) kernels (test-only, plain numpy / torch on the CPU).

Two families:

* dense -- ``NMF.reconstruct`` / ``PLCA.reconstruct``: ``reconstruct_kernel`` (nmfmu_aux.hip), exact-fp32 MFMA.  The reference
  is the float64 product; the bound is the standard one of an fp32 dot product of R terms, ``(R + 2) u |H| |W|^T`` with
  u = 2^-24, which holds for any summation order (the argument of tests/test_gpu_autograd.py).
* convolutive -- ``NMFD / NMF2D / NMF3D / SIPLCA*.reconstruct``: ``nmfd_engine.reconstruct``, split-bf16 planes through
  ``nmfmu_gemm`` with ``EPI_F32``.  Tier 1 holds the output to what the accumulators hold by ``conv_emulation`` (hi hi + lo hi
  + hi lo of the rounded planes, no eps) within ``mu_emulation.TOL['bf16x3']``, the project's tolerance for fp32 accumulation
  order over split-bf16 planes.  Tier 2 holds it to the float64 convolution within
  ``(3 * 2^-16 + (3 K + 2) u) bound64``, K = R prod(T): the lo lo product that split bf16 never forms and the two residuals
  x - hi - lo are each at most 2^-16 of the product (the unit roundoff of bf16 is 2^-8), and the three plane products are
  fp32 dot products of K terms each.

The PLCA variants multiply ``W`` by ``Z`` in fp32 on the device before the same kernels run: ``scaled_w`` forms that product
on the CPU (one IEEE multiplication per element, the same bits), the checks above then apply with it as the left factor, and
against the true float64 ``W Z`` the one extra rounding is one more u.

The checkers take the output as an array, so the CPU tests (tests/test_forward_reference.py) can feed them faulty ones; they
raise AssertionError and return the worst ratio of error to bound.  The factors of every case come from ``dense_factors`` /
``conv_factors``, so what the CPU tests establish holds for the very inputs of tests/test_gpu_forward_parity.py.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import conv_emulation as CE
import mu_emulation as E
from oracle import mu_oracle as O

U = 2.0 ** -24
U_BF16X3 = 3 * 2.0 ** -16      # lo lo and the two residuals of the split, each <= 2^-16 of the product

# (N, C, R): the branches of reconstruct_kernel
DENSE_SHAPES = [(1, 1, 1),          # single element
                (33, 130, 7),       # scalar loads
                (130, 131, 31),     # scalar loads; last stage one column short
                (128, 128, 32),     # exact tile, one stage
                (129, 127, 36),     # float4 path; second stage holds 4 columns
                (257, 129, 64),     # two whole stages; three row tiles
                (300, 257, 33),     # ragged rows and columns
                (200, 90, 256)]     # widest rank
PLCA_SHAPES = [(33, 130, 7), (129, 127, 36), (300, 257, 33)]


def _prod(xs):
    return int(np.prod(xs, dtype=np.int64)) if len(xs) else 1


# ---- inputs ----------------------------------------------------------------------------------------------------------
def dense_factors(shape, kind='rand'):
    """(H (N, R), W (C, R)) fp32 CPU tensors.  kind: 'rand' (non-negative), 'randn' (signed), 'int' (integers 0..15),
    'zeros' ('rand' with row N // 2 of H and row C // 3 of W all zero)."""
    N, C, R = shape
    g = torch.Generator().manual_seed(N * 7 + C * 3 + R + {'rand': 0, 'randn': 1, 'int': 2, 'zeros': 3}[kind] * 1009)
    if kind == 'int':
        return (torch.randint(0, 16, (N, R), generator=g).float(), torch.randint(0, 16, (C, R), generator=g).float())
    draw = torch.randn if kind == 'randn' else torch.rand
    H, W = draw(N, R, generator=g), draw(C, R, generator=g)
    if kind == 'zeros':
        H[N // 2] = 0.0
        W[C // 3] = 0.0
    return H, W


def conv_factors(shape, kind='rand'):
    """(H (B, R, *lh), W (C, R, *taps)) fp32 CPU tensors of a case (B, C, R, lh, taps).  kind: 'rand', 'int' (integers
    0..15, exact in bf16) or 'zeros' ('rand' with channel C // 3 of W and rank R - 1 of H silent)."""
    B, C, R, lh, taps = shape
    g = torch.Generator().manual_seed(B * 7 + C * 3 + R + 11 * _prod(lh) + 13 * _prod(taps)
                                      + {'rand': 0, 'int': 2, 'zeros': 3}[kind] * 1009)
    if kind == 'int':
        return (torch.randint(0, 16, (B, R, *lh), generator=g).float(),
                torch.randint(0, 16, (C, R, *taps), generator=g).float())
    H, W = torch.rand(B, R, *lh, generator=g), torch.rand(C, R, *taps, generator=g)
    if kind == 'zeros':
        W[C // 3] = 0.0
        H[:, R - 1] = 0.0
    return H, W


def rank_weights(R, seed=17):
    """Z (R,) fp32 of the PLCA cases: positive, not normalised (``reconstruct`` is a static function of its arguments)."""
    return torch.rand(R, generator=torch.Generator().manual_seed(seed + R)) + 0.25


def scaled_w(W, Z):
    """fp32(W * Z) along the rank axis: the left factor ``plca._plca_forward`` / ``_conv_reconstruct`` form on the device."""
    W, Z = torch.as_tensor(W, dtype=torch.float32), torch.as_tensor(Z, dtype=torch.float32)
    return W * Z.view(1, -1, *([1] * (W.dim() - 2)))


def _t64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def _wz64(W, Z):
    W, Z = _t64(W), _t64(Z)
    return W * Z.view(1, -1, *([1] * (W.dim() - 2)))


# ---- dense -----------------------------------------------------------------------------------------------------------
def dense_ref(H, W):
    """(float64 H W^T, bound64 = |H| |W|^T); leading dimensions of H are flattened."""
    W64 = np.asarray(W, dtype=np.float64)
    H64 = np.asarray(H, dtype=np.float64).reshape(-1, W64.shape[1])
    return H64 @ W64.T, np.abs(H64) @ np.abs(W64).T


def plca_dense_ref(H, W, Z):
    """(ref64, bound64) of the true float64 H (W Z)^T, W and Z fp32 values."""
    return dense_ref(H, _wz64(W, Z).numpy())


def _within(got, ref, bound, what):
    """Assert |got - ref| <= bound per element (a NaN fails; bound == 0 means exactly ref); the worst error / bound."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio.max())
    assert worst <= 1.0, f'{what}: {int((ratio > 1.0).sum())} of {ratio.size} elements off, worst error / bound = {worst:.4g}'
    return worst


def check_dense(got, H, W, Z=None):
    """Per element |got - ref64| <= (R + 2) u bound64; an element with bound64 == 0 must be exactly 0.  With ``Z`` the
    reference is the true float64 H (W Z)^T of fp32 W and Z, and the rounding of W * Z to fp32 is one more u."""
    R = np.shape(W)[1]
    ref, bound = dense_ref(H, W) if Z is None else plca_dense_ref(H, W, Z)
    return _within(got, ref, (R + (2 if Z is None else 3)) * U * bound, 'dense forward')


# ---- convolutive -----------------------------------------------------------------------------------------------------
ConvFigures = namedtuple('ConvFigures', 'ratio elem_err')      # worst tier-2 error / bound, worst tier-1 elem_err


def _conv64(H, W):
    H, W = _t64(H), _t64(W)
    return (O.nmfd_reconstruct(H, W) if H.dim() == 3 else O.convnd_reconstruct(H, W)).numpy()


def from_w(S, B, ls):
    """[C][(b, l)] -> (B, C, *ls), the inverse of ``conv_emulation.target_w``."""
    S = np.asarray(S)
    return np.moveaxis(S.reshape((S.shape[0], B) + tuple(ls)), 0, 1)


def conv_ref(H, W):
    """(float64 convolution (B, C, *ls), the emulated accumulator values in the same shape, bound64 = the same contraction
    of |W| and |H|)."""
    Hn, Wn = np.asarray(H, dtype=np.float32), np.asarray(W, dtype=np.float32)
    B, _, _, _, _, ls = CE.geometry(Wn, Hn)
    em = CE.reconstruction(CE.operands(Wn, Hn, 'bf16x3'), 2)
    return _conv64(Hn, Wn), from_w(em, B, ls), _conv64(np.abs(Hn), np.abs(Wn))


def conv_k(W):
    return _prod(np.shape(W)[1:])                     # K = R prod(T)


def conv_tier1(got, em):
    """``elem_err`` of the output against the emulated accumulators, both [C][(b, l)], within TOL['bf16x3']."""
    em = np.asarray(em, dtype=np.float64)
    worst = float(E.elem_err(CE.target_w(np.asarray(got, dtype=np.float64).reshape(em.shape)), CE.target_w(em)).max())
    assert worst <= E.TOL['bf16x3'], f'conv forward against the emulation: worst elem_err {worst:.4g} > {E.TOL["bf16x3"]:g}'
    return worst


def conv_tier2(got, ref, bound, K, extra_u=0):
    """|got - ref64| <= (3 * 2^-16 + (3 K + 2 + extra_u) u) bound64 per element."""
    return _within(got, ref, (U_BF16X3 + (3 * K + 2 + extra_u) * U) * bound, 'conv forward against float64')


def check_conv(got, H, W, Z=None):
    """Both tiers for the output of ``reconstruct(H, W)``; with ``Z``, of ``reconstruct(H, W, Z)``: the same two tiers with
    ``scaled_w(W, Z)`` as the left factor, and tier 2 once more against the true float64 W Z with one more u."""
    Wl = W if Z is None else scaled_w(W, Z).numpy()
    ref, em, bound = conv_ref(H, Wl)
    err = conv_tier1(got, em)
    ratio = conv_tier2(got, ref, bound, conv_k(Wl))
    if Z is not None:
        wz = _wz64(W, Z).numpy()
        ratio = max(ratio, conv_tier2(got, _conv64(H, wz), _conv64(np.abs(np.asarray(H, dtype=np.float64)), np.abs(wz)),
                                      conv_k(Wl), extra_u=1))
    return ConvFigures(ratio, err)


def fp32_accumulations(ops):
    """The emulated reconstruction [c][(b, l)] accumulated in numpy float32 in k-chunks of 16, ascending and descending: the
    two orders ``conv_emulation.fp32_order_error`` measures, as arrays (what an honest kernel may return)."""
    (wh, wl), (hh, hl) = ops['Wm'], ops['Hu']
    K = wh.shape[1]
    out = []
    for order in (1, -1):
        acc = np.zeros((wh.shape[0], hh.shape[0]), dtype=np.float32)
        for k0 in list(range(0, K, 16))[::order]:
            for a, b in ((wh, hh), (wl, hh), (wh, hl)):
                acc = acc + (a[:, k0:k0 + 16].astype(np.float32) @ b[:, k0:k0 + 16].T.astype(np.float32))
        out.append(acc)
    return out
