"""Weighted NMF on a dense target: ``NMF.fit(V, weights=M)``, ``metrics.weighted_beta_div``.

``L = sum_ij m_ij d_beta(v_ij | y_ij)`` with ``y = H W^T`` and dense ``m >= 0``: a mask (bool), counts or exposures (integer)
or per-entry confidences (floating).  The multiplicative update is the reference's (nmf.py:61-92) with both backward seeds
multiplied by ``m``; where ``m == 0`` the entry is selected away, so ``V`` may hold anything there (``NaN`` marks missing
data).  One half-step is one ``nmfmu_wmu_step`` call on the fp32 masters: a fused exact-fp32 MFMA kernel that forms ``y``,
the seeds and both contractions per tile -- nothing of size ``N x C`` is written (csrc/nmfmu_wmu.hip).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _capi
from .constants import eps
from .engine import mu_gamma

MAX_RANK = 256


def check_weights(V: Tensor, weights) -> Tensor:
    """``weights`` as ``fit`` and ``weighted_beta_div`` accept it, converted to contiguous fp32 once: a tensor of ``V``'s
    shape on ``V``'s device, bool, integer or floating, every value finite and >= 0.  ``ValueError`` otherwise."""
    if not isinstance(weights, Tensor):
        raise ValueError(f'weights must be a tensor of the shape of V, got {type(weights).__name__}')
    if weights.is_sparse or tuple(weights.shape) != tuple(V.shape):
        raise ValueError(f'weights must be a dense tensor of the shape of V {tuple(V.shape)}, got '
                         f'{"a sparse tensor of shape " if weights.is_sparse else ""}{tuple(weights.shape)}')
    if weights.device != V.device:
        raise ValueError(f'weights live on {weights.device}, V on {V.device}')
    if weights.is_complex() or not (weights.dtype == torch.bool or weights.dtype.is_floating_point
                                    or weights.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
        raise ValueError(f'weights must be bool, integer or floating, got {weights.dtype}')
    M = weights.detach().float().contiguous()
    if M.numel() and not bool((torch.isfinite(M) & (M >= 0)).all().item()):
        raise ValueError('weights must be finite and non-negative (0 marks an entry that is left out)')
    return M


class WeightedTarget:
    """A dense target with its weights, prepared once: contiguous fp32 ``V`` and ``M`` (N, C), the two flags of
    nmf.py:329-336 over the WEIGHTED entries only, and the terms of the loss that hold ``v`` alone per beta."""

    def __init__(self, V: Tensor, weights):
        if V.is_sparse or V.dim() != 2:
            raise ValueError('a weighted target is a dense 2-D tensor')
        self.M = check_weights(V, weights)
        self.V = V.detach().float().contiguous()
        self.shape, self.device = tuple(V.shape), V.device
        sel = self.M > 0
        vs = self.V[sel]
        self.bad = bool((~(vs >= 0)).any().item()) if vs.numel() else False      # negative or NaN where it counts
        self.has_zero = bool((vs == 0).any().item()) if vs.numel() else False
        self._sel, self._v_term = sel, {}

    def v_term(self, beta: float) -> float:
        """``sum m * (the terms of metrics.beta_div that hold v alone)`` (metrics.py:22, 39, 57, 85-96) in float64 over the
        weighted entries -- what ``nmfmu_wmu_loss`` takes as ``v_term``.  Once per (target, beta); a Python float."""
        if beta not in self._v_term:
            if beta == 2.0:
                t = 0.0
            else:
                vd = torch.where(self._sel, self.V, torch.ones((), device=self.device)).double()
                md = self.M.double()
                if beta == 1.0:
                    t = md * (vd * (vd + eps).log() - vd)
                elif beta == 0.0:
                    t = md * (-(vd + eps).log() - 1.0)
                else:
                    t = md * (vd + eps if beta < 0 else vd).pow(beta)
                t = float(t.sum().item())
            self._v_term[beta] = t
        return self._v_term[beta]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32(x: Tensor) -> Tensor:
    return x.detach().float().contiguous()


def workspace_floats(rows: int, contraction: int, r_pad: int, nsplit: int = 0) -> int:
    return int(_capi.load().nmfmu_wmu_ws(rows, contraction, r_pad, nsplit))


def _wmu_call(T: WeightedTarget, side: str, owner: Tensor, panel: Tensor, beta: float, step=None, nsplit: int = 0,
              _fill=None, _ws=None):
    """``nmfmu_wmu_terms`` (``step`` None: returns (num, den), fp32 ``[owner rows, r_pad]``) or ``nmfmu_wmu_step`` (``step`` =
    (l1, l2, gamma): ``owner`` updated in place).  ``owner`` / ``panel``: contiguous fp32 ``[rows, R]``.  Enqueued only.
    ``_fill``: tests pre-fill the outputs and the workspace with it."""
    lib = _capi.load()
    N, Cc = T.shape
    rows, R = owner.shape
    w_side = side == 'w'
    assert rows == (Cc if w_side else N) and tuple(panel.shape) == ((N if w_side else Cc), R)
    r_pad = lib.nmfmu_pad_rank(R)
    n_float = lib.nmfmu_wmu_ws(rows, N if w_side else Cc, r_pad, nsplit)
    ws = _ws if _ws is not None else torch.empty(max(n_float, 1), dtype=torch.float32, device=T.device)
    assert ws.numel() >= n_float
    if _fill is not None:
        ws.fill_(_fill)
    head = (T.V.data_ptr(), T.M.data_ptr(), Cc, N, Cc, int(w_side), owner.data_ptr(), panel.data_ptr(), R, r_pad, beta)
    if step is not None:
        l1, l2, gamma = step
        _capi.check(lib.nmfmu_wmu_step(*head, l1, l2, gamma, nsplit, ws.data_ptr(), _stream()), 'nmfmu_wmu_step')
        return None
    num = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    den = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    _capi.check(lib.nmfmu_wmu_terms(*head, nsplit, ws.data_ptr(), num.data_ptr(), den.data_ptr(), _stream()),
                'nmfmu_wmu_terms')
    return num, den


def _wmu_loss(Hc: Tensor, Wc: Tensor, T: WeightedTarget, beta: float, part=None, out=None) -> Tensor:
    """The weighted loss as a 1-element float64 device tensor.  Enqueued only (the terms of v alone are cached on the target
    after their first use)."""
    lib = _capi.load()
    N, Cc = T.shape
    if part is None:
        part = torch.empty(lib.nmfmu_wmu_loss_parts(N, Cc), dtype=torch.float64, device=T.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=T.device)
    _capi.check(lib.nmfmu_wmu_loss(T.V.data_ptr(), T.M.data_ptr(), Cc, N, Cc, Hc.data_ptr(), Wc.data_ptr(), Hc.shape[1], beta,
                                   T.v_term(beta), part.data_ptr(), out.data_ptr(), _stream()), 'nmfmu_wmu_loss')
    return out


class WeightedMU:
    """The engine of ``NMF.fit(V, weights=M)``: ``DenseMU``'s four methods (target_flags / w_step / h_step / divergence) on a
    dense target with dense weights.

    ``V``, ``M``: (N, C) on the device (or a ready-made ``WeightedTarget`` as ``V`` with ``M`` None).  ``W`` (C, R) / ``H``
    (N, R): the contiguous fp32 masters, updated in place -- no operand images, no column sums, exact fp32 arithmetic.  A
    half-step is one ``nmfmu_wmu_step`` call."""
    precision_name = 'fp32'

    def __init__(self, V, M, W, H, beta, l1=0.0, l2=0.0, update_W=True, update_H=True, nsplit: int = 0):
        self.beta = float(beta)
        T = V if isinstance(V, WeightedTarget) else WeightedTarget(V, M)
        N, Cc = T.shape
        R = W.shape[1]
        assert W.shape == (Cc, R) and H.shape == (N, R)
        if R > MAX_RANK:
            raise NotImplementedError(f'weights: rank {R} > {MAX_RANK}, the limit of the exact-fp32 kernels')
        for f in (W, H):
            assert f.dtype == torch.float32 and f.is_contiguous() and f.device == T.device, \
                'WeightedMU works on contiguous fp32 masters on the target\'s device'
        self.T, self.W, self.H = T, W, H
        self.update_W, self.update_H = bool(update_W), bool(update_H)
        self.reg = (float(l1), float(l2), mu_gamma(self.beta))
        self.nsplit = int(nsplit)
        lib, dev = _capi.load(), T.device
        r_pad = lib.nmfmu_pad_rank(R)
        n_ws = max(lib.nmfmu_wmu_ws(N, Cc, r_pad, self.nsplit), lib.nmfmu_wmu_ws(Cc, N, r_pad, self.nsplit))
        self.ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        self.loss_part = torch.empty(lib.nmfmu_wmu_loss_parts(N, Cc), dtype=torch.float64, device=dev)
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=dev)

    def target_flags(self):
        return self.T.bad, self.T.has_zero

    def w_step(self):
        if self.update_W:
            _wmu_call(self.T, 'w', self.W, self.H, self.beta, step=self.reg, nsplit=self.nsplit, _ws=self.ws)

    def h_step(self):
        if self.update_H:
            _wmu_call(self.T, 'h', self.H, self.W, self.beta, step=self.reg, nsplit=self.nsplit, _ws=self.ws)

    def divergence(self) -> float:
        """The weighted loss.  One host sync."""
        return float(_wmu_loss(self.H, self.W, self.T, self.beta, self.loss_part, self.loss_out).item())


class _WeightedBetaDivFn(torch.autograd.Function):
    """The weighted loss; both gradients are up (den - num) of one ``nmfmu_wmu_terms`` call per wanted side."""

    @staticmethod
    def forward(ctx, H, W, T, beta):
        ctx.save_for_backward(H, W)
        ctx.T, ctx.beta = T, beta
        return _wmu_loss(_f32(H), _f32(W), T, beta)[0].float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        H, W = ctx.saved_tensors
        Hc, Wc = _f32(H), _f32(W)
        up = g.detach().float()
        R = H.shape[1]

        def grad(side, owner, panel, like):
            num, den = _wmu_call(ctx.T, side, owner, panel, ctx.beta)
            return (up * (den - num))[:, :R].to(like.dtype)
        gH = grad('h', Hc, Wc, H) if ctx.needs_input_grad[0] else None
        gW = grad('w', Wc, Hc, W) if ctx.needs_input_grad[1] else None
        return gH, gW, None, None


def weighted_beta_div(H: Tensor, W: Tensor, V, weights: Optional[Tensor] = None, beta: float = 2) -> Tensor:
    """``sum_ij weights_ij * d_beta(V_ij | (H @ W.T)_ij)`` with the reference's ``beta_div`` terms, without the N x C product.

    ``H`` is (N, R), ``W`` (C, R), rank <= 256; ``V`` a dense (N, C) tensor with ``weights`` of its shape (bool, integer or
    floating, >= 0), or a ``WeightedTarget`` prepared once (``weights`` None).  Entries of weight 0 count for nothing whatever
    ``V`` holds there; beta <= 0 needs strictly positive ``V`` wherever the weight is positive.  Returns a 0-dim float32 device
    tensor, differentiable with respect to ``H`` and ``W`` (first order): ``grad = up * (den - num)`` of the weighted update's
    terms -- at beta <= 0 the loss adds eps to the target and the update rule does not, so there the gradient misses
    ``eps / (y + eps)^(2 - beta)`` per entry."""
    beta = float(beta)
    assert H.dim() == 2 and W.dim() == 2 and H.shape[1] == W.shape[1], 'H must be (N, R) and W (C, R)'
    if isinstance(V, WeightedTarget):
        assert weights is None, 'a WeightedTarget carries its weights'
        T = V
    else:
        if V.is_sparse:
            raise NotImplementedError("weighted_beta_div takes a dense target; for a sparse one use "
                                      "sparse_beta_div(..., unstored='missing')")
        assert tuple(V.shape) == (H.shape[0], W.shape[0]), \
            f'target {tuple(V.shape)} does not match H {tuple(H.shape)} and W {tuple(W.shape)}'
        T = WeightedTarget(V, weights)          # (validates the weights: ValueError before anything else)
    if H.shape[1] > MAX_RANK:
        raise NotImplementedError(f'weighted_beta_div: rank {H.shape[1]} > {MAX_RANK}, the limit of the exact-fp32 kernels')
    if H.device.type != 'cuda' or W.device.type != 'cuda':
        raise _capi.NmfmuError('weighted_beta_div: tensors must live on the ROCm device (no CPU fallback)')
    assert tuple(T.shape) == (H.shape[0], W.shape[0]) and H.device == W.device == T.device, \
        'H, W and the target must match and live on the same device'
    if not (H.dtype.is_floating_point and W.dtype.is_floating_point):
        raise NotImplementedError(f'factors must be floating point; got H {H.dtype}, W {W.dtype}')
    assert not T.bad, 'Target should be non-negative.'
    if beta <= 0 and T.has_zero:
        raise ValueError('When beta <= 0 and V contains zeros, the training process may diverge. '
                         'Please add small values to V, or use a positive beta value.')
    if torch.is_grad_enabled() and (H.requires_grad or W.requires_grad):
        return _WeightedBetaDivFn.apply(H, W, T, beta)
    return _wmu_loss(_f32(H), _f32(W), T, beta)[0].float()
