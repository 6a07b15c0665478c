"""``torchnmf.metrics``-compatible divergences, evaluated on the ROCm device.

Reference: torchnmf/metrics.py:6-96.  ``input`` is the reconstruction, ``target``
the data.  Each call launches one fused elementwise-reduction HIP kernel
(``nmfmu_beta_div``) and returns a 0-dim float32 tensor on the inputs' device;
there is no CPU path.  The divergences are differentiable with respect to
``input`` (``torch.autograd``, first order): when it requires grad the result
carries a ``grad_fn`` whose backward is one elementwise HIP kernel
(``nmfmu_beta_div_grad``).  ``target`` is always a constant: no gradient flows
to it, whether or not it requires grad.

``sparse_beta_div(H, W, target, beta)`` is the same divergence between
``H @ W.T`` and a sparse-COO target, computed from the stored entries only
(beta in {1, 2}; ``sparse_autograd.py``): differentiable with respect to both
factors, with HIP backward kernels (``nmfmu_sp_div_backward``).  With
``unstored='missing'`` the unstored entries are unknown instead of zero: the
reference's ``beta_div`` over the stored entries alone, for any beta
(``nmfmu_sp_masked_loss`` / ``nmfmu_sp_masked_terms``).

``score_pairs`` / ``topk_scores`` (``scoring.py``) use a fitted model without the ``N x C`` product: its value at
(row, column) pairs, and the ``k`` best admissible columns per row.  ``fold_in`` (``fold_in.py``) gives ``H`` for rows that
were not in the training target, with ``W`` fixed.

``weighted_beta_div(H, W, V, weights, beta)`` (``wmu.py``) is the divergence between ``H @ W.T`` and a DENSE target with dense
per-entry weights (a mask, exposures, confidences), for any beta, without the ``N x C`` product and differentiable with respect
to both factors (``nmfmu_wmu_loss`` / ``nmfmu_wmu_terms``): the loss ``NMF.fit(V, weights=...)`` minimises.

``batched_beta_div(H, W, V, beta)`` (``batched.py``) is ``beta_div`` for every problem of a batch ``H [B, N, R]``, ``W [B, C, R]``
at once, float64 ``[B]``, without the ``B`` reconstructions (``nmfmu_bmu_loss``): the loss ``BatchedNMF.fit`` tracks.  With
``weights`` (and ``weight_index``) it is the weighted divergence per problem (``nmfmu_bwmu_loss``): what
``BatchedNMF.fit(V, weights=...)`` tracks and ``model_selection.cross_validate`` scores held-out entries with.

``separate(H, W, V, groups, power=...)`` (``separation.py``) is what follows a fit on a spectrogram: the soft mask of every group
of components, or the mixture (real, or the complex STFT) times it, on one fused kernel (``nmfmu_separate``).
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _capi
from .sparse_autograd import SparseTarget, sparse_beta_div
from .scoring import rank_scores, ranking_metrics, score_pairs, topk_scores
from .fold_in import fold_in, fold_in_cd
from .wmu import WeightedTarget, weighted_beta_div
from .batched import batched_beta_div
from .separation import separate

__all__ = ['kl_div', 'euclidean', 'is_div', 'beta_div', 'sparseness', 'SparseTarget', 'sparse_beta_div', 'score_pairs',
           'topk_scores', 'rank_scores', 'ranking_metrics', 'fold_in', 'fold_in_cd', 'WeightedTarget', 'weighted_beta_div',
           'batched_beta_div', 'separate', 'ard_objective']


def _beta_div_value(input: Tensor, target: Tensor, beta: float) -> Tensor:
    lib = _capi.load()
    x = input.detach().float().contiguous().reshape(-1)
    y = target.detach().float().contiguous().reshape(-1)
    part = torch.empty(1024, dtype=torch.float64, device=x.device)
    out = torch.zeros(1, dtype=torch.float64, device=x.device)
    _capi.check(lib.nmfmu_beta_div(x.data_ptr(), y.data_ptr(), x.numel(), float(beta), part.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), 'nmfmu_beta_div')
    return out[0].float()


class _BetaDivFn(torch.autograd.Function):
    """The value from the same ``nmfmu_beta_div`` launch as without autograd; the gradient with respect to ``input`` from
    ``nmfmu_beta_div_grad``, which reads the 0-dim incoming gradient on the device (no host sync)."""

    @staticmethod
    def forward(ctx, input, target, beta):
        ctx.save_for_backward(input, target)
        ctx.beta = float(beta)
        return _beta_div_value(input, target, beta)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        input, target = ctx.saved_tensors
        lib = _capi.load()
        x = input.detach().float().contiguous().reshape(-1)
        y = target.detach().float().contiguous().reshape(-1)
        up = g.detach().float().reshape(1).contiguous()
        gx = torch.empty_like(x)
        _capi.check(lib.nmfmu_beta_div_grad(x.data_ptr(), y.data_ptr(), x.numel(), ctx.beta, up.data_ptr(), gx.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), 'nmfmu_beta_div_grad')
        return gx.reshape(input.shape).to(input.dtype), None, None


def beta_div(input: Tensor, target: Tensor, beta: float = 2) -> Tensor:
    """beta-divergence (metrics.py:60-96); beta = 2 / 1 / 0 are the Euclidean, KL and Itakura-Saito cases.
    Differentiable with respect to ``input``; ``target`` is a constant."""
    if input.device.type != 'cuda' or target.device.type != 'cuda':
        raise _capi.NmfmuError('beta_div: tensors must live on the ROCm device (no CPU fallback)')
    assert input.shape == target.shape, 'input and target must have the same shape'
    if torch.is_grad_enabled() and input.requires_grad:
        return _BetaDivFn.apply(input, target, beta)
    return _beta_div_value(input, target, beta)


def kl_div(input: Tensor, target: Tensor) -> Tensor:
    """Generalised Kullback-Leibler divergence = beta_div(beta=1) (metrics.py:6-22)."""
    return beta_div(input, target, 1)


def euclidean(input: Tensor, target: Tensor) -> Tensor:
    """Half squared Euclidean distance = beta_div(beta=2) (metrics.py:25-39)."""
    return beta_div(input, target, 2)


def is_div(input: Tensor, target: Tensor) -> Tensor:
    """Itakura-Saito divergence = beta_div(beta=0) (metrics.py:42-57)."""
    return beta_div(input, target, 0)


def ard_objective(H: Tensor, W: Tensor, V: Tensor, lam: Tensor, beta: float, prior: str, phi: float, a: float,
                  b: float) -> Tensor:
    """The objective ``NMF.fit_ard`` minimises (``ard.py``), 0-dim float64 on the inputs' device, not differentiable::

        beta_div(H W^T, V) / phi + sum_k [ (f(W[:, k]) + f(H[:, k]) + b) / lam_k + c log lam_k ]

    ``f = ||.||_1``, ``c = N + C + a + 1`` (prior 'l1'); ``f = 1/2 ||.||^2``, ``c = (N + C) / 2 + a + 1`` ('l2').  Plain
    float64 torch arithmetic with the reference's eps conventions (metrics.py:22, 56-57, 85-88): a check of the fit, not a
    part of it -- it forms the ``N x C`` product."""
    from .ard import ard_c, check_prior
    from .constants import eps
    check_prior(prior, a)
    beta = float(beta)
    with torch.no_grad():
        H64, W64, y = H.detach().double(), W.detach().double(), V.detach().double()
        x = H64 @ W64.t()
        if beta == 2:
            div = 0.5 * ((x - y) ** 2).sum()
        elif beta == 1:
            div = (y * ((y + eps).log() - (x + eps).log())).sum() - y.sum() + x.sum()
        elif beta == 0:
            q = (y + eps) / (x + eps)
            div = (q - q.log()).sum() - y.numel()
        else:
            xe, yf = x + eps, (y + eps if beta < 0 else y)
            div = (yf.pow(beta).sum() + (beta - 1) * xe.pow(beta).sum() - beta * (yf * xe.pow(beta - 1)).sum()) / (beta * (beta - 1))
        f = (lambda t: t.sum(0)) if prior == 'l1' else (lambda t: 0.5 * (t * t).sum(0))
        lam64 = lam.detach().double()
        c = ard_c(H.shape[0], W.shape[0], float(a), prior)
        return div / float(phi) + ((f(W64) + f(H64) + float(b)) / lam64 + c * lam64.log()).sum()


def sparseness(x: Tensor) -> Tensor:
    """Hoyer's sparseness measure ``(sqrt(N) - |x|_1 / |x|_2) / (sqrt(N) - 1)`` (metrics.py:99-115)."""
    if x.device.type != 'cuda':
        raise _capi.NmfmuError('sparseness: tensors must live on the ROCm device (no CPU fallback)')
    lib = _capi.load()
    xf = x.detach().float().contiguous().reshape(-1)
    part = torch.empty(1024, dtype=torch.float64, device=x.device)
    out = torch.zeros(2, dtype=torch.float64, device=x.device)
    _capi.check(lib.nmfmu_norms(xf.data_ptr(), xf.numel(), part.data_ptr(), out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), 'nmfmu_norms')
    n = xf.numel()
    return ((n ** 0.5 - out[0] / out[1].sqrt()) / (n ** 0.5 - 1)).float()
