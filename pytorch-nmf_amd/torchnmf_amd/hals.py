"""HALS -- cyclic coordinate descent on the Frobenius objective (Cichocki & Phan 2009; the update of sklearn's NMF solver
'cd') -- behind ``NMF.fit(V, beta=2, solver='hals')``.

For beta = 2 a half-step of the multiplicative update already forms ``A = X_owner @ panel`` and ``G = panel^T panel`` and is
bound by HBM; HALS needs exactly those two and replaces the elementwise apply with a Gauss-Seidel sweep over the rank

    for r = 0 .. R-1:   F[:, r] = max(eps, (A[:, r] - l1 - sum_{j != r} F[:, j] G[j, r]) / (G[r, r] + l2 + eps))

which reaches in a handful of iterations the loss MU needs hundreds for.  The sweep is one HIP kernel
(``nmfmu_hals_sweep``: one lane per row, the rows of a wave in LDS); ``hals_sweep`` is its public face, ``HalsEngine`` the
engine ``fit`` drives.  fp32 throughout; there is no CPU path.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _capi
from .constants import eps

__all__ = ['hals_sweep', 'HalsEngine']

MAX_RANK = 256           # the limit of the sparse kernels (and of the sweep's LDS residency)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _sweep(F: Tensor, A: Tensor, lda: int, G: Tensor, l1: float, l2: float) -> None:
    _capi.check(_capi.load().nmfmu_hals_sweep(F.data_ptr(), F.shape[0], F.shape[1], A.data_ptr(), lda, G.data_ptr(),
                                              l1, l2, _stream()), 'nmfmu_hals_sweep')


@torch.no_grad()
def hals_sweep(F: Tensor, A: Tensor, G: Tensor, l1: float = 0.0, l2: float = 0.0) -> Tensor:
    """One coordinate-descent pass over the rank on ``F [rows, R]``, in place (contiguous fp32, on the ROCm device), every row
    on its own: for r = 0 .. R-1, ``F[:, r] = max(eps, (A[:, r] - l1 - sum_{j != r} F[:, j] G[j, r]) / (G[r, r] + l2 + eps))``.

    ``A [rows, >= R]``: fp32 with unit stride along the rank, read through its row stride (a padded numerator plane goes in
    as a view).  ``G [R, R]``: fp32 contiguous and symmetric (``panel^T panel``).  Neither is written.  Returns ``F``.
    Raises ``NmfmuError`` for CPU tensors, ``NotImplementedError`` above rank 256."""
    for t, what in ((F, 'F'), (A, 'A'), (G, 'G')):
        if t.device.type != 'cuda':
            raise _capi.NmfmuError(f'hals_sweep: {what} lives on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'the tensors with .cuda() (there is no CPU fallback)')
        if t.dtype != torch.float32:
            raise TypeError(f'hals_sweep: {what} must be float32, got {t.dtype}')
        if t.device != F.device:
            raise ValueError(f'hals_sweep: {what} lives on {t.device}, F on {F.device}')
    if F.dim() != 2 or not F.is_contiguous():
        raise ValueError('hals_sweep: F must be a contiguous 2-D tensor (it is updated in place)')
    rows, R = F.shape
    if A.dim() != 2 or A.shape[0] != rows or A.shape[1] < R or (A.shape[1] > 1 and A.stride(1) != 1) \
            or (rows > 1 and A.stride(0) < R):
        raise ValueError(f'hals_sweep: A must be [{rows}, >= {R}] with unit stride along the rank, got {tuple(A.shape)} '
                         f'with strides {A.stride()}')
    if tuple(G.shape) != (R, R) or not G.is_contiguous():
        raise ValueError(f'hals_sweep: G must be a contiguous [{R}, {R}] matrix, got {tuple(G.shape)}')
    if R > MAX_RANK:
        raise NotImplementedError(f'hals_sweep: rank {R} > {MAX_RANK}')
    if rows == 0 or R == 0:
        return F
    _sweep(F.detach(), A.detach(), A.stride(0) if rows > 1 else max(A.shape[1], R), G.detach(), float(l1), float(l2))
    return F


class HalsEngine:
    """The interface ``fit`` drives (``target_flags`` / ``w_step`` / ``h_step`` / ``divergence``) with HALS half-steps, beta = 2.

    ``W (C, R)`` / ``H (N, R)``: the contiguous fp32 masters, updated in place.  Before the first half-step or loss the factors
    are scaled once by the scalar that minimises ``|V - a H W^T|`` (``a = <V W, H> / <H^T H, W^T W>``, float64 dots; both
    trainable: each times sqrt(a), one: that one times a; skipped unless a is finite and positive) and the trainable ones
    clamped to >= eps: from the modules' unscaled |randn| start the first sweep would floor most entries.

    Sparse ``V``: CSR / CSC set-up, numerator (``nmfmu_sp_partial``), Gram matrix and the ``V_norm + pos - neg`` loss are
    ``SparseMU``'s, exact fp32, O(nnz R).  Dense ``V``: the numerators ``V W`` / ``V^T H`` are ``nmfmu_reconstruct_backward`` with
    ``g = V`` (exact-fp32 MFMA, V read in place), the loss is ``1/2 |V|^2 - <V W, H> + 1/2 <W^T W, H^T H>`` with float64 dots --
    nothing of size N x C is allocated."""
    precision_name = 'fp32'

    def __init__(self, V: Tensor, W: Tensor, H: Tensor, l1: float = 0.0, l2: float = 0.0, update_W: bool = True,
                 update_H: bool = True):
        for t in (V, W, H):
            if t.device.type != 'cuda':
                raise _capi.NmfmuError(f'HalsEngine: tensors live on {t.device}; torchnmf_amd computes on an MI355X only '
                                       f'(there is no CPU fallback)')
        N, Cc = V.shape
        R = W.shape[1]
        assert V.dim() == 2 and W.shape == (Cc, R) and H.shape == (N, R), \
            f'V {tuple(V.shape)}, W {tuple(W.shape)}, H {tuple(H.shape)} do not fit V ~ H @ W.T'
        if R > MAX_RANK:
            raise NotImplementedError(f"solver='hals': rank {R} > {MAX_RANK}, the limit of the sparse kernels")
        for f in (W, H):
            assert f.dtype == torch.float32 and f.is_contiguous() and f.device == V.device, \
                'HalsEngine works on contiguous fp32 masters on the target\'s device'
        self.lib = _capi.load()
        self.W, self.H, self.rank = W, H, R
        self.l1, self.l2 = float(l1), float(l2)
        self.update_W, self.update_H = bool(update_W), bool(update_H)
        self._scaled = False
        self._vw_fresh = False         # dense: num_h holds V W of the current W
        dev = V.device
        if V.is_sparse:
            from .sparse_engine import SparseMU
            self.sp = SparseMU(V, W, H, 2.0, self.l1, self.l2, update_W=update_W, update_H=update_H)
            self.V = None
            self.bad, self.has_zero = self.sp.target_flags()
            self.gram, self.gram2, self.gram_part = self.sp.gram, self.sp.gram2, self.sp.gram_part
        else:
            self.sp = None
            V = V.detach()
            if V.dtype != torch.float32:
                V = V.float()
            self.V = V = V.contiguous()
            v_min = float(V.min()) if V.numel() else 0.0
            self.bad, self.has_zero = not v_min >= 0, v_min == 0          # nmf.py:329-336 (NaN counts as bad)
            part = torch.empty(1024, dtype=torch.float64, device=dev)
            out = torch.zeros(2, dtype=torch.float64, device=dev)
            _capi.check(self.lib.nmfmu_norms(V.data_ptr(), V.numel(), part.data_ptr(), out.data_ptr(), _stream()),
                        'nmfmu_norms')
            self.half_v2 = 0.5 * float(out[1].item())
            self.gram = torch.empty(R * R, dtype=torch.float32, device=dev)
            self.gram2 = torch.empty(R * R, dtype=torch.float32, device=dev)
            self.gram_part = torch.empty(max(self.lib.nmfmu_gram_part_bytes(R), 16), dtype=torch.uint8, device=dev)
            self.num_h = torch.empty(N, R, dtype=torch.float32, device=dev)          # V W
            self.num_w = torch.empty(Cc, R, dtype=torch.float32, device=dev) if update_W else None   # V^T H
            n_ws = max(self.lib.nmfmu_reconstruct_backward_ws(N, Cc, R, 1, 0, None),
                       self.lib.nmfmu_reconstruct_backward_ws(N, Cc, R, 0, 1, None) if update_W else 0)
            self.ws = torch.empty(n_ws, dtype=torch.float32, device=dev) if n_ws > 0 else None

    def target_flags(self):
        return self.bad, self.has_zero

    # -- the two quantities of a half-step
    def _gram(self, f: Tensor, out: Tensor) -> None:
        _capi.check(self.lib.nmfmu_gram(f.data_ptr(), f.shape[0], self.rank, self.gram_part.data_ptr(), out.data_ptr(),
                                        _stream()), 'nmfmu_gram')

    def _numerator(self, which: str):
        """(A, lda): ``V W`` ('h') or ``V^T H`` ('w') from the current factors."""
        if self.sp is not None:
            st, csr = (self.sp.step_h, self.sp.csr_h) if which == 'h' else (self.sp.step_w, self.sp.csr_w)
            self.sp._numerator(st, csr)
            return st.num1, self.sp.r_pad
        N, Cc = self.V.shape
        out = self.num_h if which == 'h' else self.num_w
        _capi.check(self.lib.nmfmu_reconstruct_backward(
            self.V.data_ptr(), Cc, N, Cc, self.H.data_ptr(), self.W.data_ptr(), self.rank,
            out.data_ptr() if which == 'h' else None, out.data_ptr() if which == 'w' else None,
            self.ws.data_ptr() if self.ws is not None else None, _stream()), 'nmfmu_reconstruct_backward')
        if which == 'h':
            self._vw_fresh = True
        return out, self.rank

    def _half_step(self, which: str) -> None:
        self._ensure_scaled()
        own, pan = (self.H, self.W) if which == 'h' else (self.W, self.H)
        A, lda = self._numerator(which)
        self._gram(pan, self.gram)
        _sweep(own, A, lda, self.gram, self.l1, self.l2)
        if which == 'w':
            self._vw_fresh = False

    def w_step(self):
        if self.update_W:
            self._half_step('w')

    def h_step(self):
        if self.update_H:
            self._half_step('h')

    # -- loss and initial scale: both are <V W, H> and <H^T H, W^T W>
    def _dots(self):
        """(<V W, H>, <H^T H, W^T W>) in float64.  One host sync."""
        R = self.rank
        if self.sp is not None:
            self.sp._launch_neg()                       # sum over the stored entries of v s = <V W, H>
            vwh = self.sp.loss_out
        else:
            # (after an H half-step num_h is still V W of the current W: no second product at a checkpoint)
            A = self.num_h if self._vw_fresh else self._numerator('h')[0]
            vwh = (A.double() * self.H.double()).sum()
        self._gram(self.H, self.gram)
        self._gram(self.W, self.gram2)
        gg = self.gram.double() @ self.gram2.double()
        return float(vwh.item()), float(gg.item())

    def _ensure_scaled(self) -> None:
        if self._scaled:
            return
        self._scaled = True
        if self.update_W or self.update_H:
            vwh, gg = self._dots()
            a = vwh / gg if gg != 0 else float('nan')
            if a > 0 and a != float('inf'):
                if self.update_W and self.update_H:
                    self.W.mul_(a ** 0.5)
                    self.H.mul_(a ** 0.5)
                else:
                    (self.W if self.update_W else self.H).mul_(a)
                self._vw_fresh = False
        for f, on in ((self.W, self.update_W), (self.H, self.update_H)):
            if on:
                f.clamp_(min=eps)

    def divergence(self) -> float:
        """1/2 |V - H W^T|^2 from the Gram matrices (the plain divergence, no regularisation terms).  One host sync."""
        self._ensure_scaled()
        if self.sp is not None:
            return self.sp.divergence()
        vwh, gg = self._dots()
        return self.half_v2 - vwh + 0.5 * gg
