"""CCD -- cyclic coordinate descent over the STORED entries of a sparse target with a maintained residual (Yu, Hsieh, Si and
Dhillon, ICDM 2012) -- behind ``NMF.fit(V, beta=2, solver='ccd', unstored='missing')``  (DESIGN.md section 26).

With missing data the quadratic in a row of a factor is built from the panel rows of that row's stored entries only, so
``solver='hals'``'s single Gram matrix does not serve.  A half-step keeps, per owner row, the residuals of the row's entries

    r_e = v_e - <F[i], P[j_e]>
    for k = 0 .. R-1:   d = sum_e P[j_e, k]^2      n = sum_e r_e P[j_e, k]
                        f' = max(eps, (n + F[i, k] d - l1) / (d + l2 + eps))
                        r_e -= (f' - F[i, k]) P[j_e, k];   F[i, k] = f'

at O(nnz R) per half-step, the order of one masked multiplicative update.  The sweep is one HIP kernel
(``nmfmu_sp_ccd_sweep``: a wave per row, a workgroup per long row, the lanes across the row's entries); ``ccd_sweep`` is
its public face, ``CcdEngine`` the engine ``fit`` drives.  fp32 throughout; there is no CPU path.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _capi
from . import sparse_autograd as SA
from .constants import eps

__all__ = ['ccd_sweep', 'CcdEngine', 'RESIDENT_LIMIT', 'WG_WAVES']

MAX_RANK = SA.MAX_RANK
RESIDENT_LIMIT = 512     # nmfmu_sp_ccd_limit(): 8 entries per lane x 64 lanes keep their residuals in registers; also the
                         # default count above which a row takes a workgroup of WG_WAVES waves instead of one wave
WG_WAVES = 16            # nmfmu_sp_ccd_wg_waves()
LAYOUTS = ('direct', 'transposed', 'lds')


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def lds_rows(rank: int) -> int:
    """Entries per row up to which the row's panel rows are staged in LDS at this rank (``nmfmu_sp_ccd_lds_rows``)."""
    return int(_capi.load().nmfmu_sp_ccd_lds_rows(int(rank)))


class _Side:
    """One side's work list and the sweep's buffers: the CSR / CSC arrays, the order list (longest rows first: a stable
    device sort of the counts), the residual scratch of ``nnz`` floats and, for two of the layouts, the transposed panel
    copy.  ``layout``: where a row fetches ``P[j_e, k]`` from -- 'direct' (the row-major panel: the default, the fastest of
    the three on both sides of the benchmark target, profiles/ccd.json), 'transposed' (a ``[R, n_panel]`` copy made per
    call) or 'lds' (one-wave rows that fit stage their panel rows in LDS, the rest gather from the transposed copy).  No
    result depends on it."""

    def __init__(self, T: SA.SparseTarget, side: str, rank: int, layout: str = 'direct'):
        assert layout in LAYOUTS, f'layout must be one of {LAYOUTS}, got {layout!r}'
        (self.ptr, self.idx, self.vals), _, _, _ = T.side(side)
        dev = T.device
        self.n_rows = self.ptr.numel() - 1
        self.n_panel = T.shape[1] if side == 'h' else T.shape[0]
        self.nnz, self.rank, self.layout = T.nnz, rank, layout
        self.order = torch.argsort(torch.diff(self.ptr), descending=True, stable=True).to(torch.int32)
        self.lds_rows = lds_rows(rank) if layout == 'lds' else 0
        self.scratch = torch.empty(max(self.nnz, 4), dtype=torch.float32, device=dev)
        self.pt = torch.empty(rank * self.n_panel, dtype=torch.float32, device=dev) if layout != 'direct' else None
        self.spare = T.spare

    def sweep(self, F: Tensor, panel: Tensor, l1: float, l2: float, limit: int = 0, order=None, wg_rows: int = 0) -> None:
        order = self.order if order is None else order
        _capi.check(_capi.load().nmfmu_sp_ccd_sweep(
            self.ptr.data_ptr(), SA.entries(self.idx, self.spare), SA.entries(self.vals, self.spare), order.data_ptr(),
            self.n_rows, F.data_ptr(), panel.data_ptr(), self.n_panel, self.rank, l1, l2, self.scratch.data_ptr(),
            self.pt.data_ptr() if self.pt is not None else None, int(limit), self.lds_rows, int(wg_rows),
            _stream()), 'nmfmu_sp_ccd_sweep')


@torch.no_grad()
def ccd_sweep(F: Tensor, panel: Tensor, T, side: str, l1: float = 0.0, l2: float = 0.0, *, _limit: int = 0,
              _layout: str = 'direct', _order: Tensor = None, _wg_rows: int = 0) -> Tensor:
    """One coordinate-descent pass over the rank on ``F [rows, R]``, in place (contiguous fp32, on the ROCm device), over the
    stored entries of ``T`` alone: every owner row with entries runs the recurrence of the module docstring against the rows
    of ``panel [n, R]`` its entries name; a row without entries is not touched.

    ``T``: a ``SparseTarget`` or a 2-D sparse-COO tensor ``(N, C)``.  ``side``: 'h' -- ``F`` is ``H (N, R)``, ``panel`` is
    ``W (C, R)``; 'w' -- ``F`` is ``W``, ``panel`` is ``H``.  ``panel`` is not written.  Returns ``F``.  Raises ``NmfmuError``
    for CPU tensors, ``NotImplementedError`` above rank 256.

    ``_limit`` / ``_layout`` / ``_order`` / ``_wg_rows`` are for the tests and the benchmark: the count per wave up to which a
    row keeps its residuals in registers (0 = ``RESIDENT_LIMIT``, also the largest value), where ``P[j_e, k]`` is fetched
    from (``LAYOUTS``), the hand-out order of the rows (an int32 permutation) and the count above which a row takes a
    workgroup (0 = ``RESIDENT_LIMIT``).  A row's bits depend on none of the first three; ``_wg_rows`` moves rows between two
    summation orders."""
    what = 'ccd_sweep'
    if side not in ('h', 'w'):
        raise ValueError(f"{what}: side must be 'h' or 'w', got {side!r}")
    if not isinstance(T, SA.SparseTarget) and not (isinstance(T, Tensor) and T.is_sparse and T.dim() == 2):
        raise ValueError(f'{what}: T must be a SparseTarget or a 2-D sparse-COO tensor')
    for t, name in ((F, 'F'), (panel, 'panel'), (T, 'T')):
        if t.device.type != 'cuda':
            raise _capi.NmfmuError(f'{what}: {name} lives on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'the tensors with .cuda() (there is no CPU fallback)')
    for t, name in ((F, 'F'), (panel, 'panel')):
        if t.dtype != torch.float32:
            raise TypeError(f'{what}: {name} must be float32, got {t.dtype}')
        if t.device != F.device:
            raise ValueError(f'{what}: {name} lives on {t.device}, F on {F.device}')
    if F.dim() != 2 or not F.is_contiguous():
        raise ValueError(f'{what}: F must be a contiguous 2-D tensor (it is updated in place)')
    rows, R = F.shape
    N, Cc = int(T.shape[0]), int(T.shape[1])
    want = ((N, R), (Cc, R)) if side == 'h' else ((Cc, R), (N, R))
    if (rows, R) != want[0] or panel.dim() != 2 or tuple(panel.shape) != want[1]:
        raise ValueError(f'{what}: side {side!r} of a {N} x {Cc} target needs F {want[0]} and panel {want[1]}, got '
                         f'{tuple(F.shape)} and {tuple(panel.shape)}')
    if not 0 <= int(_limit) <= RESIDENT_LIMIT:
        raise ValueError(f'{what}: _limit must lie in 0 .. {RESIDENT_LIMIT}, got {_limit!r}')
    if int(_wg_rows) < 0:
        raise ValueError(f'{what}: _wg_rows must be >= 0, got {_wg_rows!r}')
    if R > MAX_RANK:
        raise NotImplementedError(f'{what}: rank {R} > {MAX_RANK}, the limit of the sparse kernels')
    if rows == 0 or R == 0:
        return F
    if not isinstance(T, SA.SparseTarget):
        T = SA.SparseTarget(T)
    if T.nnz == 0:
        return F
    s = _Side(T, side, R, _layout)
    s.sweep(F.detach(), panel.detach().contiguous(), float(l1), float(l2), int(_limit),
            None if _order is None else _order.to(torch.int32).contiguous(), int(_wg_rows))
    return F


class CcdEngine:
    """The interface ``fit`` drives (``target_flags`` / ``w_step`` / ``h_step`` / ``divergence``) with CCD half-steps on a
    missing-data target, beta = 2.

    ``V``: a sparse-COO tensor or a ready-made ``SparseTarget``; its stored entries are the observed ones.  ``W (C, R)`` /
    ``H (N, R)``: the contiguous fp32 masters, updated in place.  A half-step is one ``nmfmu_sp_ccd_sweep`` call; the loss is
    the masked beta = 2 loss of ``MaskedMU``.  Before the first half-step or loss the factors are scaled once by the scalar
    that minimises the loss over the stored entries, ``a = sum_e v_e s_e / sum_e s_e^2`` with ``s = scoring.score_pairs``
    (float64 dots; both trainable: each times sqrt(a), one: that one times a; skipped unless a is finite and positive) and
    the trainable ones clamped to >= eps."""
    precision_name = 'fp32'

    def __init__(self, V, W: Tensor, H: Tensor, l1: float = 0.0, l2: float = 0.0, update_W: bool = True,
                 update_H: bool = True):
        for t in (V, W, H):
            if t.device.type != 'cuda':
                raise _capi.NmfmuError(f'CcdEngine: tensors live on {t.device}; torchnmf_amd computes on an MI355X only '
                                       f'(there is no CPU fallback)')
        if not isinstance(V, SA.SparseTarget) and not (isinstance(V, Tensor) and V.is_sparse):
            raise ValueError("CcdEngine: the target must be sparse-COO (or a SparseTarget) whose stored entries are the observed "
                             "ones; for a dense V with a boolean mask pass V.sparse_mask(mask)")
        T = V if isinstance(V, SA.SparseTarget) else SA.SparseTarget(V)
        N, Cc = T.shape
        R = W.shape[1]
        assert W.shape == (Cc, R) and H.shape == (N, R), \
            f'V {tuple(T.shape)}, W {tuple(W.shape)}, H {tuple(H.shape)} do not fit V ~ H @ W.T'
        if R > MAX_RANK:
            raise NotImplementedError(f"solver='ccd': rank {R} > {MAX_RANK}, the limit of the sparse kernels")
        for f in (W, H):
            assert f.dtype == torch.float32 and f.is_contiguous() and f.device == T.device, \
                'CcdEngine works on contiguous fp32 masters on the target\'s device'
        self.T, self.W, self.H, self.rank = T, W, H, R
        self.l1, self.l2 = float(l1), float(l2)
        self.update_W, self.update_H = bool(update_W), bool(update_H)
        self.bad = bool((~(T.vals >= 0)).any().item()) if T.nnz else False      # nmf.py:329-330
        self.has_zero = T.has_zero                                             # stored zeros only: unstored is unknown
        self.side_w = _Side(T, 'w', R) if self.update_W and T.nnz else None
        self.side_h = _Side(T, 'h', R) if self.update_H and T.nnz else None
        self.loss_part = torch.empty((T.seg_h.shape[0] + 3) // 4, dtype=torch.float64, device=T.device)
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=T.device)
        self._scaled = False

    def target_flags(self):
        return self.bad, self.has_zero

    def _ensure_scaled(self) -> None:
        if self._scaled:
            return
        self._scaled = True
        if (self.update_W or self.update_H) and self.T.nnz:
            from .scoring import score_pairs
            rowptr, colidx, vals = self.T.csr
            rows = torch.repeat_interleave(torch.arange(self.T.shape[0], device=self.T.device), torch.diff(rowptr).long())
            s = score_pairs(self.H, self.W, rows, colidx).double()
            vs, ss = float((vals.double() @ s).item()), float((s @ s).item())
            a = vs / ss if ss != 0 else float('nan')
            if a > 0 and a != float('inf'):
                if self.update_W and self.update_H:
                    self.W.mul_(a ** 0.5)
                    self.H.mul_(a ** 0.5)
                else:
                    (self.W if self.update_W else self.H).mul_(a)
        for f, on in ((self.W, self.update_W), (self.H, self.update_H)):
            if on:
                f.clamp_(min=eps)

    def w_step(self):
        if self.update_W:
            self._ensure_scaled()
            if self.side_w is not None:
                self.side_w.sweep(self.W, self.H, self.l1, self.l2)

    def h_step(self):
        if self.update_H:
            self._ensure_scaled()
            if self.side_h is not None:
                self.side_h.sweep(self.H, self.W, self.l1, self.l2)

    def divergence(self) -> float:
        """1/2 sum over the stored entries of (v - <H[i], W[j]>)^2 (no regularisation terms).  One host sync."""
        self._ensure_scaled()
        return float(SA._masked_loss(self.H, self.W, self.T, 2.0, self.loss_part, self.loss_out).item())
