"""Weighted CCD -- implicit-feedback factorisation (Hu, Koren and Volinsky, ICDM 2008; element-wise ALS with a uniform missing
weight, He et al., SIGIR 2016) -- behind ``NMF.fit(V, beta=2, solver='ccd', unstored=omega)``  (DESIGN.md section 27).

Stored entries carry weight 1 (stored zeros too: explicit negatives); every unstored entry is a zero observed with a
confidence ``0 < omega < 1``.  The loss splits into a part over the stored entries and a Gram part,

    1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2  =  1/2 sum_stored [(v - y)^2 - omega y^2] + 1/2 omega <H^T H, W^T W>

so an iteration costs O(nnz R + (N + C) R^2) and nothing of size N x C is formed.  With ``c = 1 - omega`` and
``G = panel^T panel`` a half-step keeps, per owner row, the residuals of the row's stored entries

    t_e = v_e - c <F[i], P[j_e]>
    for k = 0 .. R-1:   d = sum_e P[j_e, k]^2      n = sum_e t_e P[j_e, k]      q = sum_j F[i, j] G[k, j]
                        D = c d + omega G[k, k]
                        f' = max(eps, (n - omega q + F[i, k] D - l1) / (D + l2 + eps))
                        t_e -= c (f' - F[i, k]) P[j_e, k];   F[i, k] = f'

-- omega = 0 is ``ccd.ccd_sweep``, omega = 1 the HALS sweep on the densified target; a row without entries is swept too (its
minimiser is the floor).  The sweep is one HIP entry (``nmfmu_sp_wccd_sweep``: a wave per row, a workgroup per long row, the
lanes across the row's entries, the owner row in registers); ``wccd_sweep`` is its public face, ``WeightedCcdEngine`` the
engine ``fit`` drives.  fp32 throughout; there is no CPU path.
"""
from __future__ import annotations

import numbers

import torch
from torch import Tensor

from . import _capi
from . import sparse_autograd as SA
from .ccd import RESIDENT_LIMIT, _Side, _stream
from .constants import eps

__all__ = ['wccd_sweep', 'WeightedCcdEngine']

MAX_RANK = SA.MAX_RANK


def _weight(omega, what: str) -> float:
    if isinstance(omega, bool) or not isinstance(omega, numbers.Real) or not 0.0 < float(omega) < 1.0:
        raise ValueError(f'{what}: omega must be a real number strictly between 0 and 1, got {omega!r}')
    w32 = torch.tensor(float(omega), dtype=torch.float32).item()       # what the C entry receives
    if not 0.0 < w32 < 1.0:
        raise ValueError(f'{what}: omega = {omega!r} is not strictly between 0 and 1 in fp32')
    return float(omega)


class _WSide(_Side):
    """``ccd._Side`` (the CSR / CSC arrays, the order list, the residual scratch; the row-major panel gather) with the Gram
    matrix of the panel and ``nmfmu_gram``'s scratch."""

    def __init__(self, T: SA.SparseTarget, side: str, rank: int):
        super().__init__(T, side, rank, 'direct')
        self.lib = _capi.load()
        self.gram = torch.empty(rank, rank, dtype=torch.float32, device=T.device)
        self.gram_part = torch.empty(max(self.lib.nmfmu_gram_part_bytes(rank), 16), dtype=torch.uint8, device=T.device)

    def make_gram(self, panel: Tensor) -> Tensor:
        _capi.check(self.lib.nmfmu_gram(panel.data_ptr(), panel.shape[0], self.rank, self.gram_part.data_ptr(),
                                        self.gram.data_ptr(), _stream()), 'nmfmu_gram')
        return self.gram

    def wsweep(self, F: Tensor, panel: Tensor, G: Tensor, omega: float, l1: float, l2: float, limit: int = 0, order=None,
               wg_rows: int = 0) -> None:
        order = self.order if order is None else order
        _capi.check(self.lib.nmfmu_sp_wccd_sweep(
            self.ptr.data_ptr(), SA.entries(self.idx, self.spare), SA.entries(self.vals, self.spare), order.data_ptr(),
            self.n_rows, F.data_ptr(), panel.data_ptr(), self.n_panel, self.rank, G.data_ptr(), omega, l1, l2,
            self.scratch.data_ptr(), int(limit), int(wg_rows), _stream()), 'nmfmu_sp_wccd_sweep')


@torch.no_grad()
def wccd_sweep(F: Tensor, panel: Tensor, T, side: str, omega: float, l1: float = 0.0, l2: float = 0.0, *, G: Tensor = None,
               _limit: int = 0, _order: Tensor = None, _wg_rows: int = 0) -> Tensor:
    """One coordinate-descent pass over the rank on ``F [rows, R]``, in place (contiguous fp32, on the ROCm device), for the
    weighted objective of the module docstring: every owner row -- one without stored entries too -- runs the recurrence
    against the rows of ``panel [n, R]`` its entries name and the Gram matrix of the panel.

    ``T``: a ``SparseTarget`` or a 2-D sparse-COO tensor ``(N, C)``.  ``side``: 'h' -- ``F`` is ``H (N, R)``, ``panel`` is
    ``W (C, R)``; 'w' -- ``F`` is ``W``, ``panel`` is ``H``.  ``omega``: the weight of an unstored zero, a real number strictly
    between 0 and 1.  ``G``: ``panel^T panel`` as a contiguous fp32 ``[R, R]`` device tensor, symmetric (coordinate k reads its
    row k); ``None``: computed here with ``nmfmu_gram``.  A given ``G`` is used as it is.  ``panel`` and ``G`` are not written.
    Returns ``F``.  Raises ``NmfmuError`` for CPU tensors, ``NotImplementedError`` above rank 256.

    ``_limit`` / ``_order`` / ``_wg_rows`` are for the tests and the benchmark, as in ``ccd.ccd_sweep``: the count per wave up
    to which a row keeps its residuals in registers (0 = ``ccd.RESIDENT_LIMIT``, also the largest value), the hand-out order of
    the rows (an int32 permutation) and the count above which a row takes a workgroup (0 = ``ccd.RESIDENT_LIMIT``).  A row's
    bits depend on neither of the first two; ``_wg_rows`` moves rows between two summation orders."""
    what = 'wccd_sweep'
    if side not in ('h', 'w'):
        raise ValueError(f"{what}: side must be 'h' or 'w', got {side!r}")
    if not isinstance(T, SA.SparseTarget) and not (isinstance(T, Tensor) and T.is_sparse and T.dim() == 2):
        raise ValueError(f'{what}: T must be a SparseTarget or a 2-D sparse-COO tensor')
    omega = _weight(omega, what)
    given = [(F, 'F'), (panel, 'panel')] + ([(G, 'G')] if G is not None else [])
    for t, name in given + [(T, 'T')]:
        if t.device.type != 'cuda':
            raise _capi.NmfmuError(f'{what}: {name} lives on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'the tensors with .cuda() (there is no CPU fallback)')
    for t, name in given:
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
    if G is not None and (tuple(G.shape) != (R, R) or not G.is_contiguous()):
        raise ValueError(f'{what}: G must be a contiguous [{R}, {R}] matrix, got {tuple(G.shape)}')
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
    s = _WSide(T, side, R)                   # (a target without a stored entry is swept too: the Gram term acts on every row)
    P = panel.detach().contiguous()
    Gd = s.make_gram(P) if G is None else G.detach()
    s.wsweep(F.detach(), P, Gd, omega, float(l1), float(l2), int(_limit),
             None if _order is None else _order.to(torch.int32).contiguous(), int(_wg_rows))
    return F


class WeightedCcdEngine:
    """The interface ``fit`` drives (``target_flags`` / ``w_step`` / ``h_step`` / ``divergence``) with weighted CCD half-steps,
    beta = 2: the stored entries of ``V`` carry weight 1, its unstored entries are zeros of weight ``omega``.

    ``V``: a sparse-COO tensor or a ready-made ``SparseTarget``.  ``W (C, R)`` / ``H (N, R)``: the contiguous fp32 masters,
    updated in place.  A half-step is one ``nmfmu_gram`` on the panel plus one ``nmfmu_sp_wccd_sweep`` call.  The loss is the
    weighted loss of the module docstring by its identity: the scores of the stored entries from ``scoring.score_pairs``,
    summed in float64, and ``<H^T H, W^T W>`` from float64 Gram matrices (a large term that mostly cancels against the
    stored part).  Before the first half-step or loss the factors are scaled once by the scalar that minimises the loss,
    ``a = sum_e v_e s_e / (c sum_e s_e^2 + omega <H^T H, W^T W>)`` (both trainable: each times sqrt(a), one: that one times a;
    skipped unless a is finite and positive) and the trainable ones clamped to >= eps -- ``ccd.CcdEngine``'s rules."""
    precision_name = 'fp32'

    def __init__(self, V, W: Tensor, H: Tensor, omega: float, l1: float = 0.0, l2: float = 0.0, update_W: bool = True,
                 update_H: bool = True):
        for t in (V, W, H):
            if t.device.type != 'cuda':
                raise _capi.NmfmuError(f'WeightedCcdEngine: tensors live on {t.device}; torchnmf_amd computes on an MI355X '
                                       f'only (there is no CPU fallback)')
        if not isinstance(V, SA.SparseTarget) and not (isinstance(V, Tensor) and V.is_sparse):
            raise ValueError('WeightedCcdEngine: the target must be sparse-COO (or a SparseTarget): the weight is that of its '
                             'unstored entries')
        self.omega = _weight(omega, 'WeightedCcdEngine')
        T = V if isinstance(V, SA.SparseTarget) else SA.SparseTarget(V)
        N, Cc = T.shape
        R = W.shape[1]
        assert W.shape == (Cc, R) and H.shape == (N, R), \
            f'V {tuple(T.shape)}, W {tuple(W.shape)}, H {tuple(H.shape)} do not fit V ~ H @ W.T'
        if R > MAX_RANK:
            raise NotImplementedError(f"solver='ccd': rank {R} > {MAX_RANK}, the limit of the sparse kernels")
        for f in (W, H):
            assert f.dtype == torch.float32 and f.is_contiguous() and f.device == T.device, \
                'WeightedCcdEngine works on contiguous fp32 masters on the target\'s device'
        self.T, self.W, self.H, self.rank = T, W, H, R
        self.l1, self.l2 = float(l1), float(l2)
        self.update_W, self.update_H = bool(update_W), bool(update_H)
        self.bad = bool((~(T.vals >= 0)).any().item()) if T.nnz else False      # nmf.py:329-330
        self.has_zero = T.has_zero or T.nnz < N * Cc                           # an unstored entry is an observed zero
        self.side_w = _WSide(T, 'w', R) if self.update_W else None
        self.side_h = _WSide(T, 'h', R) if self.update_H else None
        rowptr, colidx, _ = T.csr
        self.rows = torch.repeat_interleave(torch.arange(N, device=T.device), torch.diff(rowptr).long())
        self.cols = colidx
        self._scaled = False

    def target_flags(self):
        return self.bad, self.has_zero

    def _sums(self):
        """(sum_e v_e s_e, sum_e s_e^2, sum_e (v_e - s_e)^2, <H^T H, W^T W>) in float64.  One host sync."""
        if self.T.nnz:
            from .scoring import score_pairs
            s = score_pairs(self.H, self.W, self.rows, self.cols).double()
            v = self.T.csr[2].double()
            r = v - s
            part = torch.stack((v @ s, s @ s, r @ r))
        else:
            part = torch.zeros(3, dtype=torch.float64, device=self.T.device)
        Hd, Wd = self.H.double(), self.W.double()
        gg = ((Hd.t() @ Hd) * (Wd.t() @ Wd)).sum()
        return tuple(float(x) for x in torch.cat((part, gg.reshape(1))).tolist())

    def _ensure_scaled(self) -> None:
        if self._scaled:
            return
        self._scaled = True
        if self.update_W or self.update_H:
            vs, ss, _, gg = self._sums()
            den = (1.0 - self.omega) * ss + self.omega * gg
            a = vs / den if den != 0 else float('nan')
            if a > 0 and a != float('inf'):
                if self.update_W and self.update_H:
                    self.W.mul_(a ** 0.5)
                    self.H.mul_(a ** 0.5)
                else:
                    (self.W if self.update_W else self.H).mul_(a)
        for f, on in ((self.W, self.update_W), (self.H, self.update_H)):
            if on:
                f.clamp_(min=eps)

    def _half_step(self, side: _WSide, own: Tensor, pan: Tensor) -> None:
        self._ensure_scaled()
        side.wsweep(own, pan, side.make_gram(pan), self.omega, self.l1, self.l2)

    def w_step(self):
        if self.update_W:
            self._half_step(self.side_w, self.W, self.H)

    def h_step(self):
        if self.update_H:
            self._half_step(self.side_h, self.H, self.W)

    def divergence(self) -> float:
        """1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 (no regularisation terms) as
        1/2 sum_stored [(v - y)^2 - omega y^2] + 1/2 omega <H^T H, W^T W>.  One host sync."""
        self._ensure_scaled()
        _, ss, rr, gg = self._sums()
        return 0.5 * (rr - self.omega * ss) + 0.5 * self.omega * gg
