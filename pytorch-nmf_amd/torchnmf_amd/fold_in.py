"""Folding new rows into a fitted model: ``H_new`` for rows that were not in the training target,
with ``W`` fixed -- sklearn's ``NMF.transform``.

``fold_in(W, target, beta, max_iter, tol, alpha, l1_ratio, *, unstored, H0, generator, return_n_iter)`` iterates the H
half-step of ``fit`` on every new row alone (nmf.py:61-92) and stops each row by itself once
``max_r |h_k - h_(k-1)| <= tol * max_r h_k``.  ONE kernel launch (``nmfmu_fold_in``) runs all rows and all iterations: a
row's ``W`` rows are fetched once into LDS when they fit and the row never leaves its wave.  Besides it a call launches only
its set-up: the column sums of ``W`` or its Gram matrix (``unstored='zero'``) and a sort of the rows by count.

``unstored='missing'`` (any beta): numerator and denominator over the stored entries, the rule of
``fit(..., unstored='missing')``.  ``unstored='zero'``: beta 1 (denominator = the column sums of ``W``) and beta 2
(denominator = ``h @ (W^T W)``); for any other beta > 0 the positive term is a dense pass and ``NotImplementedError`` names
the route through ``fit``.

The result is detached and in the dtype of ``W``; the arithmetic is fp32.  The argument checks run before any device work
beyond what a check itself needs, in the order of ``fold_in``'s body.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _capi
from .engine import mu_gamma
from .sparse_autograd import MAX_RANK, SparseTarget

MODES = {'missing': 0, 'zero': 1}         # include/nmfmu.h: NMFMU_FOLD_MISSING / NMFMU_FOLD_ZERO

_FIT_ROUTE = "NMF(W=W, H=H0, trainable_W=False).cuda().fit(V_new, beta, unstored=...)"
_BETA_TEXT = ("When beta <= 0 and V contains zeros, the training process may diverge. "
              "Please add small values to V, or use a positive beta value.")


def default_block(rank: int) -> int:
    """Stored entries per LDS block at this rank (``nmfmu_fold_in_block``): what one wave keeps resident, and the default
    count above which a row takes a whole workgroup."""
    return int(_capi.load().nmfmu_fold_in_block(int(rank)))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _csr(target, n_rows: int):
    """(rowptr int32 [n + 1], colidx int32 [nnz], vals fp32 [nnz]) -- the CSR side alone."""
    if isinstance(target, SparseTarget):
        return target.csr
    V = target.detach().coalesce()
    idx, vals = V.indices(), V.values().float().contiguous()
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=V.device)
    rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=n_rows), 0)
    return rowptr.to(torch.int32).contiguous(), idx[1].to(torch.int32).contiguous(), vals


def fold_in(W: Tensor, target, beta: float = 1, max_iter: int = 200, tol: float = 1e-4, alpha: float = 0,
            l1_ratio: float = 0, *, unstored: str = 'zero', H0: Tensor = None, generator=None, return_n_iter: bool = False,
            _block: int = 0, _long_rows: int = 0, _fill=None):
    """``H_new [n_new, R]`` (detached, dtype of ``W``) for the rows of ``target`` -- a 2-D sparse-COO tensor ``(n_new, C)`` or
    a ``metrics.SparseTarget`` -- against the fixed ``W (C, R)``; with ``return_n_iter`` also the int32 iteration count of
    every row.

    ``beta``, ``alpha``, ``l1_ratio``: as in ``fit`` (l1 = alpha * l1_ratio, l2 = alpha * (1 - l1_ratio)).  ``unstored``:
    'zero' (beta in {1, 2}) or 'missing' (any beta; beta <= 0 needs strictly positive stored values).  ``H0``: the
    non-negative start ``[n_new, R]``; default ``|N(0, 1)|`` drawn on the device (``generator``).  A row stops after the
    first iteration ``k`` with ``max_r |h_k - h_(k-1)| <= tol * max_r h_k``; ``tol = 0`` runs ``max_iter`` iterations.  A
    row's result does not depend on the other rows of the call; a repeated call is bitwise identical.

    ``_block`` / ``_long_rows`` / ``_fill`` are for the tests: the kernel's two thresholds (0 = default) and a value the
    count array is pre-filled with."""
    what = 'fold_in'
    if unstored not in MODES:
        raise ValueError(f"unstored must be 'zero' or 'missing', got {unstored!r}")
    if not isinstance(target, SparseTarget) and not (isinstance(target, Tensor) and target.is_sparse):
        raise ValueError(f"{what}: the new rows must be a 2-D sparse-COO tensor or a SparseTarget whose stored entries are "
                         f"the observed ones; for a dense V with a boolean mask pass V.sparse_mask(mask) (mask: a sparse-COO "
                         f"tensor), for truly dense rows use {_FIT_ROUTE}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError(f'{what}: max_iter must be an int >= 0, got {max_iter!r}')
    if not float(tol) >= 0:
        raise ValueError(f'{what}: tol must be >= 0, got {tol!r}')
    if not (isinstance(W, Tensor) and W.dim() == 2 and len(target.shape) == 2 and min(W.shape) > 0):
        raise ValueError(f'{what}: W must be (C, R) and the target (n_new, C)')
    n_new, Cc = int(target.shape[0]), int(target.shape[1])
    R = W.shape[1]
    if Cc != W.shape[0]:
        raise ValueError(f'{what}: the target has {Cc} columns, W has {W.shape[0]} rows')
    if H0 is not None and not (isinstance(H0, Tensor) and tuple(H0.shape) == (n_new, R)):
        raise ValueError(f'{what}: H0 must be ({n_new}, {R}), got {tuple(H0.shape) if isinstance(H0, Tensor) else H0!r}')
    if R > MAX_RANK:
        raise NotImplementedError(f'{what}: rank {R} > {MAX_RANK}, the limit of the sparse kernels')
    for t in (W, target, H0):
        if t is not None and t.device.type != 'cuda':
            raise _capi.NmfmuError(f'{what}: tensors live on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'them with .cuda() (there is no CPU fallback)')
    if not W.dtype.is_floating_point:
        raise NotImplementedError(f'{what}: W must be floating point, got {W.dtype}')
    beta = float(beta)
    rowptr, colidx, vals = _csr(target, n_new)
    nnz = int(vals.numel())
    if nnz:
        lo = float(vals.min())
        assert lo >= 0, "Target should be non-negative."          # (NaN fails too, like torch.all(V >= 0))
    else:
        lo = 1.0
    if beta <= 0 and (unstored == 'zero' or lo == 0):
        raise ValueError(_BETA_TEXT)
    if unstored == 'zero' and beta not in (1.0, 2.0):
        raise NotImplementedError(f"{what}: unstored='zero' supports beta in {{1, 2}}, got {beta:g}: for any other beta the "
                                  f"positive term sum (h W^T + eps)^beta runs over every column, a dense pass; use "
                                  f"{_FIT_ROUTE}")
    dev = W.device
    if H0 is not None:
        assert bool(torch.all(H0 >= 0.)), "Tensor H should be non-negative."
        H = H0.detach().float().contiguous().clone()
    else:
        H = torch.randn(n_new, R, device=dev, generator=generator).abs_()
    n_iter = torch.zeros(n_new, dtype=torch.int32, device=dev)
    if _fill is not None:
        n_iter.fill_(_fill)

    if n_new and max_iter:
        lib = _capi.load()
        Wc = W.detach().float().contiguous()
        aux = None
        if unstored == 'zero' and beta == 1.0:      # nmf.py:128-131: W.sum(0)
            aux = torch.empty(R, dtype=torch.float32, device=dev)
            part = torch.empty(R * 128, dtype=torch.float32, device=dev)
            _capi.check(lib.nmfmu_rank_sums(Wc.data_ptr(), Cc, R, 1, part.data_ptr(), aux.data_ptr(), _stream()),
                        'nmfmu_rank_sums')
        elif unstored == 'zero':                    # nmf.py:616-617: W^T W
            aux = torch.empty(R * R, dtype=torch.float32, device=dev)
            part = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device=dev)
            _capi.check(lib.nmfmu_gram(Wc.data_ptr(), Cc, R, part.data_ptr(), aux.data_ptr(), _stream()), 'nmfmu_gram')
        # longest rows first (a stable device sort of the counts): the hand-out order, no result depends on it
        order = torch.argsort(torch.diff(rowptr), descending=True, stable=True).to(torch.int32)
        spare = colidx if nnz else torch.zeros(4, dtype=torch.int32, device=dev)   # an empty tensor's pointer is null
        l1, l2 = float(alpha * l1_ratio), float(alpha * (1 - l1_ratio))            # nmf.py:348-349
        _capi.check(lib.nmfmu_fold_in(rowptr.data_ptr(), spare.data_ptr(), vals.data_ptr() if nnz else spare.data_ptr(),
                                      n_new, H.data_ptr(), Wc.data_ptr(), Cc, R, beta, MODES[unstored],
                                      aux.data_ptr() if aux is not None else None, l1, l2, mu_gamma(beta), max_iter,
                                      float(tol), n_iter.data_ptr(), order.data_ptr(), int(_block), int(_long_rows),
                                      _stream()), 'nmfmu_fold_in')
    else:
        n_iter.zero_()
    out = H if W.dtype == torch.float32 else H.to(W.dtype)
    return (out, n_iter) if return_n_iter else out
