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

``fold_in_cd(W, target, 2, ..., unstored=..., solver='ccd' | 'hals')`` (beta 2; ``fold_in``'s own
signature is unchanged) folds the rows in by cyclic coordinate descent instead: one
launch of ``nmfmu_fold_in_cd`` runs every iteration of every row for the objective

    1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2 + l1 sum h + l2/2 |h|^2

with ``solver='ccd', unstored='missing'`` (omega = 0: ``ccd.ccd_sweep``'s recurrence on the row), ``solver='ccd',
unstored=omega`` (0 < omega < 1: implicit feedback, ``wccd.wccd_sweep``'s recurrence -- the objective of
``fit(solver='ccd', unstored=omega)``) and ``solver='hals', unstored='zero'`` (omega = 1).  A row's ``W`` rows, the constant
``d_k = sum_e W[j_e, k]^2`` and, for omega = 1, the whole numerator's data term are formed once per row; each iteration is an
exact minimiser per coordinate, so ``H0`` is used AS IT IS -- there is no initial scaling (``fit`` scales its factors once;
a coordinate step does not need it).  A row without stored entries is returned as it came under 'missing' and swept (to the
floor ``eps``) for omega > 0.

The result is detached and in the dtype of ``W``; the arithmetic is fp32.  The argument checks run before any device work
beyond what a check itself needs, in the order of ``_fold``'s body: the solver's name; for 'ccd' / 'hals' beta and the
reading of the unstored entries (``fit``'s refusals, in ``fit``'s words), then the range of a weight; for 'mu' the two
strings; then, for every solver, the target's type, ``max_iter``, ``tol``, the shapes, ``H0``, the rank, the devices, the
dtype of ``W``, and last the checks that read the data (non-negative target, non-negative ``H0``).
"""
from __future__ import annotations

import numbers

import torch
from torch import Tensor

from . import _capi
from .engine import mu_gamma
from .sparse_autograd import MAX_RANK, SparseTarget

MODES = {'missing': 0, 'zero': 1}         # include/nmfmu.h: NMFMU_FOLD_MISSING / NMFMU_FOLD_ZERO

_FIT_ROUTE = "NMF(W=W, H=H0, trainable_W=False).cuda().fit(V_new, beta, unstored=...)"
SOLVERS = ('mu', 'hals', 'ccd')
_BETA_TEXT = ("When beta <= 0 and V contains zeros, the training process may diverge. "
              "Please add small values to V, or use a positive beta value.")


def default_block(rank: int) -> int:
    """Stored entries per LDS block at this rank (``nmfmu_fold_in_block``): what one wave keeps resident, and the default
    count above which a row takes a whole workgroup."""
    return int(_capi.load().nmfmu_fold_in_block(int(rank)))


def default_block_cd(rank: int) -> int:
    """The largest share of a wave whose ``W`` rows ``nmfmu_fold_in_cd`` stages in LDS at this rank (``_block``'s default and
    largest value)."""
    return int(_capi.load().nmfmu_fold_in_cd_block(int(rank)))


def default_long_rows_cd(rank: int) -> int:
    """The count above which ``nmfmu_fold_in_cd`` gives a row the whole workgroup by default (``_long_rows``)."""
    return int(_capi.load().nmfmu_fold_in_cd_long_rows(int(rank)))


def _cd_omega(solver: str, beta, unstored) -> float:
    """omega of the coordinate-descent route, or ``fit``'s refusal of the combination (nmf.py, ``fit``: same classes, same
    words).  No device work."""
    weight = float(unstored) if isinstance(unstored, numbers.Real) and not isinstance(unstored, bool) else None
    if float(beta) != 2.0:
        raise NotImplementedError(f"solver={solver!r}: the coordinate minimiser is closed-form only for beta = 2, got "
                                  f"beta = {beta:g}")
    if solver == 'ccd' and weight is None and unstored != 'missing':
        raise NotImplementedError("solver='ccd' fits the stored entries only and needs unstored='missing'; for a "
                                  "target whose unstored entries are observed zeros use solver='hals'")
    if solver == 'hals' and unstored == 'missing':
        raise NotImplementedError("solver='hals': the Gram shortcut needs unstored = 'zero' (with unstored='missing' "
                                  "the denominator runs over the stored entries only: use solver='ccd')")
    bad = (unstored not in ('zero', 'missing')) if weight is None else not 0.0 < weight < 1.0      # (a NaN fails too)
    if not bad and weight is not None:
        bad = not 0.0 < torch.tensor(weight, dtype=torch.float32).item() < 1.0                     # what the C entry receives
    if bad:
        raise ValueError(f"unstored must be 'zero' or 'missing', or (solver='ccd') the weight of the unstored zeros, a "
                         f"real number strictly between 0 and 1; got {unstored!r}")
    if weight is not None and solver != 'ccd':
        raise NotImplementedError(f"unstored={unstored!r}: confidence-weighted unstored zeros are fitted by "
                                  f"solver='ccd' only (beta = 2), not by solver={solver!r}")
    return 1.0 if solver == 'hals' else (0.0 if weight is None else weight)


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
    return _fold(W, target, beta, max_iter, tol, alpha, l1_ratio, unstored, 'mu', H0, generator, return_n_iter, _block,
                 _long_rows, _fill)


def fold_in_cd(W: Tensor, target, beta: float = 2, max_iter: int = 200, tol: float = 1e-4, alpha: float = 0,
               l1_ratio: float = 0, *, unstored='missing', solver: str = 'ccd', H0: Tensor = None, generator=None,
               return_n_iter: bool = False, _block: int = 0, _long_rows: int = 0, _fill=None):
    """``fold_in`` by cyclic coordinate descent (beta = 2): ``H_new [n_new, R]`` (detached, dtype of ``W``) for the rows of
    ``target`` against the fixed ``W (C, R)``, every iteration of every row in one launch of ``nmfmu_fold_in_cd``; arguments,
    stop rule, return value and promises as for ``fold_in``.

    ``solver='ccd'`` with ``unstored='missing'`` (the stored entries only) or a real number strictly between 0 and 1, the
    confidence of the unstored zeros -- the objective of ``fit(solver='ccd', unstored=...)``; ``solver='hals'`` with
    ``unstored='zero'``.  ``H0`` is used as it is: unlike ``fit(solver='ccd')`` there is NO initial scaling -- the
    coordinate step is an exact minimiser and needs none.  Under 'missing' a row without stored entries is returned as it
    came; for a weight or 'zero' it is swept to the floor.  The refusals are ``fit``'s, in its words; ``solver='mu'`` is
    ``fold_in`` itself."""
    return _fold(W, target, beta, max_iter, tol, alpha, l1_ratio, unstored, solver, H0, generator, return_n_iter, _block,
                 _long_rows, _fill)


def _fold(W, target, beta, max_iter, tol, alpha, l1_ratio, unstored, solver, H0, generator, return_n_iter, _block, _long_rows,
          _fill):
    what = 'fold_in'
    if solver not in SOLVERS:
        raise ValueError(f"solver must be 'mu', 'hals' or 'ccd', got {solver!r}")
    cd = solver != 'mu'
    if cd:
        omega = _cd_omega(solver, beta, unstored)
    elif not isinstance(unstored, str) or unstored not in MODES:
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
    if not cd and beta <= 0 and (unstored == 'zero' or lo == 0):
        raise ValueError(_BETA_TEXT)
    if not cd and unstored == 'zero' and beta not in (1.0, 2.0):
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
        if cd:
            if omega > 0:                           # one Gram matrix per fold-in
                aux = torch.empty(R * R, dtype=torch.float32, device=dev)
                part = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device=dev)
                _capi.check(lib.nmfmu_gram(Wc.data_ptr(), Cc, R, part.data_ptr(), aux.data_ptr(), _stream()), 'nmfmu_gram')
        elif unstored == 'zero' and beta == 1.0:    # nmf.py:128-131: W.sum(0)
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
        if cd:
            _capi.check(lib.nmfmu_fold_in_cd(rowptr.data_ptr(), spare.data_ptr(), vals.data_ptr() if nnz else spare.data_ptr(),
                                             n_new, H.data_ptr(), Wc.data_ptr(), Cc, R,
                                             aux.data_ptr() if aux is not None else None, omega, l1, l2, max_iter, float(tol),
                                             n_iter.data_ptr(), order.data_ptr(), int(_block), int(_long_rows), _stream()),
                        'nmfmu_fold_in_cd')
        else:
            _capi.check(lib.nmfmu_fold_in(rowptr.data_ptr(), spare.data_ptr(), vals.data_ptr() if nnz else spare.data_ptr(),
                                          n_new, H.data_ptr(), Wc.data_ptr(), Cc, R, beta, MODES[unstored],
                                          aux.data_ptr() if aux is not None else None, l1, l2, mu_gamma(beta), max_iter,
                                          float(tol), n_iter.data_ptr(), order.data_ptr(), int(_block), int(_long_rows),
                                          _stream()), 'nmfmu_fold_in')
    else:
        n_iter.zero_()
    out = H if W.dtype == torch.float32 else H.to(W.dtype)
    return (out, n_iter) if return_n_iter else out
