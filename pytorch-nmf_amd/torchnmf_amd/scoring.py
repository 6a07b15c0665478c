"""Scoring a fitted model without the ``N x C`` product.

``score_pairs(H, W, rows, cols)``            the model's value ``<H[rows[p]], W[cols[p]]>`` at (row, column) pairs --
                                             held-out evaluation (``nmfmu_score_pairs``)
``topk_scores(H, W, k, rows, exclude)``      the ``k`` best admissible columns of every requested row -- recommendation,
                                             retrieval (``nmfmu_topk``: an exact-fp32 MFMA GEMM fused with the selection)

``rank_scores(H, W, heldout, exclude)``      the rank of every held-out (row, column) pair among ALL admissible columns of
                                             its row, under ``topk_scores``'s order (``nmfmu_rank_pairs``: the same score
                                             tile, counted instead of selected)
``ranking_metrics(H, W, heldout, ks, ...)``  recall@k / precision@k / ndcg@k for any k, MRR and AUC from those ranks

All read the fp32 factors ``H`` (N, R) and ``W`` (C, R) directly; nothing of size ``N x C`` or ``n_rows x C`` is allocated.
Outputs are detached: there is no autograd here (a held-out *loss* with gradients is ``sparse_beta_div(...,
unstored='missing')`` on a test-set ``SparseTarget``).  Scores are taken to be finite: ``-inf`` marks an inadmissible
column inside the kernel, so a score of ``-inf`` or NaN is never returned.

The argument checks run before any device work, in the order of ``_check_*`` below; the index range check is the one host
synchronisation of a call (a min / max of the index tensors).
"""
from __future__ import annotations

from collections import namedtuple

import torch
from torch import Tensor

from . import _capi
from .sparse_autograd import MAX_RANK, SparseTarget

MAX_K = 128          # the partial kernel keeps ceil(k / 64) <= 2 list entries per lane
TILE_ROWS = 64       # csrc/nmfmu_score.hip: kTopRows
TILE_COLS = 128      # csrc/nmfmu_score.hip: kTopCols

RANK_SCAN_ABOVE = 24  # csrc/nmfmu_rank.hip: kRkScanAbove -- rows with more held-out pairs count by the per-lane scan

TopK = namedtuple('topk_scores', ['values', 'indices'])
Ranks = namedtuple('rank_scores', ['rows', 'cols', 'ranks', 'scores', 'admissible'])


def choose_nsplit(n_rows: int, C: int, n_cu: int) -> int:
    """Column ranges per row block: enough workgroups for about two per CU, never more than there are column tiles, never
    fewer than 1.  A pure function of its arguments."""
    row_blocks = max(1, -(-int(n_rows) // TILE_ROWS))
    tiles = max(1, -(-int(C) // TILE_COLS))
    want = -(-2 * max(1, int(n_cu)) // row_blocks)
    return max(1, min(want, tiles))


# ---- argument checks (before anything touches the device) ---------------------------------------------------------------------
def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f'k must be an int >= 1, got {k!r}')
    if k > MAX_K:
        raise NotImplementedError(f'k = {k} > {MAX_K}, the limit of the top-k kernel (scoring.MAX_K)')
    return k


def _check_rank(H: Tensor, W: Tensor, what: str) -> None:
    for f in (H, W):
        if isinstance(f, Tensor) and f.dim() == 2 and f.shape[1] > MAX_RANK:
            raise NotImplementedError(f'{what}: rank {f.shape[1]} > {MAX_RANK}, the limit of the sparse kernels')


def _check_factor_shapes(H: Tensor, W: Tensor, what: str) -> None:
    if not (isinstance(H, Tensor) and isinstance(W, Tensor) and H.dim() == 2 and W.dim() == 2 and H.shape[1] == W.shape[1]
            and min(H.shape + W.shape) > 0):
        raise ValueError(f'{what}: H must be (N, R) and W (C, R) with N, C, R >= 1')
    if max(H.shape[0], W.shape[0]) >= 2 ** 31:
        raise ValueError(f'{what}: N and C must be below 2^31')


def _check_index_dtype(what: str, **idx) -> None:
    for name, t in idx.items():
        if t is not None and t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'{what}: {name} must be an int32 or int64 tensor, got {t.dtype}')


def _check_factor_dtype(H: Tensor, W: Tensor, what: str) -> None:
    if not (H.dtype.is_floating_point and W.dtype.is_floating_point):
        raise TypeError(f'{what}: factors must be floating point; got H {H.dtype}, W {W.dtype}')


def _check_device(what: str, *tensors) -> None:
    for t in tensors:
        if t is not None and t.device.type != 'cuda':
            raise _capi.NmfmuError(f'{what}: tensors must live on the ROCm device (no CPU fallback)')
    devs = {t.device for t in tensors if t is not None}
    if len(devs) > 1:
        raise _capi.NmfmuError(f'{what}: tensors must live on the same device, got {sorted(map(str, devs))}')


def _check_range(what: str, t: Tensor, n: int, name: str) -> None:
    """One host synchronisation per index tensor."""
    if t.numel():
        lo, hi = torch.aminmax(t)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= n:
            raise IndexError(f'{what}: {name} must lie in [0, {n}), got [{lo}, {hi}]')


def _f32(x: Tensor) -> Tensor:
    return x.detach().float().contiguous()


def _i32(x: Tensor) -> Tensor:
    return x.detach().to(torch.int32).contiguous()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- pairs -------------------------------------------------------------------------------------------------------------------
def score_pairs(H: Tensor, W: Tensor, rows: Tensor, cols: Tensor) -> Tensor:
    """fp32 ``[n]`` with ``out[p] = <H[rows[p]], W[cols[p]]>``.  ``rows`` / ``cols``: 1-D int32 or int64 device tensors of
    equal length, in any order, repeats allowed; ``n = 0`` gives an empty tensor.  Rank <= 256.  One host synchronisation
    (the index range check)."""
    what = 'score_pairs'
    _check_rank(H, W, what)
    _check_factor_shapes(H, W, what)
    if not (isinstance(rows, Tensor) and isinstance(cols, Tensor) and rows.dim() == 1 and cols.dim() == 1
            and rows.shape == cols.shape):
        raise ValueError(f'{what}: rows and cols must be 1-D tensors of equal length')
    _check_index_dtype(what, rows=rows, cols=cols)
    _check_factor_dtype(H, W, what)
    _check_device(what, H, W, rows, cols)
    N, C, R = H.shape[0], W.shape[0], H.shape[1]
    _check_range(what, rows, N, 'rows')
    _check_range(what, cols, C, 'cols')
    n = rows.numel()
    out = torch.empty(n, dtype=torch.float32, device=H.device)
    if n == 0:
        return out
    Hc, Wc, r32, c32 = _f32(H), _f32(W), _i32(rows), _i32(cols)
    _capi.check(_capi.load().nmfmu_score_pairs(r32.data_ptr(), c32.data_ptr(), n, Hc.data_ptr(), N, Wc.data_ptr(), C, R,
                                               out.data_ptr(), _stream()), 'nmfmu_score_pairs')
    return out


# ---- top k -------------------------------------------------------------------------------------------------------------------
def _exclude_csr(exclude, dev):
    """(rowptr int32 [N + 1], colidx int32 [nnz]) of the pattern; a stored zero counts."""
    if isinstance(exclude, SparseTarget):
        return exclude.csr[0], exclude.csr[1]
    E = exclude.detach().coalesce()
    idx = E.indices()
    rowptr = torch.zeros(E.shape[0] + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=E.shape[0]), 0)
    return rowptr.to(torch.int32).contiguous(), idx[1].to(torch.int32).contiguous()


def topk_scores(H: Tensor, W: Tensor, k: int, rows: Tensor = None, exclude=None, *, _nsplit=None, _fill=None) -> TopK:
    """``(values fp32 [n_rows, k], indices int64 [n_rows, k])``: for every requested row ``i`` (``rows=None``: all ``N`` rows
    in order; else a 1-D int32 / int64 device tensor, any order, repeats allowed) the ``k`` largest ``<H[i], W[j]>`` over the
    admissible columns ``j``.  ``exclude``: a 2-D sparse-COO tensor (N, C) or a ``metrics.SparseTarget`` -- every stored
    position of it is inadmissible (pattern only; a stored zero counts); typically the training target.

    The order is total: score descending, equal fp32 scores by ascending column.  A row with fewer than ``k`` admissible
    columns ends in ``(-inf, -1)``.  ``k <= scoring.MAX_K``, rank <= 256.  The result is bitwise independent of how the
    columns are split over workgroups.  One host synchronisation when ``rows`` is given (its range check).

    ``_nsplit`` / ``_fill`` are for the tests: force the number of column ranges; pre-fill outputs and workspace."""
    what = 'topk_scores'
    k = _check_k(k)
    _check_rank(H, W, what)
    _check_factor_shapes(H, W, what)
    N, C, R = H.shape[0], W.shape[0], H.shape[1]
    if exclude is not None:
        if not (isinstance(exclude, SparseTarget) or (isinstance(exclude, Tensor) and exclude.is_sparse)):
            raise TypeError(f'{what}: exclude must be a 2-D sparse COO tensor or a SparseTarget')
        if tuple(exclude.shape) != (N, C):
            raise ValueError(f'{what}: exclude {tuple(exclude.shape)} does not match (N, C) = {(N, C)}')
    if rows is not None and not (isinstance(rows, Tensor) and rows.dim() == 1):
        raise ValueError(f'{what}: rows must be a 1-D tensor')
    _check_index_dtype(what, rows=rows)
    _check_factor_dtype(H, W, what)
    _check_device(what, H, W, rows, exclude)
    if rows is not None:
        _check_range(what, rows, N, 'rows')
    dev = H.device
    n_rows = N if rows is None else rows.numel()
    val = torch.empty(n_rows, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n_rows, k, dtype=torch.int32, device=dev)
    if n_rows == 0:
        return TopK(val, idx.long())
    lib = _capi.load()
    if _nsplit is None:
        _nsplit = choose_nsplit(n_rows, C, torch.cuda.get_device_properties(dev).multi_processor_count)
    nsplit = int(_nsplit)
    n_bytes = lib.nmfmu_topk_ws(n_rows, k, nsplit)
    ws = torch.empty(n_bytes // 4, dtype=torch.float32, device=dev) if n_bytes else None
    if _fill is not None:
        val.fill_(_fill)
        idx.fill_(-7)
        if ws is not None:
            ws.fill_(_fill)
    Hc, Wc = _f32(H), _f32(W)
    r32 = _i32(rows) if rows is not None else None
    rowptr, colidx = _exclude_csr(exclude, dev) if exclude is not None else (None, None)
    # (a pattern without a stored entry has an empty column array, whose pointer is null; no range of rowptr reads it, so
    # any valid address serves)
    _capi.check(lib.nmfmu_topk(Hc.data_ptr(), N, r32.data_ptr() if r32 is not None else None, n_rows, Wc.data_ptr(), C, R, k,
                               rowptr.data_ptr() if rowptr is not None else None,
                               (colidx.data_ptr() if colidx.numel() else rowptr.data_ptr()) if colidx is not None else None,
                               nsplit, ws.data_ptr() if ws is not None else None, val.data_ptr(), idx.data_ptr(),
                               _stream()), 'nmfmu_topk')
    return TopK(val, idx.long())


# ---- full ranking ------------------------------------------------------------------------------------------------------------
def _check_ks(ks) -> tuple:
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f'ks must be a sequence of ints >= 1, got {ks!r}') from None
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f'ks must hold ints >= 1, got {k!r}')
    return ks


def _check_pattern(what: str, name: str, P, N: int, C: int) -> None:
    if not (isinstance(P, SparseTarget) or (isinstance(P, Tensor) and P.is_sparse)):
        raise ValueError(f'{what}: {name} must be a 2-D sparse COO tensor or a SparseTarget')
    if tuple(P.shape) != (N, C):
        raise ValueError(f'{what}: {name} {tuple(P.shape)} does not match (N, C) = {(N, C)}')


def _check_rank_args(what: str, H, W, heldout, exclude) -> None:
    _check_rank(H, W, what)
    _check_factor_shapes(H, W, what)
    _check_pattern(what, 'heldout', heldout, H.shape[0], W.shape[0])
    if exclude is not None:
        _check_pattern(what, 'exclude', exclude, H.shape[0], W.shape[0])
    _check_factor_dtype(H, W, what)
    _check_device(what, H, W, heldout, exclude)


class _RankPlan:
    """What one ``nmfmu_rank_pairs`` call reads and writes; ``args`` is its argument list (tools/bench_rank.py times the
    passes apart through ``nmfmu_rank_pass(pass, form, *args)``).  ``args`` is None when there is no held-out pair."""

    def __init__(self, H: Tensor, W: Tensor, heldout, exclude, nsplit=None, fill=None):
        dev = H.device
        N, C, R = H.shape[0], W.shape[0], H.shape[1]
        h_rowptr, self.colidx = _exclude_csr(heldout, dev)
        counts = torch.diff(h_rowptr)
        self.n = n = self.colidx.numel()
        self.rows = torch.repeat_interleave(torch.arange(N, device=dev), counts.long())      # coalesced order: row-major
        self.ex = _exclude_csr(exclude, dev) if exclude is not None else None
        self.admissible = torch.full((N,), C, dtype=torch.int64, device=dev)
        if self.ex is not None:
            self.admissible -= torch.diff(self.ex[0]).long()
        self.scores = torch.empty(n, dtype=torch.float32, device=dev)
        self.ranks = torch.empty(n, dtype=torch.int32, device=dev)
        self.args = None
        if n == 0:
            return
        self.row_ids = torch.nonzero(counts).flatten().to(torch.int32)      # the rows with held-out pairs (one host sync)
        self.n_rows = n_rows = self.row_ids.numel()
        # rows without a pair have equal consecutive pointers: the pointers of the kept rows are already the compact CSR
        self.ho_rowptr = torch.cat([h_rowptr[self.row_ids.long()], h_rowptr[-1:]]).contiguous()
        if nsplit is None:
            nsplit = choose_nsplit(n_rows, C, torch.cuda.get_device_properties(dev).multi_processor_count)
        self.nsplit = int(nsplit)
        self.ws = torch.empty(_capi.load().nmfmu_rank_ws(n, n_rows, self.nsplit) // 4, dtype=torch.int32, device=dev)
        self.adm_rows = torch.empty(n_rows, dtype=torch.int32, device=dev)
        if fill is not None:
            self.scores.fill_(fill)
            self.ranks.fill_(-7)
            self.adm_rows.fill_(-7)
            self.ws.fill_(0x7f7f7f7f)
        self.Hc, self.Wc = _f32(H), _f32(W)
        rowptr, colidx = self.ex if self.ex is not None else (None, None)
        # (an exclusion pattern without a stored entry: see topk_scores)
        self.args = (self.Hc.data_ptr(), N, self.row_ids.data_ptr(), n_rows, self.Wc.data_ptr(), C, R,
                     self.ho_rowptr.data_ptr(), self.colidx.data_ptr(),
                     rowptr.data_ptr() if rowptr is not None else None,
                     (colidx.data_ptr() if colidx.numel() else rowptr.data_ptr()) if colidx is not None else None,
                     self.nsplit, self.ws.data_ptr(), self.scores.data_ptr(), self.ranks.data_ptr(), self.adm_rows.data_ptr())

    def result(self) -> Ranks:
        if self.args is not None:
            self.admissible[self.row_ids.long()] = self.adm_rows.long()
        return Ranks(self.rows, self.colidx.long(), self.ranks.long(), self.scores, self.admissible)


def rank_scores(H: Tensor, W: Tensor, heldout, exclude=None, *, _nsplit=None, _fill=None, _form=None) -> Ranks:
    """``Ranks(rows int64 [n], cols int64 [n], ranks int64 [n], scores fp32 [n], admissible int64 [N])``: for every stored
    position ``(i, c)`` of ``heldout`` (a 2-D sparse-COO tensor (N, C) or a ``metrics.SparseTarget``; pattern only), in its
    coalesced order, the number of admissible columns ``j != c`` of row ``i`` that come before ``c`` in ``topk_scores``'s total
    order -- ``s_ij > s_ic``, or equal fp32 scores and ``j < c`` (0-based).  A column is admissible when ``exclude`` (same
    types, pattern only, a stored zero counts) does not store it; the other held-out columns of the row compete like any
    other column.  A pair that ``exclude`` also stores gets rank ``-1`` (its score is still returned).  ``admissible[i]`` is
    the number of admissible columns of row ``i``, for every row.

    ``scores`` are the bits ``topk_scores`` returns for that (row, column), so ``rank < k`` exactly when the column is among
    ``topk_scores(H, W, k, exclude=exclude)``'s indices of the row.  Rank <= 256; factors are taken to be finite.  The result
    is bitwise independent of how the columns are split over workgroups.  One host synchronisation (the rows with pairs).

    ``_nsplit`` / ``_fill`` / ``_form`` are for the tests and the benchmark: force the number of column ranges; pre-fill
    outputs and workspace; force the form of the count (1: one ballot per threshold, 2: the per-lane scan)."""
    what = 'rank_scores'
    _check_rank_args(what, H, W, heldout, exclude)
    plan = _RankPlan(H, W, heldout, exclude, _nsplit, _fill)
    if plan.args is not None:
        lib = _capi.load()
        if _form is None:
            _capi.check(lib.nmfmu_rank_pairs(*plan.args, _stream()), 'nmfmu_rank_pairs')
        else:
            for p in range(3):
                _capi.check(lib.nmfmu_rank_pass(p, int(_form), *plan.args, _stream()), 'nmfmu_rank_pass')
    return plan.result()


def metrics_from_ranks(r: Ranks, ks=(10,)) -> dict:
    """The metrics of ``ranking_metrics`` from the output of ``rank_scores``: integer hit counts, float64 sums, torch ops on
    ``[n]`` and ``[N]`` tensors."""
    ks = _check_ks(ks)
    dev, N = r.ranks.device, r.admissible.numel()
    f64 = dict(dtype=torch.float64, device=dev)
    valid = r.ranks >= 0
    row, rk = r.rows[valid], r.ranks[valid]
    t = torch.bincount(row, minlength=N)
    use = t > 0
    tu = t[use]
    tf = tu.double()
    out = {}
    t_max = int(t.max()) if N else 0
    for k in ks:
        hit = rk < k
        hits = torch.bincount(row[hit], minlength=N)[use]
        out[f'recall@{k}'] = (hits.double() / tf).mean()
        out[f'precision@{k}'] = (hits.double() / k).mean()
        dcg = torch.zeros(N, **f64).index_add_(0, row[hit], 1.0 / torch.log2(rk[hit].double() + 2.0))[use]
        # ideal[p] = sum_{q < p} 1 / log2(q + 2): the row's min(k, t) pairs at the top
        m = min(k, t_max)
        ideal = torch.cat([torch.zeros(1, **f64), torch.cumsum(1.0 / torch.log2(torch.arange(m, **f64) + 2.0), 0)])
        out[f'ndcg@{k}'] = (dcg / ideal[tu.clamp(max=k)]).mean()
    best = torch.full((N,), 2 ** 62, dtype=torch.int64, device=dev).scatter_reduce_(0, row, rk, 'amin')[use]
    out['mrr'] = (1.0 / (1.0 + best.double())).mean()
    neg = (r.admissible[use] - tu)
    above = torch.zeros(N, dtype=torch.int64, device=dev).index_add_(0, row, rk)[use] - tu * (tu - 1) // 2
    ok = neg > 0
    out['auc'] = (1.0 - above[ok].double() / (tf[ok] * neg[ok].double())).mean()
    out['rows'] = use.sum().double()
    return out


def ranking_metrics(H: Tensor, W: Tensor, heldout, ks=(10,), exclude=None) -> dict:
    """Full-ranking metrics of the held-out pairs as 0-dim float64 device tensors: ``'recall@k'``, ``'precision@k'``,
    ``'ndcg@k'`` for every ``k`` in ``ks`` (any int >= 1, not limited to ``MAX_K``), ``'mrr'``, ``'auc'`` and ``'rows'``.  They
    are means over the rows with at least one valid held-out pair (rank >= 0), ``'rows'`` is the number of such rows.  Per
    row, with ``t`` valid pairs of ranks ``r_e``: recall@k = #{r_e < k} / t; precision@k = #{r_e < k} / k; ndcg@k =
    sum_{r_e < k} 1 / log2(r_e + 2) over sum_{p < min(k, t)} 1 / log2(p + 2); mrr = 1 / (1 + min r_e); auc = 1 - (sum r_e -
    t (t - 1) / 2) / (t (admissible - t)), a row with admissible == t left out of the AUC mean.  Without such rows a mean
    is NaN."""
    ks = _check_ks(ks)
    _check_rank_args('ranking_metrics', H, W, heldout, exclude)
    return metrics_from_ranks(rank_scores(H, W, heldout, exclude), ks)
