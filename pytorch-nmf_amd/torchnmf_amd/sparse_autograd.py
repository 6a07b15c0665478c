"""``sparse_beta_div``: the reference's sparse loss ``V_norm + pos - neg`` (nmf.py:162-181, 617-638) as a differentiable
function of the factors, for beta in {1, 2} -- ``torch.optim`` and ``trainer.SparsityProj`` on sparse-COO targets.

Only the stored entries of the target are touched: the dense ``N x C`` reconstruction never exists.

  forward   neg = sum v log(s + eps) | sum v s over the stored entries (``nmfmu_sp_div_forward``, one wave per row segment),
            pos = colsum(W) . colsum(H) (``nmfmu_rank_sums``) | 1/2 sum(H^T H * W^T W) (``nmfmu_gram``)
  backward  grad_H[i] = up (colsum(W) - sum_j v_ij / (s_ij + eps) W[j])   |   up (H[i] W^T W - sum_j v_ij W[j])
            and the same with the roles swapped (``nmfmu_sp_div_backward``, once per wanted side; the beta == 2 planes from
            ``nmfmu_rowmat``)

``unstored='missing'`` reads the target as missing data instead: its unstored entries are unknown, not zero, and the loss is
the reference's ``beta_div`` over the stored entries alone -- any beta, O(nnz R):

  forward   ``nmfmu_sp_masked_loss`` (the terms of v alone once per target on the host, float64)
  backward  grad = up (den - num), the two planes of ``nmfmu_sp_masked_terms`` (one call per wanted side): the raw sums of
            the masked multiplicative update, without its relu / eps

The planning functions below are pure torch and run on CPU tensors as well; everything else needs the ROCm device.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _capi

DEFAULT_CHUNK = 512      # stored entries per segment
MAX_RANK = 256           # the limit of the sparse kernels


# ---- planning (pure torch, any device) ---------------------------------------------------------------------------------------
def segment_counts(rowptr: Tensor, chunk: int) -> Tensor:
    """Segments per row: ceil(count / chunk), and 1 for a row without entries (every row has exactly one writer)."""
    counts = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    return torch.clamp((counts + (chunk - 1)) // chunk, min=1)


def plan_segments(rowptr: Tensor, chunk: int = DEFAULT_CHUNK) -> Tensor:
    """int32 ``[n_seg, 3]`` = (row, p_begin, p_end): every row cut into consecutive runs of at most ``chunk`` stored entries,
    in row order.  A pure function of ``rowptr`` and ``chunk``."""
    chunk = int(chunk)
    assert chunk >= 1, 'chunk must be at least 1'
    rp = rowptr.to(torch.int64)
    n_rows = rp.numel() - 1
    nsegs = segment_counts(rp, chunk)
    rows = torch.repeat_interleave(torch.arange(n_rows, device=rp.device), nsegs)
    first = torch.cumsum(nsegs, 0) - nsegs
    k = torch.arange(rows.numel(), device=rp.device) - first[rows]
    p0 = rp[rows] + k * chunk
    p1 = torch.minimum(p0 + chunk, rp[rows + 1])
    return torch.stack([rows, p0, p1], 1).to(torch.int32).contiguous()


def plan_worklist(rowptr: Tensor, chunk: int = DEFAULT_CHUNK):
    """(seg int32 [n_seg, 4], multi int32 [n_multi, 3], n_multi_segments): ``plan_segments`` with the workspace slot of every
    segment as a fourth column (-1: the row's only segment) and the (row, first slot, segments) list of the split rows --
    the two lists of include/nmfmu.h."""
    seg3 = plan_segments(rowptr, chunk).to(torch.int64)
    nsegs = segment_counts(rowptr.to(torch.int64), int(chunk))
    split = nsegs > 1
    used = torch.where(split, nsegs, torch.zeros_like(nsegs))
    slot0 = torch.cumsum(used, 0) - used
    rows = seg3[:, 0]
    first = torch.cumsum(nsegs, 0) - nsegs
    k = torch.arange(rows.numel(), device=rows.device) - first[rows]
    slot = torch.where(split[rows], slot0[rows] + k, torch.full_like(k, -1))
    seg = torch.cat([seg3, slot[:, None]], 1).to(torch.int32).contiguous()
    mrows = torch.nonzero(split).reshape(-1)
    multi = torch.stack([mrows, slot0[mrows], nsegs[mrows]], 1).to(torch.int32).contiguous()
    return seg, multi, int(used.sum())


def workspace_floats(n_multi_segments: int, r_pad: int) -> int:
    """The rule of ``nmfmu_sp_div_backward_ws``: one partial row of ``r_pad`` floats per segment of a split row."""
    return int(n_multi_segments) * int(r_pad) if n_multi_segments > 0 and r_pad > 0 else 0


def csr_csc(rows: Tensor, cols: Tensor, vals: Tensor, n_rows: int, n_cols: int):
    """From coalesced COO entries (sorted by (row, col)): ``(rowptr, colidx, vals)``, ``(colptr, rowidx, vals_csc)`` and
    ``perm`` with ``vals_csc[p] == vals[perm[p]]`` -- the CSR position of CSC entry ``p``.  Index arrays are int32."""
    rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    dev = rows.device

    def ptr(idx, n):
        out = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        out[1:] = torch.cumsum(torch.bincount(idx, minlength=n), 0)
        return out.to(torch.int32).contiguous()
    perm = torch.argsort(cols * n_rows + rows)         # keys are distinct after coalescing
    csr = (ptr(rows, n_rows), cols.to(torch.int32).contiguous(), vals.contiguous())
    csc = (ptr(cols, n_cols), rows[perm].to(torch.int32).contiguous(), vals[perm].contiguous())
    return csr, csc, perm.to(torch.int32).contiguous()


def masked_workspace_floats(n_multi_segments: int, r_pad: int) -> int:
    """The rule of ``nmfmu_sp_masked_ws``: one partial [num | den] row of ``2 r_pad`` floats per segment of a split row."""
    return int(n_multi_segments) * 2 * int(r_pad) if n_multi_segments > 0 and r_pad > 0 else 0


def masked_v_term(vals: Tensor, beta: float) -> float:
    """The terms of ``metrics.beta_div(s, v, beta)`` that hold v alone (metrics.py:22, 39, 57, 85-96), in float64 -- what
    ``nmfmu_sp_masked_loss`` takes as ``v_term``."""
    from .constants import eps
    vd = vals.double()
    if beta == 2.0:
        return 0.0
    if beta == 1.0:
        return float((vd @ (vd + eps).log() - vd.sum()).item())
    if beta == 0.0:
        return float((-(vd + eps).log().sum()).item()) - vd.numel()
    return float((vd + eps if beta < 0 else vd).pow(beta).sum().item())


def v_norm(vals: Tensor, beta: float) -> float:
    """nmf.py:172-181 over the stored values in float64 (``SparseMU`` and ``SparseTarget`` both take it from here)."""
    vd = vals.double()
    if beta == 1.0:
        return float((vd @ vd.log() - vd.sum()).item())
    if beta == 2.0:
        return float((vd @ vd).item() * 0.5)
    return float(vd.pow(beta).sum().item() / beta / (beta - 1))


def entries(t: Tensor, spare: Tensor) -> int:
    """Pointer to an entry array (column indices, values, perm).  A target without a stored entry has empty tensors, whose
    pointer is null; the kernels never read past the ranges of rowptr / the segments, so any valid address -- ``spare`` --
    serves them."""
    return t.data_ptr() if t.numel() else spare.data_ptr()


# ---- argument checks (run before anything touches the device) -----------------------------------------------------------------
def check_beta(beta) -> float:
    beta = float(beta)
    if not beta > 0:
        raise ValueError('When beta <= 0 and V contains zeros, the training process may diverge. '
                         'Please add small values to V, or use a positive beta value.')
    if beta not in (1.0, 2.0):
        raise NotImplementedError(f'sparse_beta_div supports beta in {{1, 2}}, got {beta:g}: for any other beta the positive '
                                  f'term sum (H W^T + eps)^beta / beta is a dense pass over N x C (as in the reference); use '
                                  f'beta_div(m(), V.to_dense(), beta)')
    return beta


class SparseTarget:
    """A sparse-COO target prepared once for ``sparse_beta_div``: coalesced, CSR and CSC copies, the CSC -> CSR permutation
    and the segment work lists of both sides, all on the device.  ``chunk``: stored entries per segment (``None``: rows
    and columns are not split)."""

    def __init__(self, V: Tensor, chunk=DEFAULT_CHUNK):
        assert isinstance(V, Tensor) and V.is_sparse and V.dim() == 2, 'the target must be a 2-D sparse COO tensor'
        V = V.detach().coalesce()
        N, Cc = V.shape
        idx, vals = V.indices(), V.values().float()
        assert V._nnz() < 2 ** 31 and max(N, Cc) < 2 ** 31 and min(N, Cc) > 0
        if vals.numel():
            assert bool((vals >= 0).all().item()), 'Target should be non-negative.'
        if V.device.type != 'cuda':
            raise _capi.NmfmuError('SparseTarget: the target must live on the ROCm device (no CPU fallback)')
        self.shape = (N, Cc)
        self.device = V.device
        self.nnz = int(vals.numel())
        self.vals = vals
        self.csr, self.csc, self.perm = csr_csc(idx[0], idx[1], vals, N, Cc)
        if chunk is None:
            widest = max(int(torch.diff(self.csr[0]).max()), int(torch.diff(self.csc[0]).max()), 1)
            chunk = widest
        self.chunk = int(chunk)
        self.seg_h, self.multi_h, self.n_ws_h = plan_worklist(self.csr[0], self.chunk)
        self.seg_w, self.multi_w, self.n_ws_w = plan_worklist(self.csc[0], self.chunk)
        self.spare = torch.zeros(4, dtype=torch.float32, device=V.device)     # see entries()
        self._v_norm = {}
        self._has_zero = None

    def side(self, side: str):
        """((ptr, idx, vals), seg, multi, n_ws) of one side's work list: 'h' -- the CSR list, owner rows = rows of V; 'w' --
        the CSC list, owner rows = columns of V, values in CSC order."""
        if side == 'h':
            return self.csr, self.seg_h, self.multi_h, self.n_ws_h
        return self.csc, self.seg_w, self.multi_w, self.n_ws_w

    @property
    def has_zero(self) -> bool:
        """Is a STORED value zero?  (Missing-data fits: unstored entries are not zeros.)  Once per target; one host sync."""
        if self._has_zero is None:
            self._has_zero = bool((self.vals == 0).any().item()) if self.nnz else False
        return self._has_zero

    def masked_v_term(self, beta: float) -> float:
        """Once per (target, beta); a Python float."""
        key = ('masked', beta)
        if key not in self._v_norm:
            self._v_norm[key] = masked_v_term(self.vals, beta)
        return self._v_norm[key]

    def v_norm(self, beta: float) -> float:
        """Once per (target, beta); a Python float."""
        if beta not in self._v_norm:
            self._v_norm[beta] = v_norm(self.vals, beta)
        return self._v_norm[beta]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32(x: Tensor) -> Tensor:
    return x.detach().float().contiguous()


def _small_terms(lib, Hc: Tensor, Wc: Tensor, beta: float):
    """(pos as a 0-dim float64 device tensor, the per-factor small terms the backward reuses): column sums (beta 1) or Gram
    matrices (beta 2) of H and of W."""
    R, dev = Hc.shape[1], Hc.device
    out = []
    if beta == 1.0:
        part = torch.empty(R * 128, dtype=torch.float32, device=dev)
        for f in (Hc, Wc):
            cs = torch.empty(R, dtype=torch.float32, device=dev)
            _capi.check(lib.nmfmu_rank_sums(f.data_ptr(), f.shape[0], R, 1, part.data_ptr(), cs.data_ptr(), _stream()),
                        'nmfmu_rank_sums')
            out.append(cs)
        return out[0].double() @ out[1].double(), out
    part = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device=dev)
    for f in (Hc, Wc):
        g = torch.empty(R * R, dtype=torch.float32, device=dev)
        _capi.check(lib.nmfmu_gram(f.data_ptr(), f.shape[0], R, part.data_ptr(), g.data_ptr(), _stream()), 'nmfmu_gram')
        out.append(g)
    return 0.5 * (out[0].double() @ out[1].double()), out


def _forward(Hc: Tensor, Wc: Tensor, T: SparseTarget, beta: float, want_s: bool):
    """(loss 0-dim fp32, s | None, small terms).  Enqueued only: no host synchronisation."""
    lib = _capi.load()
    dev = Hc.device
    R = Hc.shape[1]
    rowptr, colidx, vals = T.csr
    n_seg = T.seg_h.shape[0]
    s = torch.empty(max(T.nnz, 1), dtype=torch.float32, device=dev) if want_s else None
    part = torch.empty((n_seg + 3) // 4, dtype=torch.float64, device=dev)
    neg = torch.empty(1, dtype=torch.float64, device=dev)
    _capi.check(lib.nmfmu_sp_div_forward(T.seg_h.data_ptr(), n_seg, entries(colidx, T.spare), entries(vals, T.spare),
                                         Hc.data_ptr(), Wc.data_ptr(), R, beta, s.data_ptr() if want_s else None,
                                         part.data_ptr(), neg.data_ptr(), _stream()), 'nmfmu_sp_div_forward')
    pos, small = _small_terms(lib, Hc, Wc, beta)
    return (T.v_norm(beta) + pos - neg[0]).float(), s, small


def _backward_side(owner: Tensor, panel: Tensor, small_panel: Tensor, T: SparseTarget, side: str, beta: float, s, up: Tensor,
                   _fill=None):
    """grad of one factor, fp32 ``[owner rows, R]``.  ``_fill``: tests pre-fill the output and the workspace with it."""
    lib = _capi.load()
    dev = owner.device
    rows, R = owner.shape
    r_pad = lib.nmfmu_pad_rank(R)
    if side == 'h':
        (ptr, idx, vals), seg, multi, n_ws, perm = T.csr, T.seg_h, T.multi_h, T.n_ws_h, None
    else:
        (ptr, idx, vals), seg, multi, n_ws, perm = T.csc, T.seg_w, T.multi_w, T.n_ws_w, T.perm
    if beta == 1.0:
        pos, plane = small_panel, 0                       # the panel's column sums, broadcast over the rows
    else:
        pos, plane = torch.empty(rows * r_pad, dtype=torch.float32, device=dev), 1
        _capi.check(lib.nmfmu_rowmat(owner.data_ptr(), rows, R, small_panel.data_ptr(), pos.data_ptr(), r_pad, _stream()),
                    'nmfmu_rowmat')
    out = torch.empty(rows, r_pad, dtype=torch.float32, device=dev)
    n_float = lib.nmfmu_sp_div_backward_ws(n_ws, r_pad)
    ws = torch.empty(n_float, dtype=torch.float32, device=dev) if n_float else None
    if _fill is not None:
        out.fill_(_fill)
        if ws is not None:
            ws.fill_(_fill)
    _capi.check(lib.nmfmu_sp_div_backward(seg.data_ptr(), seg.shape[0], multi.data_ptr() if multi.shape[0] else None,
                                          multi.shape[0], entries(idx, T.spare), entries(vals, T.spare),
                                          entries(perm, T.spare) if perm is not None else None,
                                          s.data_ptr() if s is not None else None, panel.data_ptr(), R, beta,
                                          pos.data_ptr(), plane, up.data_ptr(), ws.data_ptr() if ws is not None else None,
                                          out.data_ptr(), r_pad, _stream()), 'nmfmu_sp_div_backward')
    return out if r_pad == R else out[:, :R].contiguous()


# ---- missing data: the stored entries only ------------------------------------------------------------------------------------
def _masked_call(T: SparseTarget, side: str, owner: Tensor, panel: Tensor, beta: float, step=None, _fill=None, _ws=None):
    """``nmfmu_sp_masked_terms`` (``step`` None: returns (num, den), fp32 ``[owner rows, r_pad]``) or ``nmfmu_sp_masked_step``
    (``step`` = (l1, l2, gamma): ``owner`` updated in place).  ``owner`` / ``panel``: contiguous fp32 ``[rows, R]``.  Enqueued
    only.  ``_fill``: tests pre-fill the outputs and the workspace with it."""
    lib = _capi.load()
    dev = owner.device
    rows, R = owner.shape
    r_pad = lib.nmfmu_pad_rank(R)
    (ptr, idx, vals), seg, multi, n_ws = T.side(side)
    assert rows == ptr.numel() - 1 and panel.shape[1] == R
    n_float = lib.nmfmu_sp_masked_ws(n_ws, r_pad)
    ws = _ws if _ws is not None else (torch.empty(n_float, dtype=torch.float32, device=dev) if n_float else None)
    if _fill is not None and ws is not None:
        ws.fill_(_fill)
    head = (seg.data_ptr(), seg.shape[0], multi.data_ptr() if multi.shape[0] else None, multi.shape[0], entries(idx, T.spare),
            entries(vals, T.spare), owner.data_ptr(), panel.data_ptr(), R, beta)
    wsp = ws.data_ptr() if ws is not None else None
    if step is not None:
        l1, l2, gamma = step
        _capi.check(lib.nmfmu_sp_masked_step(*head, l1, l2, gamma, wsp, r_pad, _stream()), 'nmfmu_sp_masked_step')
        return None
    num = torch.empty(rows, r_pad, dtype=torch.float32, device=dev)
    den = torch.empty(rows, r_pad, dtype=torch.float32, device=dev)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    _capi.check(lib.nmfmu_sp_masked_terms(*head, wsp, num.data_ptr(), den.data_ptr(), r_pad, _stream()),
                'nmfmu_sp_masked_terms')
    return num, den


def _masked_loss(Hc: Tensor, Wc: Tensor, T: SparseTarget, beta: float, part=None, out=None) -> Tensor:
    """``metrics.beta_div`` over the stored entries as a 1-element float64 device tensor.  Enqueued only (the terms of v
    alone are cached on the target after their first use)."""
    lib = _capi.load()
    rowptr, colidx, vals = T.csr
    n_seg = T.seg_h.shape[0]
    if part is None:
        part = torch.empty((n_seg + 3) // 4, dtype=torch.float64, device=Hc.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=Hc.device)
    _capi.check(lib.nmfmu_sp_masked_loss(T.seg_h.data_ptr(), n_seg, entries(colidx, T.spare), entries(vals, T.spare),
                                         Hc.data_ptr(), Wc.data_ptr(), Hc.shape[1], beta, T.masked_v_term(beta),
                                         part.data_ptr(), out.data_ptr(), _stream()), 'nmfmu_sp_masked_loss')
    return out


class _MaskedBetaDivFn(torch.autograd.Function):
    """The masked loss; both gradients are up (den - num) of one ``nmfmu_sp_masked_terms`` call per wanted side."""

    @staticmethod
    def forward(ctx, H, W, T, beta):
        ctx.save_for_backward(H, W)
        ctx.T, ctx.beta = T, beta
        return _masked_loss(_f32(H), _f32(W), T, beta)[0].float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        H, W = ctx.saved_tensors
        Hc, Wc = _f32(H), _f32(W)
        up = g.detach().float()
        R = H.shape[1]

        def grad(side, owner, panel, like):
            num, den = _masked_call(ctx.T, side, owner, panel, ctx.beta)
            return (up * (den - num))[:, :R].to(like.dtype)
        gH = grad('h', Hc, Wc, H) if ctx.needs_input_grad[0] else None
        gW = grad('w', Wc, Hc, W) if ctx.needs_input_grad[1] else None
        return gH, gW, None, None


class _SparseBetaDivFn(torch.autograd.Function):
    """The value from the same launches as without autograd; both gradients from ``nmfmu_sp_div_backward``, which reads the
    0-dim incoming gradient on the device (no host sync)."""

    @staticmethod
    def forward(ctx, H, W, T, beta):
        Hc, Wc = _f32(H), _f32(W)
        loss, s, small = _forward(Hc, Wc, T, beta, want_s=beta == 1.0)
        ctx.save_for_backward(H, W, *small, *([s] if s is not None else []))
        ctx.T, ctx.beta = T, beta
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        H, W, small_h, small_w, *rest = ctx.saved_tensors
        s = rest[0] if rest else None
        Hc, Wc = _f32(H), _f32(W)
        up = g.detach().float().reshape(1).contiguous()
        gH = gW = None
        if ctx.needs_input_grad[0]:
            gH = _backward_side(Hc, Wc, small_w, ctx.T, 'h', ctx.beta, s, up).to(H.dtype)
        if ctx.needs_input_grad[1]:
            gW = _backward_side(Wc, Hc, small_h, ctx.T, 'w', ctx.beta, s, up).to(W.dtype)
        return gH, gW, None, None


def sparse_beta_div(H: Tensor, W: Tensor, target, beta: float = 2, *, unstored: str = 'zero') -> Tensor:
    """beta-divergence between ``H @ W.T`` and a sparse-COO ``target`` (N, C), from the stored entries only: the
    reference's ``V_norm + pos - neg``; beta in {1, 2}, rank <= 256.  ``H`` is (N, R), ``W`` (C, R).  ``target`` is a
    ``SparseTarget`` (prepared once) or a sparse tensor (prepared for this call).  Returns a 0-dim float32 device tensor,
    differentiable with respect to ``H`` and ``W`` (first order); the target is a constant.

    ``unstored='zero'`` (default) counts every unstored entry as an observed zero, like the reference.  ``unstored='missing'``
    leaves them out: the result is the reference's ``beta_div`` between the reconstruction at the stored entries and the
    stored values, for ANY beta (beta <= 0 needs strictly positive stored values)."""
    if unstored not in ('zero', 'missing'):
        raise ValueError(f"unstored must be 'zero' or 'missing', got {unstored!r}")
    missing = unstored == 'missing'
    beta = float(beta) if missing else check_beta(beta)
    assert isinstance(target, SparseTarget) or (isinstance(target, Tensor) and target.is_sparse), \
        'the target must be a SparseTarget or a sparse COO tensor'
    assert H.dim() == 2 and W.dim() == 2 and H.shape[1] == W.shape[1], 'H must be (N, R) and W (C, R)'
    assert tuple(target.shape) == (H.shape[0], W.shape[0]), \
        f'target {tuple(target.shape)} does not match H {tuple(H.shape)} and W {tuple(W.shape)}'
    if H.shape[1] > MAX_RANK:
        raise NotImplementedError(f'sparse_beta_div: rank {H.shape[1]} > {MAX_RANK}, the limit of the sparse kernels')
    if not isinstance(target, SparseTarget):
        target = SparseTarget(target)
    if H.device.type != 'cuda' or W.device.type != 'cuda':
        raise _capi.NmfmuError('sparse_beta_div: tensors must live on the ROCm device (no CPU fallback)')
    assert H.device == W.device == target.device, 'H, W and the target must live on the same device'
    if not (H.dtype.is_floating_point and W.dtype.is_floating_point):
        raise NotImplementedError(f'factors must be floating point; got H {H.dtype}, W {W.dtype}')
    if missing:
        if beta <= 0 and target.has_zero:
            raise ValueError('When beta <= 0 and V contains zeros, the training process may diverge. '
                             'Please add small values to V, or use a positive beta value.')
        if torch.is_grad_enabled() and (H.requires_grad or W.requires_grad):
            return _MaskedBetaDivFn.apply(H, W, target, beta)
        return _masked_loss(_f32(H), _f32(W), target, beta)[0].float()
    if torch.is_grad_enabled() and (H.requires_grad or W.requires_grad):
        return _SparseBetaDivFn.apply(H, W, target, beta)
    return _forward(_f32(H), _f32(W), target, beta, want_s=False)[0]
