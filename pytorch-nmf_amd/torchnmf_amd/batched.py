"""Batched NMF: many independent fits of one shape per launch, each stopped on its own (``BatchedNMF``, ``batched_beta_div``).

``B`` problems ``V_b (N, C) ~ H_b (N, R) @ W_b (C, R)^T`` -- ``B`` targets, or ``B`` random starts on ONE target -- are far
too small, each, to fill an MI355X, and a loop of ``NMF.fit`` calls pays the launch gaps of every one of them.  Here one
half-step of ALL problems is one ``nmfmu_bmu_step`` call on the fp32 masters ``[B, rows, R]`` (csrc/nmfmu_bmu.hip: the
exact-fp32 MFMA tile of the weighted kernels with the problem index as a grid coordinate), the per-problem losses are one
``nmfmu_bmu_loss`` call, and the reference's stop rule (nmf.py:402-407) is applied on the device by ``nmfmu_bmu_judge``: a
problem that stops clears its ``active`` flag, every later kernel leaves at once for it, and its factors stay what they were
at its stop iteration, bit for bit, while the others go on.  The host never decides anything per problem and never syncs per
iteration.

The bits of a problem do not depend on the batch around it: ``fit`` of ``B`` problems gives each exactly what a ``B = 1`` call
gives it, in any order.

``weights`` gives every problem dense per-entry weights or a mask (``NMF.fit(V, weights=M)`` per problem, bit for bit): its own
``(B, N, C)`` slice, one shared ``(N, C)`` matrix, or one of ``G`` matrices picked by ``weight_index`` -- and ``alpha`` /
``l1_ratio`` may differ per problem.  Both go through the ``nmfmu_bwmu_*`` entries: the same launches, the weighted stage of
csrc/nmfmu_wmu.hip in the tile.  ``model_selection.cross_validate`` is built on this.
"""
from __future__ import annotations

from collections.abc import Iterable
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
from torch import Tensor, nn

from . import _capi
from .engine import mu_gamma
from .wmu import check_weights

__all__ = ['BatchedNMF', 'batched_beta_div', 'MAX_RANK', 'target_like']

MAX_RANK = 256


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def workspace_floats(batch: int, rows: int, contraction: int, r_pad: int, nsplit: int = 0) -> int:
    return int(_capi.load().nmfmu_bmu_ws(batch, rows, contraction, r_pad, nsplit))


def _new_batched_factor(spec, trainable: bool, label: str):
    """(Parameter | None, (batch, rank) | None) from a constructor argument: a non-negative 3-D tensor or a shape."""
    if isinstance(spec, Tensor):
        assert spec.dim() == 3, f'Tensor {label} should be (batch, rows, rank), got {tuple(spec.shape)}.'
        assert bool(torch.all(spec >= 0.)), f'Tensor {label} should be non-negative.'
        p = nn.Parameter(torch.empty(*spec.size()), requires_grad=trainable)
        p.data.copy_(spec)
        return p, (p.shape[0], p.shape[2])
    if isinstance(spec, Iterable):
        shape = tuple(spec)
        # like NMF, a shape always yields a trainable factor drawn from |N(0, 1)|
        return nn.Parameter(torch.randn(*shape).abs()), (shape[0], shape[2])
    return None, None


def target_like(shape, device) -> SimpleNamespace:
    """What ``wmu.check_weights`` reads of a target -- its shape and its device -- for weights that are not of ``V``'s shape."""
    return SimpleNamespace(shape=tuple(shape), device=device)


class _Weights(NamedTuple):
    """Checked weights: contiguous fp32 ``M`` (N, C) / (B, N, C) / (G, N, C), its batch stride in floats (0: shared) and the
    int32 ``[B]`` index on ``M``'s device (None: problem b reads slice b)."""
    M: Tensor
    stride: int
    index: Optional[Tensor]


def _check_weights(V: Tensor, weights, weight_index, B: int) -> Optional[_Weights]:
    """``weights`` / ``weight_index`` as ``fit`` and the loss helpers accept them, by ``wmu.check_weights``' rules (bool,
    integer or floating, finite, >= 0, on ``V``'s device; converted to fp32 once).  ``ValueError`` otherwise; None without
    weights."""
    if weights is None:
        if weight_index is not None:
            raise ValueError('weight_index needs weights (G, N, C) to index')
        return None
    N, Cc = V.shape[-2:]
    if not isinstance(weights, Tensor):
        raise ValueError(f'weights must be a tensor ({N}, {Cc}), ({B}, {N}, {Cc}) or (G, {N}, {Cc}) with weight_index, got '
                         f'{type(weights).__name__}')
    if weight_index is None:
        want = tuple(weights.shape) if tuple(weights.shape) in ((N, Cc), (B, N, Cc)) else None
        if want is None or weights.is_sparse:
            raise ValueError(f'weights must be a dense tensor ({N}, {Cc}) shared by every problem or ({B}, {N}, {Cc}), got '
                             f'{"a sparse tensor of shape " if weights.is_sparse else ""}{tuple(weights.shape)}')
        index = None
    else:
        if weights.dim() != 3 or tuple(weights.shape[1:]) != (N, Cc) or weights.shape[0] < 1 or weights.is_sparse:
            raise ValueError(f'weights with weight_index must be a dense tensor (G, {N}, {Cc}), got {tuple(weights.shape)}')
        want = tuple(weights.shape)
        if not isinstance(weight_index, Tensor) or weight_index.dtype.is_floating_point or weight_index.is_complex() \
                or weight_index.dtype == torch.bool:
            raise ValueError(f'weight_index must be an integer tensor [{B}], got '
                             f'{weight_index.dtype if isinstance(weight_index, Tensor) else type(weight_index).__name__}')
        if tuple(weight_index.shape) != (B,):
            raise ValueError(f'weight_index must have one entry per problem [{B}], got {tuple(weight_index.shape)}')
        if weight_index.device != V.device:
            raise ValueError(f'weight_index lives on {weight_index.device}, V on {V.device}')
        lo, hi = int(weight_index.min()), int(weight_index.max())
        if lo < 0 or hi >= want[0]:
            raise ValueError(f'weight_index must lie in [0, {want[0]}), got values in [{lo}, {hi}]')
        index = weight_index.detach().to(torch.int32).contiguous()
    M = check_weights(target_like(want, V.device), weights)
    return _Weights(M, 0 if M.dim() == 2 else N * Cc, index)


def _check_reg(alpha, l1_ratio, B: int):
    """``(l1, l2, reg)`` of nmf.py:348-349: two floats and None for scalar ``alpha`` and ``l1_ratio``; otherwise (0, 0) and the
    per-problem pairs as a float64 ``[B, 2]`` CPU tensor (a float, or a length-``B`` sequence or tensor, each)."""
    def vector(x, name):
        if isinstance(x, Tensor):
            v = x.detach().double().cpu().reshape(-1) if x.dim() else None
        elif isinstance(x, Iterable):
            v = torch.tensor([float(t) for t in x], dtype=torch.float64)
        else:
            v = None
        if v is not None and v.numel() != B:
            raise ValueError(f'{name} must be a float or hold one value per problem [{B}], got {v.numel()}')
        return v
    a, r = vector(alpha, 'alpha'), vector(l1_ratio, 'l1_ratio')
    if a is None and r is None:
        return float(alpha * l1_ratio), float(alpha * (1 - l1_ratio)), None
    a = torch.full((B,), float(alpha), dtype=torch.float64) if a is None else a
    r = torch.full((B,), float(l1_ratio), dtype=torch.float64) if r is None else r
    return 0.0, 0.0, torch.stack([a * r, a * (1 - r)], dim=1)


def _check_target(V, H: Tensor, W: Tensor, device: bool = True) -> None:
    """Everything about the target and the factors that can be judged without the device; raises before any launch.
    ``device`` False leaves the device check (``_check_device``) to the caller, who has more to judge first."""
    if not isinstance(V, Tensor):
        raise ValueError(f'the target must be a tensor (batch, N, C) or (N, C), got {type(V).__name__}')
    if V.is_sparse:
        raise NotImplementedError('BatchedNMF fits dense targets only; a sparse-COO target goes through NMF.fit')
    B, N, R = H.shape
    Cc = W.shape[1]
    if tuple(V.shape) not in ((B, N, Cc), (N, Cc)):
        raise ValueError(f'target {tuple(V.shape)} does not match the model: ({B}, {N}, {Cc}), or ({N}, {Cc}) for one target '
                         f'shared by all {B} problems')
    if R > MAX_RANK:
        raise NotImplementedError(f'BatchedNMF: rank {R} > {MAX_RANK}, the limit of the exact-fp32 kernels')
    if V.dtype != torch.float32:
        raise NotImplementedError(f'BatchedNMF fits fp32 targets only, got {V.dtype} (cast it once with V.float())')
    if H.dtype != torch.float32 or W.dtype != torch.float32:
        raise NotImplementedError(f'BatchedNMF keeps fp32 factors; got W {W.dtype}, H {H.dtype}')
    if device:
        _check_device(V, H, W)


def _check_device(V: Tensor, H: Tensor, W: Tensor) -> None:
    for t in (V, W, H):
        if t.device.type != 'cuda':
            raise _capi.NmfmuError(f'BatchedNMF: tensors live on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'the module and its inputs with .cuda() (there is no CPU fallback)')
    if not (V.device == H.device == W.device):
        raise ValueError(f'target on {V.device}, H on {H.device}, W on {W.device}: they must share one device')


def _v_layout(V: Tensor):
    """(contiguous fp32 V, v_batch_stride in floats, ld)"""
    Vc = V.detach().contiguous()
    return Vc, (0 if Vc.dim() == 2 else Vc.shape[1] * Vc.shape[2]), Vc.shape[-1]


def _v_terms(Vc: Tensor, vstride: int, batch: int, beta: float, weights: Optional[_Weights] = None) -> Tensor:
    """float64 ``[batch]`` on the device: the terms of ``metrics.beta_div`` that hold v alone (metrics.py:22, 39, 57, 85-96), per
    problem -- what ``nmfmu_bmu_loss`` takes as ``v_term``.  One ``nmfmu_bmu_v_term`` launch, a workgroup per problem summing
    in a fixed order, so a problem's term does not depend on the batch around it; a shared target is summed once."""
    lib = _capi.load()
    N, Cc = Vc.shape[-2:]
    if weights is not None:
        # ``nmfmu_bwmu_v_term``: a function of the problem's own (V_b, M_b); a shared target is summed once per distinct
        # weight matrix and handed to the problems that use it
        M, mstride, index = weights
        shared = vstride == 0 and (mstride == 0 or index is not None)
        k = (1 if mstride == 0 else M.shape[0]) if shared else batch
        out = torch.empty(k, dtype=torch.float64, device=Vc.device)
        _capi.check(lib.nmfmu_bwmu_v_term(Vc.data_ptr(), vstride, _ptr(M), mstride, None if shared else _ptr(index), Cc,
                                          k, N, Cc, beta, out.data_ptr(), _stream()), 'nmfmu_bwmu_v_term')
        if not shared:
            return out
        return out.expand(batch).contiguous() if mstride == 0 else out[index.long()].contiguous()
    k = 1 if vstride == 0 else batch
    out = torch.empty(k, dtype=torch.float64, device=Vc.device)
    _capi.check(lib.nmfmu_bmu_v_term(Vc.data_ptr(), vstride, Cc, k, N, Cc, beta, out.data_ptr(), _stream()), 'nmfmu_bmu_v_term')
    return out if k == batch else out.expand(batch).contiguous()


def _bmu_call(Vc: Tensor, vstride: int, side: str, owner: Tensor, panel: Tensor, beta: float, step=None, nsplit: int = 0,
              active: Optional[Tensor] = None, _fill=None, _ws=None, weights: Optional[_Weights] = None,
              reg: Optional[Tensor] = None):
    """``nmfmu_bmu_terms`` (``step`` None: returns (num, den), fp32 ``[batch, owner rows, r_pad]``) or ``nmfmu_bmu_step``
    (``step`` = (l1, l2, gamma): ``owner`` updated in place) for every problem whose ``active`` flag is set (None: all).
    ``owner`` / ``panel``: contiguous fp32 ``[batch, rows, R]``.  Enqueued only.  ``_fill``: tests pre-fill the outputs and the
    workspace with it.

    ``weights`` (``_check_weights``) and / or ``reg`` (fp32 ``[batch, 2]`` on the device: every problem's own (l1, l2), replacing
    those of ``step``) go through ``nmfmu_bwmu_terms`` / ``nmfmu_bwmu_step``; without either the call is what it always was."""
    lib = _capi.load()
    N, Cc = Vc.shape[-2:]
    B, rows, R = owner.shape
    w_side = side == 'w'
    assert rows == (Cc if w_side else N) and tuple(panel.shape) == (B, (N if w_side else Cc), R)
    assert owner.is_contiguous() and panel.is_contiguous() and (active is None or active.dtype == torch.int32)
    r_pad = lib.nmfmu_pad_rank(R)
    n_float = lib.nmfmu_bmu_ws(B, rows, N if w_side else Cc, r_pad, nsplit)
    ws = _ws if _ws is not None else torch.empty(max(n_float, 1), dtype=torch.float32, device=Vc.device)
    assert ws.numel() >= n_float
    if _fill is not None:
        ws.fill_(_fill)
    tail = (Cc, B, N, Cc, int(w_side), owner.data_ptr(), panel.data_ptr(), R, r_pad, beta)
    head = (Vc.data_ptr(), vstride) + tail
    weighted = weights is not None or reg is not None
    if weighted:
        M, mstride, index = weights if weights is not None else (None, 0, None)
        assert reg is None or (reg.dtype == torch.float32 and tuple(reg.shape) == (B, 2) and reg.is_contiguous())
        whead = (Vc.data_ptr(), vstride, _ptr(M), mstride, _ptr(index)) + tail
    if step is not None:
        l1, l2, gamma = step
        if weighted:
            _capi.check(lib.nmfmu_bwmu_step(*whead, l1, l2, _ptr(reg), gamma, nsplit, _ptr(active), ws.data_ptr(), _stream()),
                        'nmfmu_bwmu_step')
            return None
        _capi.check(lib.nmfmu_bmu_step(*head, l1, l2, gamma, nsplit, _ptr(active), ws.data_ptr(), _stream()),
                    'nmfmu_bmu_step')
        return None
    num = torch.empty(B, rows, r_pad, dtype=torch.float32, device=Vc.device)
    den = torch.empty(B, rows, r_pad, dtype=torch.float32, device=Vc.device)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    if weighted:
        _capi.check(lib.nmfmu_bwmu_terms(*whead, nsplit, _ptr(active), ws.data_ptr(), num.data_ptr(), den.data_ptr(),
                                         _stream()), 'nmfmu_bwmu_terms')
        return num, den
    _capi.check(lib.nmfmu_bmu_terms(*head, nsplit, _ptr(active), ws.data_ptr(), num.data_ptr(), den.data_ptr(), _stream()),
                'nmfmu_bmu_terms')
    return num, den


def _bmu_loss(H: Tensor, W: Tensor, Vc: Tensor, vstride: int, beta: float, v_term: Tensor, active: Optional[Tensor] = None,
              part: Optional[Tensor] = None, out: Optional[Tensor] = None, weights: Optional[_Weights] = None) -> Tensor:
    """The per-problem divergences as a float64 ``[batch]`` device tensor (``out`` of an inactive problem is left as it was);
    with ``weights`` the weighted ones (``nmfmu_bwmu_loss``).  Enqueued only."""
    lib = _capi.load()
    B, N, R = H.shape
    Cc = W.shape[1]
    if part is None:
        part = torch.empty(B * lib.nmfmu_bmu_loss_parts(N, Cc), dtype=torch.float64, device=H.device)
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=H.device)
    if weights is not None:
        M, mstride, index = weights
        _capi.check(lib.nmfmu_bwmu_loss(Vc.data_ptr(), vstride, _ptr(M), mstride, _ptr(index), Cc, B, N, Cc, H.data_ptr(),
                                        W.data_ptr(), R, beta, v_term.data_ptr(), _ptr(active), part.data_ptr(),
                                        out.data_ptr(), _stream()), 'nmfmu_bwmu_loss')
        return out
    _capi.check(lib.nmfmu_bmu_loss(Vc.data_ptr(), vstride, Cc, B, N, Cc, H.data_ptr(), W.data_ptr(), R, beta,
                                   v_term.data_ptr(), _ptr(active), part.data_ptr(), out.data_ptr(), _stream()),
                'nmfmu_bmu_loss')
    return out


def _target_flags(Vc: Tensor, beta: float, weights: Optional[_Weights] = None) -> None:
    """nmf.py:329-336 for the whole batch from ONE device pass (the minimum; a NaN anywhere makes it NaN).  With ``weights``
    the pass runs over the entries that carry a positive weight in at least one problem that uses them (``WeightedTarget``'s
    rule): weight 0 hides whatever ``V`` holds."""
    if weights is not None:
        M, _, index = weights
        sel = M > 0
        if index is not None:
            sel = sel[index.long().unique()].any(0) if Vc.dim() == 2 else sel[index.long()]
        elif Vc.dim() == 2 and sel.dim() == 3:
            sel = sel.any(0)
        vs = Vc[:, sel] if sel.dim() < Vc.dim() else Vc[sel]
        if not vs.numel():
            return
        assert not bool((~(vs >= 0)).any()), 'Target should be non-negative.'
        v_min = float(vs.min())
    else:
        v_min = float(Vc.min()) if Vc.numel() else 0.0
    assert v_min >= 0, 'Target should be non-negative.'
    if v_min == 0 and beta <= 0:
        raise ValueError('When beta <= 0 and V contains zeros, the training process may diverge. '
                         'Please add small values to V, or use a positive beta value.')


def batched_beta_div(H: Tensor, W: Tensor, V: Tensor, beta: float = 2, weights=None, weight_index=None) -> Tensor:
    """``metrics.beta_div(H_b @ W_b.T, V_b, beta)`` for every problem of a batch, without the ``B`` reconstructions in HBM.

    ``H`` is (B, N, R), ``W`` (B, C, R), fp32, rank <= 256; ``V`` a dense fp32 (B, N, C) tensor, or (N, C): one target shared by
    all problems.  Every beta; beta <= 0 needs a strictly positive target.  Returns a float64 ``[B]`` device tensor (the value
    only: not differentiable -- the gradients are ``den - num`` of ``nmfmu_bmu_terms``).

    ``weights`` / ``weight_index`` as in ``BatchedNMF.fit``: the weighted divergences ``sum_ij m_ij d_beta(v_ij | y_ij)``; an
    entry of weight 0 counts for nothing whatever ``V`` holds there."""
    beta = float(beta)
    assert H.dim() == 3 and W.dim() == 3 and H.shape[0] == W.shape[0] and H.shape[2] == W.shape[2], \
        'H must be (B, N, R) and W (B, C, R)'
    _check_target(V, H, W, device=False)
    wt = _check_weights(V, weights, weight_index, H.shape[0])
    _check_device(V, H, W)
    Vc, vstride, _ = _v_layout(V)
    _target_flags(Vc, beta, wt)
    return _bmu_loss(H.detach().contiguous(), W.detach().contiguous(), Vc, vstride, beta,
                     _v_terms(Vc, vstride, H.shape[0], beta, wt), weights=wt)


class BatchedNMF(nn.Module):
    """``B`` independent factorisations ``V_b (N, C) ~ H_b (N, R) @ W_b (C, R)^T`` fitted together.

        m = BatchedNMF((B, N, C), rank=R).cuda()       # H [B, N, R], W [B, C, R] drawn from |N(0, 1)| like NMF
        n_iter = m.fit(V, beta=1)                      # V [B, N, C], or [N, C]: one target, B restarts
        best = m.best(V, beta=1); model = m.problem(best)

    ``W`` / ``H`` may be given as non-negative (B, rows, R) tensors; ``trainable_W`` / ``trainable_H`` freeze a factor of every
    problem.  Dense fp32 targets, ``solver='mu'`` arithmetic in exact fp32 (``last_precision`` is 'fp32'), rank <= 256, not
    sharded.  ``fit(V, weights=M)`` fits every problem under dense weights or a mask, and ``alpha`` / ``l1_ratio`` may be given
    per problem (``model_selection.cross_validate`` sweeps rank and ``alpha`` that way).

    When to prefer it over a loop of ``NMF.fit``: when one problem cannot fill the device.  Measured on an MI355X per
    100-iteration fit: 0.057 ms at 512 targets of 513 x 128, rank 16, and 0.007 ms at 4096 targets of
    64 x 64, rank 8, against 2.9 - 5.3 ms per fit in a loop (56 - 470x faster: a loop pays about 30 us of launches per
    iteration however small the problem).  At 32 restarts of a 5168 x 1025 target, rank 88, one problem fills the device and the
    loop of ``NMF.fit`` is 1.5 - 2.2x FASTER (6.7 - 8.2 against 13.8 - 14.5 ms per fit: its split-bf16 kernels against exact
    fp32 here) -- prefer the loop there.  The crossover between was not measured; the two rates put it near
    ``N * C * R = 1e8``."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, W=None, H=None, trainable_W: bool = True,
                 trainable_H: bool = True):
        super().__init__()
        if isinstance(Vshape, Iterable):
            batch, n_rows, n_cols = Vshape
            rank = rank if rank else n_cols
            W = (batch, n_cols, rank) if W is None else W
            H = (batch, n_rows, rank) if H is None else H
        w_param, w_br = _new_batched_factor(W, trainable_W, 'W')
        h_param, h_br = _new_batched_factor(H, trainable_H, 'H')
        assert w_param is not None and h_param is not None, 'BatchedNMF needs a shape (B, N, C) with a rank, or W and H'
        assert w_br == h_br, f'W {tuple(w_param.shape)} and H {tuple(h_param.shape)} must share batch and rank'
        self.register_parameter('W', w_param)
        self.register_parameter('H', h_param)
        self.batch, self.rank = h_br
        self.last_precision = None
        self.last_loss = None

    def extra_repr(self) -> str:
        return f'batch={self.batch}, rank={self.rank}, rows={self.H.shape[1]}, out_channels={self.W.shape[1]}'

    def forward(self) -> Tensor:
        """The ``[B, N, C]`` reconstructions."""
        return torch.bmm(self.H, self.W.transpose(1, 2))

    @torch.no_grad()
    def loss(self, V: Tensor, beta: float = 1, weights=None, weight_index=None) -> Tensor:
        """float64 ``[B]`` on the device: ``metrics.beta_div`` per problem (``batched_beta_div``), weighted with ``weights``."""
        return batched_beta_div(self.H.data, self.W.data, V, beta, weights, weight_index)

    @torch.no_grad()
    def best(self, V: Tensor, beta: float = 1, weights=None, weight_index=None) -> int:
        """The index of the problem with the smallest (weighted) loss (a NaN loss never wins)."""
        loss = self.loss(V, beta, weights, weight_index)
        return int(torch.where(torch.isnan(loss), torch.full_like(loss, float('inf')), loss).argmin())

    def problem(self, b: int):
        """An ``NMF`` holding copies of problem ``b``'s factors (on their device, with this module's trainable flags)."""
        from .nmf import NMF
        m = NMF(W=self.W.data[b].cpu(), H=self.H.data[b].cpu(), trainable_W=self.W.requires_grad,
                trainable_H=self.H.requires_grad)
        return m.to(self.H.device)

    @torch.no_grad()
    def fit(self, V: Tensor, beta: float = 1, tol: float = 1e-4, max_iter: int = 200, alpha=0, l1_ratio=0, *,
            nsplit: int = 0, weights=None, weight_index=None) -> Tensor:
        """The contract of ``NMF.fit`` (reference nmf.py:297-409) applied to every problem independently: a W half-step, then
        an H half-step with the new W; at every 10th iteration ``loss = sqrt(2 * beta_div)``, and a problem stops once
        ``(previous - loss) / loss_init < tol`` (a negative divergence gives NaN and never stops).  A stopped problem's
        factors are frozen at its stop iteration while the others go on.  ``alpha`` / ``l1_ratio`` penalise as in ``NMF.fit``.

        ``V``: dense fp32 ``[B, N, C]``, or ``[N, C]`` -- one target shared by all ``B`` problems (restarts).  Returns a
        ``torch.int64`` tensor ``[B]`` on the CPU with every problem's iteration count (``max_iter`` for one that never
        stopped); ``self.last_loss`` holds the float64 ``[B]`` divergences of the final factors on the device.

        ``nsplit`` (0: the library's rule, a function of the shape alone) forces the number of parts of the contraction.

        ``weights``: dense per-entry weights or a mask, bool, integer or floating, finite and >= 0 -- ``(N, C)`` shared by every
        problem, ``(B, N, C)``, or ``(G, N, C)`` with ``weight_index`` (an integer tensor ``[B]`` with values in ``[0, G)``:
        problem ``b`` reads ``weights[weight_index[b]]``).  Problem ``b`` is then ``NMF.fit(V_b, weights=M_b)`` bit for bit:
        both seeds of the update are multiplied by ``m``, an entry of weight 0 is left out whatever ``V`` holds there (NaN
        marks missing data), and the tracked loss, the stop rule and ``last_loss`` are the weighted loss.  A problem whose
        weights are all 0 has loss 0, never stops and, with ``alpha = 0``, keeps its factors.  ``alpha`` and ``l1_ratio`` each
        take a float or one value per problem (a length-``B`` sequence or tensor)."""
        W, H = self.W, self.H
        _check_target(V, H, W, device=False)
        wt = _check_weights(V, weights, weight_index, H.shape[0])
        l1, l2, reg_vec = _check_reg(alpha, l1_ratio, H.shape[0])
        _check_device(V, H, W)
        max_iter = int(max_iter)
        if max_iter < 0 or nsplit < 0:
            raise ValueError(f'max_iter and nsplit must be >= 0, got {max_iter} and {nsplit}')
        beta = float(beta)
        lib, dev = _capi.load(), H.device
        Vc, vstride, _ = _v_layout(V)
        if not (W.data.is_contiguous() and H.data.is_contiguous()):
            W.data, H.data = W.data.contiguous(), H.data.contiguous()
        Wd, Hd = W.data, H.data
        B, N, R = Hd.shape
        Cc = Wd.shape[1]
        self.last_precision = 'fp32'
        _target_flags(Vc, beta, wt)
        if reg_vec is not None:
            reg_vec = reg_vec.float().contiguous().to(dev)
        kw = {} if wt is None and reg_vec is None else dict(weights=wt, reg=reg_vec)      # none: the calls of always
        lkw = {} if wt is None else dict(weights=wt)

        r_pad = lib.nmfmu_pad_rank(R)
        ws = torch.empty(max(1, lib.nmfmu_bmu_ws(B, N, Cc, r_pad, nsplit), lib.nmfmu_bmu_ws(B, Cc, N, r_pad, nsplit)),
                         dtype=torch.float32, device=dev)
        part = torch.empty(B * lib.nmfmu_bmu_loss_parts(N, Cc), dtype=torch.float64, device=dev)
        div = torch.empty(B, dtype=torch.float64, device=dev)
        v_term = _v_terms(Vc, vstride, B, beta, wt)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        n_iter = torch.full((B,), max_iter, dtype=torch.int64, device=dev)
        n_active = torch.full((1,), B, dtype=torch.int32, device=dev)
        arrived = torch.empty(1, dtype=torch.int32).pin_memory()
        reg = (l1, l2, mu_gamma(beta))

        _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, None, part, div, **lkw)
        loss_init = (2.0 * div).sqrt()                  # nmf.py:355-363; NaN for a negative divergence, like nmf._sqrt2
        previous = loss_init.clone()
        pending = None                                  # the event behind the last checkpoint's copy of n_active
        for it in range(max_iter):
            if W.requires_grad:
                _bmu_call(Vc, vstride, 'w', Wd, Hd, beta, step=reg, nsplit=nsplit, active=active, _ws=ws, **kw)
            if H.requires_grad:
                _bmu_call(Vc, vstride, 'h', Hd, Wd, beta, step=reg, nsplit=nsplit, active=active, _ws=ws, **kw)
            if it % 10 == 9:
                # the previous checkpoint's count arrived long ago: no problem left means nothing below changes a bit
                if pending is not None:
                    pending.synchronize()
                    if int(arrived[0]) == 0:
                        break
                _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, active, part, div, **lkw)
                _capi.check(lib.nmfmu_bmu_judge(B, div.data_ptr(), loss_init.data_ptr(), previous.data_ptr(), float(tol), it,
                                                active.data_ptr(), n_iter.data_ptr(), n_active.data_ptr(), _stream()),
                            'nmfmu_bmu_judge')
                arrived.copy_(n_active, non_blocking=True)
                pending = torch.cuda.Event()
                pending.record()
        self.last_loss = _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, None, part, div, **lkw).clone()
        return n_iter.cpu()
