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
"""
from __future__ import annotations

from collections.abc import Iterable
from typing import Optional

import torch
from torch import Tensor, nn

from . import _capi
from .engine import mu_gamma

__all__ = ['BatchedNMF', 'batched_beta_div', 'MAX_RANK']

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


def _check_target(V, H: Tensor, W: Tensor) -> None:
    """Everything about the target and the factors that can be judged without the device; raises before any launch."""
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


def _v_terms(Vc: Tensor, vstride: int, batch: int, beta: float) -> Tensor:
    """float64 ``[batch]`` on the device: the terms of ``metrics.beta_div`` that hold v alone (metrics.py:22, 39, 57, 85-96), per
    problem -- what ``nmfmu_bmu_loss`` takes as ``v_term``.  One ``nmfmu_bmu_v_term`` launch, a workgroup per problem summing
    in a fixed order, so a problem's term does not depend on the batch around it; a shared target is summed once."""
    lib = _capi.load()
    N, Cc = Vc.shape[-2:]
    k = 1 if vstride == 0 else batch
    out = torch.empty(k, dtype=torch.float64, device=Vc.device)
    _capi.check(lib.nmfmu_bmu_v_term(Vc.data_ptr(), vstride, Cc, k, N, Cc, beta, out.data_ptr(), _stream()), 'nmfmu_bmu_v_term')
    return out if k == batch else out.expand(batch).contiguous()


def _bmu_call(Vc: Tensor, vstride: int, side: str, owner: Tensor, panel: Tensor, beta: float, step=None, nsplit: int = 0,
              active: Optional[Tensor] = None, _fill=None, _ws=None):
    """``nmfmu_bmu_terms`` (``step`` None: returns (num, den), fp32 ``[batch, owner rows, r_pad]``) or ``nmfmu_bmu_step``
    (``step`` = (l1, l2, gamma): ``owner`` updated in place) for every problem whose ``active`` flag is set (None: all).
    ``owner`` / ``panel``: contiguous fp32 ``[batch, rows, R]``.  Enqueued only.  ``_fill``: tests pre-fill the outputs and the
    workspace with it."""
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
    head = (Vc.data_ptr(), vstride, Cc, B, N, Cc, int(w_side), owner.data_ptr(), panel.data_ptr(), R, r_pad, beta)
    if step is not None:
        l1, l2, gamma = step
        _capi.check(lib.nmfmu_bmu_step(*head, l1, l2, gamma, nsplit, _ptr(active), ws.data_ptr(), _stream()),
                    'nmfmu_bmu_step')
        return None
    num = torch.empty(B, rows, r_pad, dtype=torch.float32, device=Vc.device)
    den = torch.empty(B, rows, r_pad, dtype=torch.float32, device=Vc.device)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    _capi.check(lib.nmfmu_bmu_terms(*head, nsplit, _ptr(active), ws.data_ptr(), num.data_ptr(), den.data_ptr(), _stream()),
                'nmfmu_bmu_terms')
    return num, den


def _bmu_loss(H: Tensor, W: Tensor, Vc: Tensor, vstride: int, beta: float, v_term: Tensor, active: Optional[Tensor] = None,
              part: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """The per-problem divergences as a float64 ``[batch]`` device tensor (``out`` of an inactive problem is left as it was).
    Enqueued only."""
    lib = _capi.load()
    B, N, R = H.shape
    Cc = W.shape[1]
    if part is None:
        part = torch.empty(B * lib.nmfmu_bmu_loss_parts(N, Cc), dtype=torch.float64, device=H.device)
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=H.device)
    _capi.check(lib.nmfmu_bmu_loss(Vc.data_ptr(), vstride, Cc, B, N, Cc, H.data_ptr(), W.data_ptr(), R, beta,
                                   v_term.data_ptr(), _ptr(active), part.data_ptr(), out.data_ptr(), _stream()),
                'nmfmu_bmu_loss')
    return out


def _target_flags(Vc: Tensor, beta: float) -> None:
    """nmf.py:329-336 for the whole batch from ONE device pass (the minimum; a NaN anywhere makes it NaN)."""
    v_min = float(Vc.min()) if Vc.numel() else 0.0
    assert v_min >= 0, 'Target should be non-negative.'
    if v_min == 0 and beta <= 0:
        raise ValueError('When beta <= 0 and V contains zeros, the training process may diverge. '
                         'Please add small values to V, or use a positive beta value.')


def batched_beta_div(H: Tensor, W: Tensor, V: Tensor, beta: float = 2) -> Tensor:
    """``metrics.beta_div(H_b @ W_b.T, V_b, beta)`` for every problem of a batch, without the ``B`` reconstructions in HBM.

    ``H`` is (B, N, R), ``W`` (B, C, R), fp32, rank <= 256; ``V`` a dense fp32 (B, N, C) tensor, or (N, C): one target shared by
    all problems.  Every beta; beta <= 0 needs a strictly positive target.  Returns a float64 ``[B]`` device tensor (the value
    only: not differentiable -- the gradients are ``den - num`` of ``nmfmu_bmu_terms``)."""
    beta = float(beta)
    assert H.dim() == 3 and W.dim() == 3 and H.shape[0] == W.shape[0] and H.shape[2] == W.shape[2], \
        'H must be (B, N, R) and W (B, C, R)'
    _check_target(V, H, W)
    Vc, vstride, _ = _v_layout(V)
    _target_flags(Vc, beta)
    return _bmu_loss(H.detach().contiguous(), W.detach().contiguous(), Vc, vstride, beta, _v_terms(Vc, vstride, H.shape[0], beta))


class BatchedNMF(nn.Module):
    """``B`` independent factorisations ``V_b (N, C) ~ H_b (N, R) @ W_b (C, R)^T`` fitted together.

        m = BatchedNMF((B, N, C), rank=R).cuda()       # H [B, N, R], W [B, C, R] drawn from |N(0, 1)| like NMF
        n_iter = m.fit(V, beta=1)                      # V [B, N, C], or [N, C]: one target, B restarts
        best = m.best(V, beta=1); model = m.problem(best)

    ``W`` / ``H`` may be given as non-negative (B, rows, R) tensors; ``trainable_W`` / ``trainable_H`` freeze a factor of every
    problem.  Dense fp32 targets, ``solver='mu'`` arithmetic in exact fp32 (``last_precision`` is 'fp32'), rank <= 256, no
    weights, not sharded.

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
    def loss(self, V: Tensor, beta: float = 1) -> Tensor:
        """float64 ``[B]`` on the device: ``metrics.beta_div`` per problem (``batched_beta_div``)."""
        return batched_beta_div(self.H.data, self.W.data, V, beta)

    @torch.no_grad()
    def best(self, V: Tensor, beta: float = 1) -> int:
        """The index of the problem with the smallest loss (a NaN loss never wins)."""
        loss = self.loss(V, beta)
        return int(torch.where(torch.isnan(loss), torch.full_like(loss, float('inf')), loss).argmin())

    def problem(self, b: int):
        """An ``NMF`` holding copies of problem ``b``'s factors (on their device, with this module's trainable flags)."""
        from .nmf import NMF
        m = NMF(W=self.W.data[b].cpu(), H=self.H.data[b].cpu(), trainable_W=self.W.requires_grad,
                trainable_H=self.H.requires_grad)
        return m.to(self.H.device)

    @torch.no_grad()
    def fit(self, V: Tensor, beta: float = 1, tol: float = 1e-4, max_iter: int = 200, alpha: float = 0,
            l1_ratio: float = 0, *, nsplit: int = 0) -> Tensor:
        """The contract of ``NMF.fit`` (reference nmf.py:297-409) applied to every problem independently: a W half-step, then
        an H half-step with the new W; at every 10th iteration ``loss = sqrt(2 * beta_div)``, and a problem stops once
        ``(previous - loss) / loss_init < tol`` (a negative divergence gives NaN and never stops).  A stopped problem's
        factors are frozen at its stop iteration while the others go on.  ``alpha`` / ``l1_ratio`` penalise as in ``NMF.fit``.

        ``V``: dense fp32 ``[B, N, C]``, or ``[N, C]`` -- one target shared by all ``B`` problems (restarts).  Returns a
        ``torch.int64`` tensor ``[B]`` on the CPU with every problem's iteration count (``max_iter`` for one that never
        stopped); ``self.last_loss`` holds the float64 ``[B]`` divergences of the final factors on the device.

        ``nsplit`` (0: the library's rule, a function of the shape alone) forces the number of parts of the contraction."""
        W, H = self.W, self.H
        _check_target(V, H, W)
        max_iter = int(max_iter)
        if max_iter < 0 or nsplit < 0:
            raise ValueError(f'max_iter and nsplit must be >= 0, got {max_iter} and {nsplit}')
        beta = float(beta)
        l1 = float(alpha * l1_ratio)        # nmf.py:348-349
        l2 = float(alpha * (1 - l1_ratio))
        lib, dev = _capi.load(), H.device
        Vc, vstride, _ = _v_layout(V)
        if not (W.data.is_contiguous() and H.data.is_contiguous()):
            W.data, H.data = W.data.contiguous(), H.data.contiguous()
        Wd, Hd = W.data, H.data
        B, N, R = Hd.shape
        Cc = Wd.shape[1]
        self.last_precision = 'fp32'
        _target_flags(Vc, beta)

        r_pad = lib.nmfmu_pad_rank(R)
        ws = torch.empty(max(1, lib.nmfmu_bmu_ws(B, N, Cc, r_pad, nsplit), lib.nmfmu_bmu_ws(B, Cc, N, r_pad, nsplit)),
                         dtype=torch.float32, device=dev)
        part = torch.empty(B * lib.nmfmu_bmu_loss_parts(N, Cc), dtype=torch.float64, device=dev)
        div = torch.empty(B, dtype=torch.float64, device=dev)
        v_term = _v_terms(Vc, vstride, B, beta)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        n_iter = torch.full((B,), max_iter, dtype=torch.int64, device=dev)
        n_active = torch.full((1,), B, dtype=torch.int32, device=dev)
        arrived = torch.empty(1, dtype=torch.int32).pin_memory()
        reg = (l1, l2, mu_gamma(beta))

        _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, None, part, div)
        loss_init = (2.0 * div).sqrt()                  # nmf.py:355-363; NaN for a negative divergence, like nmf._sqrt2
        previous = loss_init.clone()
        pending = None                                  # the event behind the last checkpoint's copy of n_active
        for it in range(max_iter):
            if W.requires_grad:
                _bmu_call(Vc, vstride, 'w', Wd, Hd, beta, step=reg, nsplit=nsplit, active=active, _ws=ws)
            if H.requires_grad:
                _bmu_call(Vc, vstride, 'h', Hd, Wd, beta, step=reg, nsplit=nsplit, active=active, _ws=ws)
            if it % 10 == 9:
                # the previous checkpoint's count arrived long ago: no problem left means nothing below changes a bit
                if pending is not None:
                    pending.synchronize()
                    if int(arrived[0]) == 0:
                        break
                _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, active, part, div)
                _capi.check(lib.nmfmu_bmu_judge(B, div.data_ptr(), loss_init.data_ptr(), previous.data_ptr(), float(tol), it,
                                                active.data_ptr(), n_iter.data_ptr(), n_active.data_ptr(), _stream()),
                            'nmfmu_bmu_judge')
                arrived.copy_(n_active, non_blocking=True)
                pending = torch.cuda.Event()
                pending.record()
        self.last_loss = _bmu_loss(Hd, Wd, Vc, vstride, beta, v_term, None, part, div).clone()
        return n_iter.cpu()
