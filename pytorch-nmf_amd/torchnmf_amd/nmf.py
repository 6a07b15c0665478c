"""``torchnmf.nmf``-compatible module surface over the MI355X MU engine.

Mirrors the public behaviour of the reference's ``BaseComponent`` / ``NMF`` /
``NMFD`` (torchnmf/nmf.py:173-409, 641-779): same constructor arguments,
attributes (``W``, ``H``, ``rank``, ``out_channels``, ``kernel_size``),
``forward`` / ``reconstruct`` / ``fit`` signatures, return values and error
types.  What differs is *where* the arithmetic happens: every compute entry
point runs hand-written HIP kernels on the module's ROCm device through the C
ABI of ``include/nmfmu.h``; there is no CPU path (a CPU-resident module raises
on ``forward`` / ``fit``).

``NMF2D`` / ``NMF3D`` (nmf.py:782-942) and sparse-COO targets of ``NMF.fit`` (nmf.py:351-398, 602-638) run on
the same engines.  ``NMF.forward`` / ``NMF.reconstruct`` are differentiable (``torch.autograd`` through an exact-fp32
MFMA backward, ``nmfmu_reconstruct_backward``): ``beta_div(m(), V, beta).backward()`` and any ``torch.optim`` optimizer
work as in the reference.  The convolutive ``forward`` (``NMFD`` / ``NMF2D`` / ``NMF3D``) is differentiable the same way
(``nmfmu_conv_backward``).  ``sparse_fit`` (Hoyer's sparseness-constrained fitting, nmf.py:411-599) runs on those backward
kernels, the MU engines and one batched projection kernel (``hoyer.hoyer_project`` / ``nmfmu_hoyer_project``) for dense targets
on all four model classes; sparse-COO targets of ``sparse_fit`` are not implemented.
"""
from __future__ import annotations

import numbers
import os
from collections.abc import Iterable
from typing import Optional

import torch
from torch import Tensor, nn

from . import _capi
from .constants import eps  # noqa: F401  (re-exported like the reference)

__all__ = ['BaseComponent', 'NMF', 'NMFD', 'NMF2D', 'NMF3D']      # torchnmf/nmf.py:16-18


def _sqrt2(div: float) -> float:
    """``sqrt(2 * divergence)`` of nmf.py:362 / 402.  A divergence that fp32 rounding pushed slightly below zero gives
    NaN, as ``Tensor.sqrt`` does in the reference (a Python float power would return a complex number and make the
    ``< tol`` comparison raise)."""
    d = 2.0 * div
    return d ** 0.5 if d >= 0 else float('nan')


def _new_factor(spec, trainable: bool, label: str):
    """Turn a constructor argument into (Parameter | None, inferred rank | None) -- nmf.py:213-237."""
    if isinstance(spec, Tensor):
        assert bool(torch.all(spec >= 0.)), f"Tensor {label} should be non-negative."
        p = nn.Parameter(torch.empty(*spec.size()), requires_grad=trainable)
        p.data.copy_(spec)
        return p, p.shape[1]
    if isinstance(spec, Iterable):
        shape = tuple(spec)
        # like the reference, a shape always yields a trainable factor drawn from |N(0, 1)|
        return nn.Parameter(torch.randn(*shape).abs()), shape[1]
    return None, None


def _require_device(t: Tensor, what: str) -> None:
    if t.device.type != 'cuda':
        raise _capi.NmfmuError(f'{what}: tensors live on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                               f'the module and its inputs with .cuda() (there is no CPU fallback)')


def _reconstruct_forward(H: Tensor, W: Tensor) -> Tensor:
    lib = _capi.load()
    lead = tuple(H.shape[:-1])                       # F.linear accepts leading batch dimensions (nmf.py:693)
    Hc = H.detach().float().reshape(-1, H.shape[-1]).contiguous()
    Wc = W.detach().float().contiguous()
    out = torch.empty(Hc.shape[0], Wc.shape[0], dtype=torch.float32, device=H.device)
    _capi.check(lib.nmfmu_reconstruct(Hc.data_ptr(), Hc.shape[0], Wc.data_ptr(), Wc.shape[0], Hc.shape[1],
                                      out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream),
                'nmfmu_reconstruct')
    out = out.reshape(lead + (Wc.shape[0],))
    return out if H.dtype == torch.float32 else out.to(H.dtype)      # (a module cast to another dtype answers in it)


def reconstruct_backward_splits(m: int, k: int, rank: int):
    """(parts of grad_owner's contraction, parts of grad_panel's) for an ``m x k`` incoming gradient: the split rule of
    ``nmfmu_reconstruct_backward`` (include/nmfmu.h), a pure function of the shape."""
    import ctypes
    splits = (ctypes.c_int * 2)()
    _capi.load().nmfmu_reconstruct_backward_ws(m, k, rank, 1, 1, splits)
    return splits[0], splits[1]


def _reconstruct_backward(G: Tensor, H: Tensor, W: Tensor, need_h: bool, need_w: bool):
    """(grad_H | None, grad_W | None) of ``out = H @ W.T`` given ``G = d loss / d out``, in the inputs' shapes and dtypes.
    ``G`` is read in place through its row stride; only a last stride other than 1 costs a copy."""
    lib = _capi.load()
    R, C = H.shape[-1], W.shape[0]
    Hc = H.detach().float().reshape(-1, R).contiguous()
    Wc = W.detach().float().contiguous()
    N = Hc.shape[0]                                  # leading dimensions of H flattened: grad_W sums over all of them
    G2 = G.detach().float().reshape(N, C)
    if G2.stride(1) != 1 or (N > 1 and G2.stride(0) < C):
        G2 = G2.contiguous()
    ld = G2.stride(0) if N > 1 else C
    gH = torch.empty(N, R, dtype=torch.float32, device=G2.device) if need_h else None
    gW = torch.empty(C, R, dtype=torch.float32, device=G2.device) if need_w else None
    n_ws = lib.nmfmu_reconstruct_backward_ws(N, C, R, int(need_h), int(need_w), None)
    ws = torch.empty(n_ws, dtype=torch.float32, device=G2.device) if n_ws > 0 else None
    _capi.check(lib.nmfmu_reconstruct_backward(G2.data_ptr(), ld, N, C, Hc.data_ptr(), Wc.data_ptr(), R,
                                               gH.data_ptr() if need_h else None, gW.data_ptr() if need_w else None,
                                               ws.data_ptr() if ws is not None else None,
                                               torch.cuda.current_stream().cuda_stream), 'nmfmu_reconstruct_backward')
    if need_h:
        gH = gH.reshape(H.shape).to(H.dtype)
    if need_w:
        gW = gW.to(W.dtype)
    return gH, gW


class _ReconstructFn(torch.autograd.Function):
    """``NMF.reconstruct`` with a device backward.  The forward is the same ``nmfmu_reconstruct`` launch as without autograd
    (bit-identical output)."""

    @staticmethod
    def forward(ctx, H, W):
        ctx.save_for_backward(H, W)
        return _reconstruct_forward(H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        H, W = ctx.saved_tensors
        return _reconstruct_backward(G, H, W, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def conv_backward_splits(H_shape, W_shape):
    """(parts of grad_H's contraction, parts of grad_W's) for factors of these shapes: the split rule of
    ``nmfmu_conv_backward`` (include/nmfmu.h), a pure function of the shape."""
    import ctypes
    nd = len(H_shape) - 2
    splits = (ctypes.c_int * 2)()
    _capi.load().nmfmu_conv_backward_ws(H_shape[0], W_shape[0], H_shape[1], nd, (ctypes.c_int32 * nd)(*H_shape[2:]),
                                        (ctypes.c_int32 * nd)(*W_shape[2:]), 1, 1, splits)
    return splits[0], splits[1]


def _conv_reconstruct_backward(G: Tensor, H: Tensor, W: Tensor, need_h: bool, need_w: bool):
    """(grad_H | None, grad_W | None) of the convolutive reconstruction given ``G = d loss / d out``, in the inputs' shapes
    and dtypes: one ``nmfmu_conv_backward`` call.  A contiguous fp32 ``G`` is read in place; anything else is copied once."""
    import ctypes
    lib = _capi.load()
    Hc, Wc = H.detach().float().contiguous(), W.detach().float().contiguous()
    Gc = G.detach().float().contiguous()
    nd = Hc.dim() - 2
    B, R, Cc = Hc.shape[0], Hc.shape[1], Wc.shape[0]
    lh, taps = (ctypes.c_int32 * nd)(*Hc.shape[2:]), (ctypes.c_int32 * nd)(*Wc.shape[2:])
    assert tuple(Gc.shape) == (B, Cc) + tuple(a + t - 1 for a, t in zip(Hc.shape[2:], Wc.shape[2:]))
    gH = torch.empty_like(Hc) if need_h else None
    gW = torch.empty_like(Wc) if need_w else None
    n_ws = lib.nmfmu_conv_backward_ws(B, Cc, R, nd, lh, taps, int(need_h), int(need_w), None)
    _capi.check(min(n_ws, 0), 'nmfmu_conv_backward_ws')
    ws = torch.empty(n_ws, dtype=torch.float32, device=Gc.device) if n_ws > 0 else None
    _capi.check(lib.nmfmu_conv_backward(Gc.data_ptr(), Wc.data_ptr(), Hc.data_ptr(), B, Cc, R, nd, lh, taps,
                                        gH.data_ptr() if need_h else None, gW.data_ptr() if need_w else None,
                                        ws.data_ptr() if ws is not None else None,
                                        torch.cuda.current_stream().cuda_stream), 'nmfmu_conv_backward')
    return (gH.to(H.dtype) if need_h else None), (gW.to(W.dtype) if need_w else None)


class _ConvReconstructFn(torch.autograd.Function):
    """``NMFD / NMF2D / NMF3D.reconstruct`` with a device backward.  The forward is ``nmfd_engine.reconstruct`` itself: the
    same launches as without autograd (bit-identical output)."""

    @staticmethod
    def forward(ctx, H, W):
        from .nmfd_engine import reconstruct as _recon
        ctx.save_for_backward(H, W)
        return _recon(H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        H, W = ctx.saved_tensors
        return _conv_reconstruct_backward(G, H, W, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class BaseComponent(nn.Module):
    """Base of the NMF modules (reference: nmf.py:173-292)."""

    def __init__(self, rank: Optional[int] = None, W=None, H=None, trainable_W: bool = True, trainable_H: bool = True):
        super().__init__()
        w_param, w_rank = _new_factor(W, trainable_W, 'W')
        h_param, h_rank = _new_factor(H, trainable_H, 'H')
        self.register_parameter('W', w_param)
        self.register_parameter('H', h_param)
        inferred = h_rank if h_rank is not None else w_rank
        if inferred is None:
            assert rank, "A rank should be given when W and H are not available!"
        else:
            if h_param is not None:
                assert h_param.shape[1] == inferred, "Latent size of H does not match with others!"
            if w_param is not None:
                assert w_param.shape[1] == inferred, "Latent size of W does not match with others!"
                self.out_channels = w_param.shape[0]
                if w_param.ndim > 2:
                    self.kernel_size = tuple(w_param.shape[2:])
            rank = inferred
        self.rank = rank

    def extra_repr(self) -> str:
        parts = [str(self.rank)]
        if self.W is not None:
            parts.append(f'out_channels={self.out_channels}')
            if hasattr(self, 'kernel_size'):
                parts.append(f'kernel_size={self.kernel_size}')
        return ', '.join(parts)

    def forward(self, H: Tensor = None, W: Tensor = None) -> Tensor:
        """Reconstruction with the module's own factors substituted for missing arguments (nmf.py:261-284)."""
        H = self.H if H is None else H
        W = self.W if W is None else W
        assert H is not None
        assert W is not None
        out = self.reconstruct(H, W)
        # provenance for trainer.BetaMu's single-layer path: which layer, and which factors, produced this tensor
        out._nmf_source = (self, H, W)
        return out

    @staticmethod
    def reconstruct(H: Tensor, W: Tensor) -> Tensor:
        raise NotImplementedError

    def separate(self, V: Tensor = None, groups=None, *, power=1.0, select=None) -> Tensor:
        """``separation.separate`` with the module's own factors: ``[S, *target shape]``, the soft mask of every selected
        group of components (``groups``: ``R`` labels, default every component alone), or the mixture ``V`` (real, or the
        ``complex64`` STFT) times it.  Detached; the module is not modified."""
        from .separation import separate
        assert self.H is not None
        assert self.W is not None
        return separate(self.H, self.W, V, groups, power=power, select=select)

    def _make_engine(self, V, beta, l1, l2, precision, group, allreduce=None):
        raise NotImplementedError

    def fit_ard(self, V: Tensor, *args, **kwargs) -> int:
        """ARD-NMF (``NMF.fit_ard``) is not implemented for the convolutive models."""
        raise NotImplementedError(f'fit_ard is implemented for NMF only, not {type(self).__name__}')

    def _projected_half_step(self, p, recon, V, beta: float, l1: float, stepsize: float) -> float:
        """One sparseness-constrained half-step on the factor ``p`` (nmf.py:494-520 / 545-572): the gradient of
        ``beta_div(recon(p), V, beta)`` through the autograd kernels, then up to 10 tries of gradient step, projection of
        every slice along dim 1 (ONE launch; k1 = l1 * norm, k2 = norm^2, formed on the device) and loss, accepting the
        first try whose loss did not grow (the one host sync of a try); the step size halves per rejection and grows by
        1.2 at the end.  The last candidate is stored whether accepted or not, as in the reference."""
        from .hoyer import hoyer_project, slice_norms
        from .metrics import beta_div
        p.grad = None
        with torch.enable_grad():
            loss = beta_div(recon(p), V, beta)
            loss.backward()
        with torch.no_grad():
            grad = p.grad
            for _ in range(10):
                new = p - stepsize * grad
                norms = slice_norms(new, 1)
                hoyer_project(new, l1 * norms, norms * norms, 1, out=new)
                new_loss = beta_div(recon(new), V, beta)
                if new_loss <= loss:
                    break
                stepsize *= 0.5
            stepsize *= 1.2
            p.copy_(new)
        return stepsize

    def sparse_fit(self, V: Tensor, beta: float = 2, max_iter: int = 200, verbose: bool = False,
                   sW: Optional[float] = None, sH: Optional[float] = None) -> int:
        """Minimise the beta-divergence under Hoyer's sparseness constraints (Hoyer 2004; reference nmf.py:411-599).

        ``sW`` / ``sH`` in (0, 1) fix the sparseness of every ``W[:, r]`` / ``H[:, r]``; ``None`` leaves that factor
        unconstrained.  The constrained factors are first projected to unit L2 norm at the target sparseness.  Then, every
        iteration: a half-step on W, a half-step on H, ``H`` renormalised to unit L2 norm per component (W rescaled to
        compensate).  An unconstrained half-step is the multiplicative update of ``fit`` (l1 = l2 = 0) on the MU engine in
        its fp32-grade split-bf16 mode ('bf16x3', fixed: ``fit``'s ``precision`` choice and TORCHNMF_AMD_PRECISION do not apply
        here, the line search compares losses of neighbouring points); a constrained one is a projected gradient step with a halving line search
        (``_projected_half_step``) whose projection is one launch of the batched HIP kernel (``hoyer.hoyer_project``).
        Returns the number of iterations (always ``max_iter``: there is no stopping rule); with ``verbose`` a progress bar
        shows ``sqrt(2 * loss)`` every 10th iteration.

        Dense targets on all four model classes.  Sparse-COO targets raise ``NotImplementedError``: they are deliberately
        left out (the reference's sparse loss path is a second implementation of every step above).  A module in another
        float dtype is fitted on fp32 working copies and keeps its dtype, as in ``fit``.

        There is no CPU path: a module or target that is not on the ROCm device raises ``NotImplementedError`` ("sparse_fit
        has no CPU path") before the library is loaded -- the one place where the missing CPU fallback is not an
        ``NmfmuError`` (this entry point answered ``NotImplementedError`` before it existed, and callers rely on it)."""
        W, H = self.W, self.H
        assert W is not None and H is not None
        for t in (V, W, H):
            if t.device.type != 'cuda':
                raise NotImplementedError(f'sparse_fit has no CPU path: tensors live on {t.device}; torchnmf_amd computes '
                                          f'on an MI355X only -- move the module and its target with .cuda()')
        if V.is_sparse:
            raise NotImplementedError('sparse_fit: sparse-COO targets are not implemented (dense targets only); for a Hoyer-'
                                      'constrained fit on a sparse target drive trainer.SparsityProj with the closure '
                                      'metrics.sparse_beta_div(m.H, m.W, SparseTarget(V), beta) (beta in {1, 2}); otherwise '
                                      'use V.to_dense(), or NMF.fit for the multiplicative update on a sparse target')
        if W.dtype != torch.float32 or H.dtype != torch.float32:
            if not (W.dtype.is_floating_point and H.dtype.is_floating_point):
                raise NotImplementedError(f'factors must be floating point; got W {W.dtype}, H {H.dtype}')
            keep = (W.data, H.data)
            W.grad = H.grad = None
            W.data, H.data = W.data.float().contiguous(), H.data.float().contiguous()
            try:
                return self.sparse_fit(V, beta, max_iter, verbose, sW, sH)
            finally:
                w32, h32 = W.data, H.data
                W.grad = H.grad = None
                W.data, H.data = keep
                W.data.copy_(w32)
                H.data.copy_(h32)
        from .hoyer import hoyer_project, slice_norms
        from .metrics import beta_div
        beta = float(beta)
        V = V.detach()
        if V.dtype != torch.float32:
            V = V.float()
        V = V.contiguous()
        v_min = float(V.min()) if V.numel() else 0.0
        assert v_min >= 0, "Target should be non-negative."          # (NaN fails too, like torch.all(V >= 0))
        if v_min == 0 and beta <= 0:
            raise ValueError("When beta <= 0 and V contains zeros, the training process may diverge. "
                             "Please add small values to V, or use a positive beta value.")
        for q in (W, H):
            if not q.data.is_contiguous():
                q.data = q.data.contiguous()

        def unit_l1(q, s):         # L1 norm of a unit-L2 slice with sparseness s (nmf.py:459-472)
            n = q[:, 0].numel()
            return n ** 0.5 * (1 - s) + s
        l1_w = unit_l1(W, sW) if sW is not None and W.requires_grad else None
        l1_h = unit_l1(H, sH) if sH is not None and H.requires_grad else None
        if l1_w is not None:
            hoyer_project(W.data, l1_w, 1.0, 1, out=W.data)
        if l1_h is not None:
            hoyer_project(H.data, l1_h, 1.0, 1, out=H.data)

        mu_w, mu_h = W.requires_grad and l1_w is None, H.requires_grad and l1_h is None
        eng = None
        if mu_w or mu_h:
            # the fp32-grade mode of the MU engine ('bf16x3'; NMF above rank 128 runs it on the GEMM engine): the line search
            # compares losses of neighbouring points, a single-plane operand mode is not its grade
            with torch.no_grad():
                eng = self._make_engine(V, beta, 0.0, 0.0, 'bf16x3', None)
        stale = False                  # W / H changed behind the engine's back: its operand images must be rebuilt

        def mu_step(which):
            nonlocal stale
            with torch.no_grad():
                if stale:
                    eng.refresh_images()
                    stale = False
                eng.w_step() if which == 'W' else eng.h_step()

        def renorm_h():                # _renorm(W, H, 'H'), nmf.py:139-158
            with torch.no_grad():
                norms = slice_norms(H.data, 1)
                H.data /= norms.view((1, -1) + (1,) * (H.dim() - 2))
                W.data *= norms.view((1, -1) + (1,) * (W.dim() - 2))

        step_w = step_h = 1.0
        pbar = None
        if verbose:
            from tqdm import tqdm
            pbar = tqdm(total=max_iter)
        n_iter = -1
        try:
            for n_iter in range(max_iter):
                if W.requires_grad:
                    if l1_w is None:
                        mu_step('W')
                    else:
                        step_w = self._projected_half_step(W, lambda w: self.reconstruct(H.detach(), w), V, beta, l1_w, step_w)
                        stale = True
                if H.requires_grad:
                    if l1_h is None:
                        mu_step('H')
                    else:
                        step_h = self._projected_half_step(H, lambda h: self.reconstruct(h, W.detach()), V, beta, l1_h, step_h)
                    renorm_h()
                    stale = True
                if pbar is not None and n_iter % 10 == 9:
                    with torch.no_grad():
                        loss = _sqrt2(float(beta_div(self.reconstruct(H, W), V, beta)))
                    pbar.set_postfix(loss=loss)
                    pbar.update(10)
        finally:
            if pbar is not None:
                pbar.close()
        return n_iter + 1

    @torch.no_grad()
    def fit(self, V: Tensor, beta: float = 1, tol: float = 1e-4, max_iter: int = 200, verbose: bool = False,
            alpha: float = 0, l1_ratio: float = 0, *, precision: Optional[str] = None, process_group=None,
            allreduce: Optional[str] = None, unstored: str = 'zero', weights: Optional[Tensor] = None,
            solver: str = 'mu') -> int:
        """Minimise the beta-divergence between ``V`` and the model by multiplicative updates.

        Same contract as the reference (nmf.py:297-409): W half-step, then H
        half-step with the new W, every iteration; every 10th iteration the loss
        ``sqrt(2 * beta_div)`` is evaluated and the loop stops once
        ``(previous - loss) / loss_init < tol``.  Returns the number of iterations.

        Extra keyword-only arguments (not in the reference):
          precision      None / 'auto' (default): the fastest mode that meets the reference's 1e-4 bar.  With both
                         dimensions >= 4096, rank <= 256 and the data inside fp16's range that is a single-plane fp16
                         mode at bf16's MFMA rate: 'f16' (fp16 operands AND target) when V is exactly representable in
                         fp16, else 'f16x' (fp16 operands, V stays fp32 in HBM: nothing is rounded that the reference
                         does not round, twice the V stream).  Otherwise 'bf16x3' (split-bf16 MFMA, 3x the MFMA work,
                         matches the fp32 reference to ~1e-5; above rank 128 on the GEMM engine).  Never plain bf16.
                         Explicit: 'f16' (a V that fp16 does not hold exactly is rounded to 11 significant bits: a few
                         1e-5 per iteration, ~3e-4 after 200), 'f16x', 'bf16x3', 'bf16' (V and operands rounded to
                         bf16: objective within 1e-4, factors ~1e-3).
                         The convolutive models (NMFD / NMF2D / NMF3D): 'f16' for beta == 1 when taps and frames of
                         the last shift axis are multiples of 8, every contraction has >= 1024 terms and the data fit
                         fp16's range; otherwise 'bf16x3'.
                         The environment variable TORCHNMF_AMD_PRECISION overrides the default.  After the call
                         ``self.last_precision`` names the mode that ran.
          process_group  a torch.distributed group: V and W are then this rank's column shard
                         (V[:, Cg], W[Cg]); H is replicated.
          allreduce      sharded fits only: 'single' = ONE all-reduce of the packed [numerator | denominator] buffer per
                         iteration; 'overlap' = the H half-step in two row halves, the first half's all-reduce travelling
                         behind the second half's kernel (two collectives); 'direct' = 'single' with the whole half-step
                         (kernel, slab reduction, RCCL all-reduce, apply) enqueued by ONE C call on the compute stream
                         through the library's own communicator (nmfmu_mu_step_allreduce) instead of torch.distributed;
                         None = TORCHNMF_AMD_AR_OVERLAP / TORCHNMF_AMD_COMM; default 'single' over torch.distributed, the
                         form BASELINE's north_star names (round 5: 'overlap' was the default before, with no N > 1
                         measurement behind it).  'direct' raises when the backend has no communicator entry.
          unstored       sparse targets only: 'zero' (default) counts every unstored entry as an observed zero, like the
                         reference.  'missing' fits the STORED entries only -- ratings, unsampled pairs, masked bins: numerator
                         and denominator of the update and the tracked loss (``beta_div`` over the stored entries) run over
                         the stored set, O(nnz * rank) for every beta; beta <= 0 is admitted when the stored values are
                         strictly positive.  Exact fp32: ``precision`` is ignored and ``last_precision`` is 'fp32'.  A dense
                         target with a mask goes in as ``V.sparse_mask(mask)``.  NMF only, not sharded.
                         A real number omega strictly between 0 and 1 (not a bool; 'zero' stands for 1, 'missing' for 0):
                         implicit feedback -- stored entries carry weight 1 (stored zeros too: explicit negatives), every
                         unstored entry is a zero observed with confidence omega (Hu, Koren, Volinsky 2008).  The loss is
                         ``1/2 sum_stored (v - y)^2 + 1/2 omega sum_unstored y^2``, evaluated without the N x C product.
                         beta == 2 with solver='ccd' only (``wccd.WeightedCcdEngine``), O(nnz R + (N + C) R^2) per
                         iteration; a row or column without a stored entry goes to the floor.  NMF only, rank <= 256, not
                         sharded, exact fp32.
          weights        dense targets only: a tensor of V's shape on V's device -- a mask (bool), counts or exposures
                         (integer) or per-entry confidences such as inverse noise variances (floating), every value finite
                         and >= 0; converted to fp32 once.  The fit minimises ``sum_ij weights_ij * d_beta(V_ij | (H W^T)_ij)``:
                         both seeds of the multiplicative update are multiplied by the weight and the tracked loss is
                         ``metrics.weighted_beta_div``.  An entry of weight 0 counts for nothing WHATEVER V holds there (NaN,
                         Inf, a negative value: mark missing data with NaN); beta <= 0 is admitted when V is strictly
                         positive wherever the weight is.  One fused exact-fp32 MFMA kernel per half-step
                         (``wmu.WeightedMU``), 12 N C rank flop per iteration whatever the weights: ``precision`` is ignored
                         and ``last_precision`` is 'fp32'.  A mask that keeps a small part of V is cheaper as
                         ``fit(V.sparse_mask(mask), unstored='missing')``, whose cost follows the stored entries: measured at
                         4096 x 65536 the weighted kernel is faster once the mask keeps more than about
                         5 % of V at rank 64 and 13 % at rank 128 (3.9x - 9.9x at a density of 0.5).  None (default): the
                         unweighted fit, bit for bit.  NMF only, solver='mu', rank <= 256, not sharded.
          solver         'mu' (default): the multiplicative update.  'hals': cyclic coordinate descent (Cichocki & Phan 2009;
                         sklearn's default solver) for beta == 2 -- the same ``X @ panel`` and Gram matrix as a beta = 2 MU
                         half-step, then one Gauss-Seidel sweep over the rank per row (``hals.hals_sweep``): a few
                         iterations reach the loss MU needs hundreds for.  The factors are first scaled by the scalar that
                         minimises the loss and floored at eps (``hals.HalsEngine``); entries never fall below eps, so an MU
                         fit can continue from the result.  Loss, stop rule and return value as above; alpha / l1_ratio
                         penalise as in the MU denominators.  Dense and sparse-COO (unstored='zero') targets, NMF only,
                         rank <= 256, not sharded.  Exact fp32: ``precision`` is ignored and ``last_precision`` is 'fp32'.
                         'ccd': the same coordinate minimiser for a MISSING-DATA fit (beta == 2, unstored='missing'), where
                         the quadratic of a row is built from its stored entries only and one Gram matrix cannot serve:
                         cyclic coordinate descent with a maintained residual over the stored entries (Yu, Hsieh, Si,
                         Dhillon 2012; ``ccd.ccd_sweep``), O(nnz * rank) per half-step like the masked multiplicative
                         update.  The factors are first scaled by the scalar that minimises the loss over the stored
                         entries and floored at eps (``ccd.CcdEngine``); a row or column without a stored entry is left as
                         it is.  Loss (``beta_div`` over the stored entries), stop rule, return value and alpha / l1_ratio
                         as for 'hals'.  Sparse-COO targets, NMF only, rank <= 256, not sharded, exact fp32.
        """
        if solver not in ('mu', 'hals', 'ccd'):
            raise ValueError(f"solver must be 'mu', 'hals' or 'ccd', got {solver!r}")
        # a real number (not a bool) for `unstored` is the confidence of the unstored zeros; its range is judged below, where
        # the strings are
        weight = float(unstored) if isinstance(unstored, numbers.Real) and not isinstance(unstored, bool) else None
        if weights is not None:
            # judged before anything else touches the target or the device; the scan of the values comes last
            if V.is_sparse:
                raise NotImplementedError("weights: a sparse target is not weighted per entry; its stored set is the mask -- "
                                          "fit(V, unstored='missing') fits the stored entries only")
            if not isinstance(self, NMF):
                raise NotImplementedError(f'weights are implemented for NMF only, not {type(self).__name__}')
            if process_group is not None:
                raise NotImplementedError('weights: a weighted fit is not sharded (process_group must be None)')
            if solver != 'mu':
                raise NotImplementedError(f"weights are fitted by solver='mu' only, not by solver={solver!r}")
            if self.W is not None and self.W.shape[1] > 256:
                raise NotImplementedError(f'weights: rank {self.W.shape[1]} > 256, the limit of the exact-fp32 kernels')
            from .wmu import check_weights
            weights = check_weights(V, weights)
        if solver == 'ccd':
            if float(beta) != 2.0:
                raise NotImplementedError(f"solver='ccd': the coordinate minimiser is closed-form only for beta = 2, got "
                                          f"beta = {beta:g}")
            if not isinstance(self, NMF):
                raise NotImplementedError(f"solver='ccd' is implemented for NMF only, not {type(self).__name__}")
            if weight is None and unstored != 'missing':
                raise NotImplementedError("solver='ccd' fits the stored entries only and needs unstored='missing'; for a "
                                          "target whose unstored entries are observed zeros use solver='hals'")
            if process_group is not None:
                raise NotImplementedError("solver='ccd' is not sharded (process_group must be None)")
            if self.W is not None and self.W.shape[1] > 256:
                raise NotImplementedError(f"solver='ccd': rank {self.W.shape[1]} > 256, the limit of the sparse kernels")
        if solver == 'hals':
            if float(beta) != 2.0:
                raise NotImplementedError(f"solver='hals': the coordinate minimiser is closed-form only for beta = 2, got "
                                          f"beta = {beta:g}")
            if not isinstance(self, NMF):
                raise NotImplementedError(f"solver='hals' is implemented for NMF only, not {type(self).__name__}")
            if unstored == 'missing':
                raise NotImplementedError("solver='hals': the Gram shortcut needs unstored = 'zero' (with unstored='missing' "
                                          "the denominator runs over the stored entries only: use solver='ccd')")
            if process_group is not None:
                raise NotImplementedError("solver='hals' is not sharded (process_group must be None)")
            if self.W is not None and self.W.shape[1] > 256:
                raise NotImplementedError(f"solver='hals': rank {self.W.shape[1]} > 256, the limit of the sparse kernels")
        if (unstored not in ('zero', 'missing')) if weight is None else not 0.0 < weight < 1.0:     # (a NaN fails too)
            raise ValueError(f"unstored must be 'zero' or 'missing', or (solver='ccd') the weight of the unstored zeros, a "
                             f"real number strictly between 0 and 1; got {unstored!r}")
        if weight is not None and solver != 'ccd':
            raise NotImplementedError(f"unstored={unstored!r}: confidence-weighted unstored zeros are fitted by "
                                      f"solver='ccd' only (beta = 2), not by solver={solver!r}")
        if unstored == 'missing':
            if not V.is_sparse:
                raise ValueError("unstored='missing' needs a sparse-COO target whose stored entries are the observed ones; "
                                 "for a dense V with a boolean mask pass V.sparse_mask(mask) (mask: a sparse-COO tensor)")
            if process_group is not None:
                raise NotImplementedError("unstored='missing': sparse targets are not sharded")
        if weight is not None and not V.is_sparse:
            raise ValueError(f"unstored={unstored!r} needs a sparse-COO target: the weight is that of its unstored entries (a "
                             f"dense target stores every entry)")
        sparse = V.is_sparse
        if sparse and not isinstance(self, NMF):
            raise NotImplementedError('sparse targets are supported by NMF only (as in the reference)')
        W, H = self.W, self.H
        assert W is not None and H is not None
        _require_device(V, 'fit')
        _require_device(W, 'fit')
        _require_device(H, 'fit')
        if W.dtype != torch.float32 or H.dtype != torch.float32:
            # The reference runs in whatever dtype the module was cast to (m.double(); nmf.py:216-221).  The engine's masters
            # are fp32: fit on fp32 working copies of the factors and store the result in the module's dtype (round 6;
            # float64 / float16 / bfloat16 modules -- against the reference in float64 the factors agree like the fp32 ones do).
            if not (W.dtype.is_floating_point and H.dtype.is_floating_point):
                raise NotImplementedError(f'factors must be floating point; got W {W.dtype}, H {H.dtype}')
            keep = (W.data, H.data)
            W.data, H.data = W.data.float().contiguous(), H.data.float().contiguous()
            try:
                return self.fit(V, beta, tol, max_iter, verbose, alpha, l1_ratio, precision=precision,
                                process_group=process_group, allreduce=allreduce, unstored=unstored, weights=weights,
                                solver=solver)
            finally:
                w32, h32 = W.data, H.data
                W.data, H.data = keep
                W.data.copy_(w32)
                H.data.copy_(h32)
        if precision is None:
            precision = os.environ.get('TORCHNMF_AMD_PRECISION', 'auto')
        beta = float(beta)
        l1 = float(alpha * l1_ratio)        # nmf.py:348-349
        l2 = float(alpha * (1 - l1_ratio))
        V = V.detach()
        if V.dtype != torch.float32:
            V = V.float()
        if weights is not None:
            from .wmu import WeightedMU
            if not (W.data.is_contiguous() and H.data.is_contiguous()):
                W.data, H.data = W.data.contiguous(), H.data.contiguous()
            eng = WeightedMU(V, weights, W.data, H.data, beta, l1, l2, update_W=W.requires_grad, update_H=H.requires_grad)
        elif solver == 'ccd':
            if not (W.data.is_contiguous() and H.data.is_contiguous()):
                W.data, H.data = W.data.contiguous(), H.data.contiguous()
            if weight is not None:
                from .wccd import WeightedCcdEngine
                eng = WeightedCcdEngine(V, W.data, H.data, weight, l1, l2, update_W=W.requires_grad,
                                        update_H=H.requires_grad)
            else:
                from .ccd import CcdEngine
                eng = CcdEngine(V, W.data, H.data, l1, l2, update_W=W.requires_grad, update_H=H.requires_grad)
        elif solver == 'hals':
            from .hals import HalsEngine
            if not (W.data.is_contiguous() and H.data.is_contiguous()):
                W.data, H.data = W.data.contiguous(), H.data.contiguous()
            eng = HalsEngine(V, W.data, H.data, l1, l2, update_W=W.requires_grad, update_H=H.requires_grad)
        elif sparse:
            if process_group is not None:
                raise NotImplementedError('sparse targets are not sharded')
            from .sparse_engine import MaskedMU, SparseMU
            if unstored == 'missing':
                if not (W.data.is_contiguous() and H.data.is_contiguous()):
                    W.data, H.data = W.data.contiguous(), H.data.contiguous()
                eng = MaskedMU(V, W.data, H.data, beta, l1, l2, update_W=W.requires_grad, update_H=H.requires_grad)
            else:
                eng = SparseMU(V, W.data, H.data, beta, l1, l2, update_W=W.requires_grad, update_H=H.requires_grad)
        else:
            if allreduce not in (None, 'single', 'overlap', 'direct'):
                raise ValueError(f"allreduce must be None, 'single', 'overlap' or 'direct', got {allreduce!r}")
            if allreduce is not None and (process_group is None or not isinstance(self, NMF)):
                # (the choice used to be ignored silently here)
                import warnings
                warnings.warn(f"torchnmf_amd: allreduce={allreduce!r} only applies to a column-sharded NMF.fit "
                              "(process_group=...); ignored", stacklevel=2)
            eng = self._make_engine(V, beta, l1, l2, precision, process_group, allreduce)
        self.last_precision = getattr(eng, 'precision_name', None)   # what 'auto' resolved to (plain attribute, not state)

        has_bad, has_zero = eng.target_flags()   # nmf.py:329-336, computed during packing
        assert not has_bad, "Target should be non-negative."
        if has_zero and beta <= 0:
            raise ValueError("When beta <= 0 and V contains zeros, the training process may diverge. "
                             "Please add small values to V, or use a positive beta value.")

        loss_init = _sqrt2(eng.divergence())   # nmf.py:355-363
        previous = loss_init
        pbar = None
        if verbose:
            from tqdm import tqdm
            pbar = tqdm(total=max_iter)
        n_iter = -1
        warned = False
        # Loss checkpoints without a host sync (engines with AsyncLossMixin; unsharded, no progress bar): the loss of
        # checkpoint k is enqueued -- with a snapshot of W and H -- and judged at checkpoint k + 10, when its value has long
        # arrived; if the stop rule of nmf.py:405 had fired at k, the snapshot is restored and k + 1 returned: the same
        # factors and the same count as the synchronous loop, without draining the launch queue every ten iterations.
        use_async = (process_group is None and not verbose and hasattr(eng, 'checkpoint_begin')
                     and os.environ.get('TORCHNMF_AMD_ASYNC_LOSS', '1') != '0')
        pending = None           # iteration index of the checkpoint whose loss is still in flight

        def range_warning():
            nonlocal warned
            import warnings
            warned = True
            warnings.warn("torchnmf_amd: a factor grew beyond fp16's range (65504) during the fit; its fp16 "
                          "operand image is clamped from here on and the updates no longer follow the "
                          "reference.  Re-run with precision='bf16x3' (or rescale V).")

        def judge(loss, left):
            """nmf.py:402-407 for one checkpoint; True = stop there."""
            nonlocal previous
            if left and not warned:
                range_warning()
            if (previous - loss) / loss_init < tol:
                return True
            previous = loss
            return False

        def settle():
            """Judge the pending checkpoint; on stop restore its factors and return its iteration index, else None."""
            nonlocal pending
            k, pending = pending, None
            div, left = eng.checkpoint_result()
            if judge(_sqrt2(div), left):
                eng.rollback()
                return k
            return None
        try:
            for n_iter in range(max_iter):
                if W.requires_grad:
                    eng.w_step()
                if H.requires_grad:
                    eng.h_step()
                if n_iter % 10 == 9:
                    if use_async:
                        if pending is not None:
                            stopped_at = settle()
                            if stopped_at is not None:
                                n_iter = stopped_at
                                break
                        if n_iter + 1 < max_iter:     # (the last iteration's loss decides nothing: n_iter + 1 is returned either way)
                            eng.checkpoint_begin()
                            pending = n_iter
                        continue
                    loss = _sqrt2(eng.divergence())
                    left = getattr(eng, 'left_f16_range', None) is not None and not warned and eng.left_f16_range()
                    if pbar is not None:
                        pbar.set_postfix(loss=loss)
                        pbar.update(10)
                    if judge(loss, left):
                        break
            if pending is not None:                   # max_iter reached with one checkpoint still unjudged
                stopped_at = settle()
                if stopped_at is not None:
                    n_iter = stopped_at
            # fits shorter than ten iterations never reach a checkpoint: ask once more at the end
            if not warned and getattr(eng, 'left_f16_range', None) is not None and eng.left_f16_range():
                range_warning()
        finally:
            if pbar is not None:
                pbar.close()
        return n_iter + 1


class NMF(BaseComponent):
    """Non-negative matrix factorisation ``V (N, C) ~ H (N, R) @ W (C, R)^T`` (reference: nmf.py:641-697)."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, **kwargs):
        if isinstance(Vshape, Iterable):
            n_rows, n_cols = Vshape
            rank = rank if rank else n_cols
            kwargs['W'] = (n_cols, rank)
            kwargs['H'] = (n_rows, rank)
        super().__init__(rank, **kwargs)

    @staticmethod
    def reconstruct(H: Tensor, W: Tensor) -> Tensor:
        """``H @ W.T`` (nmf.py:691-693) by an exact-fp32 MFMA kernel on the device.

        Differentiable like the reference's ``F.linear``: with grad mode on and ``H`` or ``W`` requiring grad the result
        carries a ``grad_fn`` whose backward is one ``nmfmu_reconstruct_backward`` call (first order only).  Under
        ``torch.no_grad()`` -- ``fit()``, ``BetaMu.step`` -- nothing is recorded."""
        _require_device(H, 'reconstruct')
        _require_device(W, 'reconstruct')
        assert H.dim() >= 2 and W.dim() == 2 and H.shape[-1] == W.shape[1]
        if torch.is_grad_enabled() and (H.requires_grad or W.requires_grad):
            return _ReconstructFn.apply(H, W)
        return _reconstruct_forward(H, W)

    @torch.no_grad()
    def fit_restarts(self, V: Tensor, n_init: int, beta: float = 1, tol: float = 1e-4, max_iter: int = 200,
                     alpha: float = 0, l1_ratio: float = 0, generator: Optional[torch.Generator] = None):
        """``n_init`` fits of the same dense fp32 ``V`` from different starts in one batched run (``batched.BatchedNMF`` on the
        shared target, exact fp32, every start stopped on its own by ``fit``'s rule); the best start's factors are stored.

        The first start is the module's current factors; the others are drawn from ``|N(0, 1)|`` with ``generator`` (on the
        generator's device, the CPU by default), trainable factors only -- a frozen factor is shared by every start.  Returns
        ``(n_iter, losses, best)``: the iteration counts (int64 ``[n_init]``) and final divergences (float64 ``[n_init]``) on
        the CPU and the index of the smallest loss, whose factors the module now holds.  ``fit`` itself is untouched.

        Restarts of a WEIGHTED fit are ``batched.BatchedNMF.fit(V, weights=M)`` on the shared target and the shared weights;
        choosing the rank or ``alpha`` by held-out loss is ``model_selection.cross_validate``."""
        from .batched import BatchedNMF
        n_init = int(n_init)
        if n_init < 1:
            raise ValueError(f'n_init must be >= 1, got {n_init}')
        W, H = self.W, self.H
        assert W is not None and H is not None

        def starts(p):
            first = p.data.detach().float()
            if n_init == 1 or not p.requires_grad:
                return first[None].expand(n_init, *p.shape).contiguous()
            where = generator.device if generator is not None else 'cpu'
            drawn = torch.randn(n_init - 1, *p.shape, generator=generator, device=where).abs()
            return torch.cat([first[None], drawn.to(first.device)])
        bm = BatchedNMF(W=starts(W), H=starts(H), trainable_W=W.requires_grad, trainable_H=H.requires_grad).to(H.device)
        n_iter = bm.fit(V, beta=beta, tol=tol, max_iter=max_iter, alpha=alpha, l1_ratio=l1_ratio)
        losses = bm.last_loss.cpu()
        best = int(torch.where(torch.isnan(losses), torch.full_like(losses, float('inf')), losses).argmin())
        W.data.copy_(bm.W.data[best])
        H.data.copy_(bm.H.data[best])
        self.last_precision = bm.last_precision
        return n_iter, losses, best

    @torch.no_grad()
    def fit_ard(self, V: Tensor, beta: float = 1, prior: str = 'l1', phi: float = 1.0, a: float = 5.0,
                b: Optional[float] = None, tol: float = 1e-5, max_iter: int = 1000, verbose: bool = False, *,
                precision: Optional[str] = None) -> int:
        """Fit with automatic relevance determination (Tan & Fevotte, IEEE TPAMI 2013): start from a generous rank, fit ONCE,
        and let the update shrink the components the data does not need -- the one-fit answer to "which rank?" (the other one
        is ``model_selection.cross_validate``, one batched fit per candidate).

        Model: column ``k`` of ``W`` and column ``k`` of ``H`` share a scale ``lambda_k`` with an inverse-gamma prior
        (shape ``a``, scale ``b``); their entries are exponential (``prior='l1'``) or half-normal (``prior='l2'``) with that
        scale.  The fit minimises ::

            D_beta(V | H W^T) / phi + sum_k [ (f(W[:, k]) + f(H[:, k]) + b) / lambda_k + c log lambda_k ]

        with ``f = ||.||_1``, ``c = N + C + a + 1`` ('l1') or ``f = 1/2 ||.||^2``, ``c = (N + C) / 2 + a + 1`` ('l2'), by the
        multiplicative update of ``fit`` with the per-component penalty ``phi / lambda_k`` in its denominator (``ard.ArdMU``;
        W half-step, H half-step, then ``lambda_k = (f(W[:, k]) + f(H[:, k]) + b) / c``), which never increases it.

        ``phi`` is the DISPERSION of the noise model (the variance for beta = 2; for beta = 1 and 0 the scale of the
        Poisson / gamma noise) and must match the data's scale and noise: it weighs the fit against the prior, and the number
        of components that survive depends on it -- too small and nothing is pruned, too large and real components go too.
        This method does not estimate it.  ``a`` must be > 2 ('l1') or > 1 ('l2'); ``b`` defaults to the moment match
        ``mean(V) = R E[w] E[h]`` (``ard.default_b``).

        Stop rule: every 10th iteration, stop when that iteration's ``max_k |lambda_k - previous lambda_k| / previous
        lambda_k < tol``.  Returns the number of iterations.  Afterwards ``last_relevance`` holds lambda (fp32 ``[R]``),
        ``last_relative_relevance`` holds ``(lambda - B) / B`` with the floor ``B = b / c`` (about 0 for a pruned component)
        and ``last_precision`` names the mode that ran.  No component is removed: see ``effective_rank`` and ``prune``.

        Dense targets, ``NMF`` only, rank <= 256 on the fused kernels (``precision`` as in ``fit``), not sharded.  A frozen
        factor (``requires_grad=False``) is not updated; its norm still enters lambda."""
        from .ard import ArdMU, check_prior, default_b
        if V.is_sparse:
            raise NotImplementedError('fit_ard: sparse targets are not implemented (dense targets only)')
        check_prior(prior, a)
        if not float(phi) > 0:
            raise ValueError(f'phi (the dispersion) must be > 0, got {phi!r}')
        if b is not None and not float(b) > 0:
            raise ValueError(f'b must be > 0, got {b!r}')
        W, H = self.W, self.H
        assert W is not None and H is not None
        R = W.shape[1]
        if R > 256:
            raise NotImplementedError(f'fit_ard: rank {R} > 256, the limit of the fused kernels')
        _require_device(V, 'fit_ard')
        _require_device(W, 'fit_ard')
        _require_device(H, 'fit_ard')
        if W.dtype != torch.float32 or H.dtype != torch.float32:      # fp32 working copies, as in fit
            if not (W.dtype.is_floating_point and H.dtype.is_floating_point):
                raise NotImplementedError(f'factors must be floating point; got W {W.dtype}, H {H.dtype}')
            keep = (W.data, H.data)
            W.data, H.data = W.data.float().contiguous(), H.data.float().contiguous()
            try:
                return self.fit_ard(V, beta, prior, phi, a, b, tol, max_iter, verbose, precision=precision)
            finally:
                w32, h32 = W.data, H.data
                W.data, H.data = keep
                W.data.copy_(w32)
                H.data.copy_(h32)
        if precision is None:
            precision = os.environ.get('TORCHNMF_AMD_PRECISION', 'auto')
        beta = float(beta)
        V = V.detach()
        if V.dtype != torch.float32:
            V = V.float()
        assert V.dim() == 2 and V.shape == (H.shape[0], W.shape[0]), \
            f'V must be {(H.shape[0], W.shape[0])}, got {tuple(V.shape)}'
        for p in (W, H):
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
        if b is None:
            v_mean = float(V.mean(dtype=torch.float64))
            # (a mean that is not positive -- negative entries, NaN, all zeros: the target checks below say what is wrong)
            b = default_b(v_mean, R, float(a), prior) if v_mean > 0 else 1.0
        eng = ArdMU(V, W.data, H.data, beta, prior, phi, a, b, precision, update_W=W.requires_grad,
                    update_H=H.requires_grad)
        self.last_precision = eng.precision_name
        has_bad, has_zero = eng.target_flags()
        assert not has_bad, "Target should be non-negative."
        if has_zero and beta <= 0:
            raise ValueError("When beta <= 0 and V contains zeros, the training process may diverge. "
                             "Please add small values to V, or use a positive beta value.")
        pbar = None
        if verbose:
            from tqdm import tqdm
            pbar = tqdm(total=max_iter)
        n_iter = -1
        try:
            for n_iter in range(max_iter):
                if W.requires_grad:
                    eng.w_step()
                if H.requires_grad:
                    eng.h_step()
                eng.relevance_step()
                if n_iter % 10 == 9:
                    delta = float(eng.delta)          # the loop's one host sync
                    if pbar is not None:
                        pbar.set_postfix(delta=delta)
                        pbar.update(10)
                    if delta < tol:
                        break
            if eng.left_f16_range():
                import warnings
                warnings.warn("torchnmf_amd: a factor grew beyond fp16's range (65504) during the fit; its fp16 operand "
                              "image was clamped and the updates no longer follow the model.  Re-run with "
                              "precision='bf16x3' (or rescale V).")
        finally:
            if pbar is not None:
                pbar.close()
        self.last_relevance = eng.lam.clone()
        self.last_relative_relevance = eng.relative_relevance()
        return n_iter + 1

    def _relative_relevance(self) -> Tensor:
        rel = getattr(self, 'last_relative_relevance', None)
        if rel is None or rel.numel() != self.W.shape[1]:
            raise RuntimeError('no relevance to judge by: call fit_ard first')
        return rel

    def effective_rank(self, rel_tol: float = 1e-2) -> int:
        """Number of components whose relative relevance after ``fit_ard`` exceeds ``rel_tol``."""
        return int((self._relative_relevance() > rel_tol).sum())

    def prune(self, rel_tol: float = 1e-2) -> 'NMF':
        """A new ``NMF`` holding only the components that survived ``fit_ard`` (relative relevance > ``rel_tol``), in their
        original order, on this module's device and in its dtype; this module is not modified."""
        keep = (self._relative_relevance() > rel_tol).nonzero().flatten().to(self.W.device)
        if keep.numel() == 0:
            raise RuntimeError(f'prune: no component has a relative relevance above {rel_tol:g}')
        W, H = self.W.data.index_select(1, keep), self.H.data.index_select(1, keep)
        out = NMF(W=W.float().cpu(), H=H.float().cpu(), trainable_W=self.W.requires_grad, trainable_H=self.H.requires_grad)
        out = out.to(device=self.W.device, dtype=self.W.dtype)
        out.W.data.copy_(W)
        out.H.data.copy_(H)
        return out

    def predict(self, rows: Tensor, cols: Tensor) -> Tensor:
        """The model's value at (row, column) pairs, fp32 ``[n]``, without the ``N x C`` reconstruction
        (``scoring.score_pairs`` on ``H``, ``W``; detached)."""
        from .scoring import score_pairs
        return score_pairs(self.H, self.W, rows, cols)

    def topk(self, k: int, rows: Tensor = None, exclude=None):
        """``(values, indices)`` of the ``k`` best columns of every requested row, the stored positions of ``exclude``
        (typically the sparse training target) left out (``scoring.topk_scores`` on ``H``, ``W``; detached)."""
        from .scoring import topk_scores
        return topk_scores(self.H, self.W, k, rows=rows, exclude=exclude)

    def rank_scores(self, heldout, exclude=None):
        """``Ranks(rows, cols, ranks, scores, admissible)``: the rank of every stored position of ``heldout`` among all
        columns of its row that ``exclude`` (typically the sparse training target) does not store, under ``topk``'s order
        (``scoring.rank_scores`` on ``H``, ``W``; detached)."""
        from .scoring import rank_scores
        return rank_scores(self.H, self.W, heldout, exclude)

    def ranking_metrics(self, heldout, ks=(10,), exclude=None):
        """recall@k / precision@k / ndcg@k for every ``k`` in ``ks``, MRR, AUC and the number of evaluated rows, from the full
        ranking of the held-out pairs (``scoring.ranking_metrics`` on ``H``, ``W``)."""
        from .scoring import ranking_metrics
        return ranking_metrics(self.H, self.W, heldout, ks, exclude)

    def transform(self, V_new, beta: float = 1, max_iter: int = 200, tol: float = 1e-4, alpha: float = 0,
                  l1_ratio: float = 0, *, unstored: str = 'zero', H0: Tensor = None, generator=None,
                  return_n_iter: bool = False):
        """``H_new [n_new, R]`` for rows that were not in the training target -- a 2-D sparse-COO tensor ``(n_new, C)`` or a
        ``metrics.SparseTarget`` -- with ``self.W`` fixed: every row iterated on its own, stopped on its own, all in one
        kernel launch (``fold_in.fold_in``; detached, in the dtype of ``W``).  The module is not modified and ``self.H`` plays
        no part."""
        from .fold_in import fold_in
        assert self.W is not None
        return fold_in(self.W, V_new, beta, max_iter, tol, alpha, l1_ratio, unstored=unstored, H0=H0, generator=generator,
                       return_n_iter=return_n_iter)

    def transform_cd(self, V_new, beta: float = 2, max_iter: int = 200, tol: float = 1e-4, alpha: float = 0,
                     l1_ratio: float = 0, *, unstored='missing', solver: str = 'ccd', H0: Tensor = None, generator=None,
                     return_n_iter: bool = False):
        """``transform`` by coordinate descent for beta = 2 (``fold_in.fold_in_cd``): ``solver='ccd'`` with
        ``unstored='missing'`` or the weight a ``fit(solver='ccd', unstored=omega)`` was trained with, ``solver='hals'`` with
        ``unstored='zero'``; ``H0`` is used without an initial scaling.  The module is not modified and ``self.H`` plays no
        part."""
        from .fold_in import fold_in_cd
        assert self.W is not None
        return fold_in_cd(self.W, V_new, beta, max_iter, tol, alpha, l1_ratio, unstored=unstored, solver=solver, H0=H0,
                          generator=generator, return_n_iter=return_n_iter)

    def _make_engine(self, V, beta, l1, l2, precision, group, allreduce=None):
        from .engine import DenseMU
        assert V.dim() == 2 and V.shape == (self.H.shape[0], self.W.shape[0]), \
            f'V must be {(self.H.shape[0], self.W.shape[0])}, got {tuple(V.shape)}'
        for p in (self.W, self.H):
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
        R = self.W.shape[1]
        # The fused kernels keep rank-wide accumulators in registers: single-plane operands (fp16 / bf16) up to rank 256,
        # the fp32-grade split-bf16 mode up to rank 128.  Everything else runs on the GEMM engine (NMF = the T = 1 member
        # of the NMFD family), which has no rank limit but is not sharded.  'auto' means "meets the 1e-4 parity bar":
        # at rank 129..256 that is the fp16 mode of the fused kernel when DenseMU's size / range test admits it, else
        # (unsharded) the GEMM engine, else (sharded) an error -- never silently the plain bf16 mode.
        auto = precision in (None, 'auto')
        wide = R > 256 or (R > 128 and precision == 'bf16x3')
        if R > 128 and R <= 256 and auto:
            # one admission test for both engines (DenseMU.auto_mode; sharded: its answer is all-reduced, so every
            # rank takes the same branch -- including the raise below)
            from .engine import DenseMU as _D, DEFAULT_BACKEND_FACTORY
            be = DEFAULT_BACKEND_FACTORY()
            single = _D.auto_mode(V, self.W.data, self.H.data, be.pad_rank(R), be, beta, group)
            if single is not None:
                precision = single
            elif group is None:
                wide = True
            else:
                raise NotImplementedError(
                    "precision='auto' on a column-sharded fit at rank 129..256 needs a single-plane fp16 mode (both "
                    f"dimensions >= {_D.F16_MIN_DIM} on every rank, data within fp16's range); pass precision='bf16' "
                    f"(factors ~1e-3), 'f16' or 'f16x' explicitly")
        if wide and group is not None:
            raise NotImplementedError('column sharding is implemented for the fused kernels (rank <= 256; bf16x3 up to '
                                      'rank 128)')
        if wide:
            from .nmfd_engine import WideRankMU
            return WideRankMU(V, self.W.data, self.H.data, beta, l1, l2, precision=precision,
                              update_W=self.W.requires_grad, update_H=self.H.requires_grad)
        return DenseMU(V, self.W.data, self.H.data, beta, l1, l2, precision=precision, group=group,
                       update_W=self.W.requires_grad, update_H=self.H.requires_grad, allow_f16=True,
                       ar_overlap=None if allreduce is None else allreduce == 'overlap', allow_gram=True,
                       ar_direct=None if allreduce is None else allreduce == 'direct')


class NMFD(BaseComponent):
    """1-D convolutive NMF ``V[b,c,l] ~ sum_t sum_r W[c,r,t] H[b,r,l-t]`` (reference: nmf.py:700-779)."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, T=1, **kwargs):
        if isinstance(Vshape, Iterable):
            if isinstance(T, Iterable):
                T, = tuple(T)
            batch, n_chan, length = Vshape
            rank = rank if rank else n_chan
            kwargs['W'] = (n_chan, rank, T)
            kwargs['H'] = (batch, rank, length - T + 1)
        super().__init__(rank, **kwargs)

    @staticmethod
    def reconstruct(H: Tensor, W: Tensor) -> Tensor:
        """``F.convNd(H, W.flip(..), padding=T - 1)`` (nmf.py:776-779; NMF2D / NMF3D inherit this with two / three shift
        axes) through the split-bf16 GEMM on the device.

        Differentiable like the reference's convolution: with grad mode on and ``H`` or ``W`` requiring grad the result
        carries a ``grad_fn`` whose backward is one ``nmfmu_conv_backward`` call (exact-fp32 MFMA, first order only).
        Under ``torch.no_grad()`` -- ``fit()``, ``BetaMu.step`` -- nothing is recorded."""
        from .nmfd_engine import reconstruct as _recon
        if torch.is_grad_enabled() and (H.requires_grad or W.requires_grad):
            _require_device(H, 'reconstruct')
            _require_device(W, 'reconstruct')
            return _ConvReconstructFn.apply(H, W)
        return _recon(H, W)

    def _make_engine(self, V, beta, l1, l2, precision, group, allreduce=None):
        from .nmfd_engine import ConvMU
        if group is not None:
            raise NotImplementedError('NMFD is not sharded (replicas only): sharding L needs a (T-1)-column halo')
        for p in (self.W, self.H):                      # the engine works on the parameters' storage in place
            if not p.data.is_contiguous():
                p.data = p.data.contiguous()
        return ConvMU(V, self.W.data, self.H.data, beta, l1, l2, precision=precision,
                      update_W=self.W.requires_grad, update_H=self.H.requires_grad)


def _ntuple(x, n):
    return tuple(x) if isinstance(x, Iterable) else (x,) * n


class NMF2D(NMFD):
    """2-D convolutive NMF ``V[b,c,l,m] ~ sum W[c,r,i,j] H[b,r,l-i,m-j]`` (reference: nmf.py:782-865).  Same engine
    as NMFD with two shift axes (explicit unfold / fold kernels, nmfmu_convnd_*)."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, kernel_size=1, **kwargs):
        if isinstance(Vshape, Iterable):
            kernel_size = _ntuple(kernel_size, 2)
            batch, channel, K, M = Vshape
            rank = rank if rank else K
            kwargs['W'] = (channel, rank) + kernel_size
            kwargs['H'] = (batch, rank, K - kernel_size[0] + 1, M - kernel_size[1] + 1)
        BaseComponent.__init__(self, rank, **kwargs)


class NMF3D(NMFD):
    """3-D convolutive NMF (reference: nmf.py:868-942); three shift axes."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, kernel_size=1, **kwargs):
        if isinstance(Vshape, Iterable):
            kernel_size = _ntuple(kernel_size, 3)
            batch, channel, N, K, M = Vshape
            rank = rank if rank else K
            kwargs['W'] = (channel, rank) + kernel_size
            kwargs['H'] = (batch, rank, N - kernel_size[0] + 1, K - kernel_size[1] + 1, M - kernel_size[2] + 1)
        BaseComponent.__init__(self, rank, **kwargs)
