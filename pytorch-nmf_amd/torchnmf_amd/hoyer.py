"""Hoyer's sparseness projection on the ROCm device (reference: ``_proj_func``, torchnmf/nmf.py:21-49).

``hoyer_project`` moves every slice of a tensor along ``dim`` to the closest non-negative point with a prescribed L1 norm
``k1`` and squared L2 norm ``k2`` (Hoyer 2004, section 3.3).  The reference projects one slice at a time in a Python loop
with a host sync in every pass; here ALL slices of a factor go through ONE call of ``nmfmu_hoyer_project`` (one workgroup
per slice, the data-dependent loop inside the kernel) and the per-slice targets are device tensors, so nothing waits for
the host.  ``BaseComponent.sparse_fit`` and ``trainer.SparsityProj`` are built on it.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor

from . import _capi

__all__ = ['hoyer_project']

LDS_MAX_ELEMS = 40896      # the longest slice the kernel keeps in LDS (include/nmfmu.h); longer ones are streamed from a copy


def slice_norms(x: Tensor, dim: int = 1) -> Tensor:
    """L2 norm of every slice of ``x`` along ``dim`` (``_get_norm``, nmf.py:131-136): plain torch reductions on x's device."""
    dims = [d for d in range(x.dim()) if d != dim % x.dim()]
    x2 = x * x
    return (x2.sum(dims) if dims else x2).sqrt()


def _targets(k, J: int, device, what: str) -> Tensor:
    if isinstance(k, Tensor):
        if k.device != device:
            raise _capi.NmfmuError(f'hoyer_project: {what} lives on {k.device}, x on {device}')
        k = k.detach().to(torch.float32).reshape(-1)
        if k.numel() == 1 and J != 1:
            k = k.expand(J)
        if k.numel() != J:
            raise ValueError(f'hoyer_project: {what} must hold one value per slice ({J}), got {k.numel()}')
        return k.contiguous()
    return torch.full((J,), float(k), dtype=torch.float32, device=device)


def project_(x: Tensor, k1, k2, dim: int = 1, lds_max_elems: Optional[int] = None) -> Tensor:
    """The launch itself: projects the slices of the contiguous fp32 device tensor ``x`` along ``dim`` in place and returns
    the per-slice status (int32, on the device; never read here): the number of passes made, negative when the cap of n
    passes ended the loop.  ``lds_max_elems`` overrides the residency threshold (tests)."""
    if x.device.type != 'cuda':
        raise _capi.NmfmuError(f'hoyer_project: tensors live on {x.device}; torchnmf_amd computes on an MI355X only '
                               f'(there is no CPU fallback)')
    assert x.dtype == torch.float32 and x.is_contiguous(), 'project_ needs a contiguous float32 tensor'
    lib = _capi.load()
    dim = dim % x.dim()
    outer, J, inner = 1, x.shape[dim], 1
    for d in range(dim):
        outer *= x.shape[d]
    for d in range(dim + 1, x.dim()):
        inner *= x.shape[d]
    if outer * inner == 0 or J == 0:
        return torch.zeros(J, dtype=torch.int32, device=x.device)
    k1 = _targets(k1, J, x.device, 'k1')
    k2 = _targets(k2, J, x.device, 'k2')
    lds = LDS_MAX_ELEMS if lds_max_elems is None else int(lds_max_elems)
    n_ws = lib.nmfmu_hoyer_project_ws(outer, J, inner, lds)
    _capi.check(min(n_ws, 0), 'nmfmu_hoyer_project_ws')
    ws = torch.empty(n_ws, dtype=torch.uint8, device=x.device) if n_ws > 0 else None
    status = torch.empty(J, dtype=torch.int32, device=x.device)
    _capi.check(lib.nmfmu_hoyer_project(x.data_ptr(), outer, J, inner, k1.data_ptr(), k2.data_ptr(), lds,
                                        ws.data_ptr() if ws is not None else None, status.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), 'nmfmu_hoyer_project')
    return status


@torch.no_grad()
def hoyer_project(x: Tensor, k1: Union[Tensor, float], k2: Union[Tensor, float], dim: int = 1, *,
                  out: Optional[Tensor] = None) -> Tensor:
    """Project every slice ``x.select(dim, j)`` onto ``{v >= 0, sum v = k1[j], sum v^2 = k2[j]}``.

    ``k1`` / ``k2``: one value per slice (a tensor on x's device) or a float for all of them.  Returns ``out`` (a new tensor
    when ``out`` is None); ``out is x`` projects in place -- without a copy when x is contiguous float32.  The arithmetic is
    fp32 whatever the dtype of ``x``.  Raises ``NmfmuError`` for CPU tensors."""
    if x.device.type != 'cuda':
        raise _capi.NmfmuError(f'hoyer_project: tensors live on {x.device}; torchnmf_amd computes on an MI355X only -- move '
                               f'them with .cuda() (there is no CPU fallback)')
    if out is not None and (out.shape != x.shape or out.device != x.device):
        raise ValueError('hoyer_project: out must have the shape and device of x')
    xd = x.detach()
    if out is x and xd.dtype == torch.float32 and xd.is_contiguous():
        project_(xd, k1, k2, dim)
        return x
    work = xd.to(torch.float32, copy=True).contiguous() if xd.dtype == torch.float32 else xd.float().contiguous()
    project_(work, k1, k2, dim)
    if out is None:
        return work if x.dtype == torch.float32 else work.to(x.dtype)
    out.detach().copy_(work)
    return out
