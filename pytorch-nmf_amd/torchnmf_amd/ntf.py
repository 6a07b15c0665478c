"""Non-negative tensor factorisation: the CP / PARAFAC model of a 3-way tensor, ``NTF(V.shape, rank).fit(V, weights=M)``.

``V[i, j, k] ~ sum_r A[i, r] B[j, r] C[k, r]`` fitted by the beta-divergence multiplicative update of ``NMF.fit`` (nmf.py:61-92),
``L = sum m d_beta(v | y)`` with optional dense weights ``m >= 0`` of ``V``'s shape (0 marks a missing entry: ``V`` may hold
anything there).  One half-step is one ``nmfmu_ntf_step`` call on the fp32 masters: the fused exact-fp32 MFMA kernel of
csrc/nmfmu_ntf.hip walks the three unfoldings of the row-major tensor in place and forms the Khatri-Rao rows 32 at a time in
LDS -- nothing of ``V``'s size and no Khatri-Rao matrix is allocated beyond ``V`` and ``M`` themselves.

A 3-D sparse COO tensor is fitted over its STORED entries, ``fit(V_sparse, unstored='missing' | 'zero')``: ``SparseNtfTarget``
holds one sorted copy per mode, one half-step is one ``nmfmu_sp_ntf_step`` call (csrc/nmfmu_sparse_ntf.hip: two panel rows
gathered per stored entry and multiplied in registers; under 'zero' the denominator comes from column sums or Gram matrices
of the factors).  ``sparse_ntf_terms`` / ``sparse_ntf_loss`` are the functional forms.

``fit(beta=2, solver='hals')`` is HALS (Cichocki & Phan 2009), the coordinate descent of ``NMF.fit(solver='hals')`` on tensors: a
half-step is the MTTKRP ``num[o] = sum_(a,b) V(o, a, b) Pa[a] o Pb[b]`` (``ntf_mttkrp``: csrc/nmfmu_ntf_mttkrp.hip, ``V`` read once,
no reconstruction; on a sparse 'zero' target the numerator of ``nmfmu_sp_ntf_terms``), two Gram matrices and one
``nmfmu_hals_sweep``.  ``precision='bf16x3'`` runs the dense MTTKRP in split bf16 (csrc/nmfmu_ntf_mttkrp_x3.hip: three bf16
MFMAs per product); the default is exact fp32.

``fit(beta=2, solver='ccd', unstored='missing')`` is the coordinate descent of ``NMF.fit(solver='ccd')`` on the CP model (the
CCD-TC of Karlsson, Kressner & Uschmajew 2016): with missing data every owner row has its own quadratic, so a half-step keeps
the residuals of the row's stored entries and walks the rank once -- one ``nmfmu_sp_ntf_ccd_sweep`` call
(csrc/nmfmu_sparse_ntf_ccd.hip: a wave per row, a workgroup per long row, two panel rows gathered per entry four coordinates
at a time and multiplied in registers).  ``ntf_ccd_sweep`` is the functional form.  ``gram_rows=`` sends the rows above that
many entries through their own normal equations instead (csrc/nmfmu_sparse_ntf_ccd_gram.hip: a row cut into parts over the
whole device, ``Q = sum q q^T`` by exact-fp32 MFMA, then the coordinate sweep on ``Q``) -- the route for a mode of few, long rows.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from . import _capi
from . import sparse_autograd as SA
from .constants import eps
from .hals import _sweep
from .engine import mu_gamma
from .nmf import _require_device, _sqrt2
from .wmu import check_weights

__all__ = ['NTF', 'NtfTarget', 'ntf_terms', 'ntf_loss', 'SparseNtfTarget', 'sparse_ntf_terms', 'sparse_ntf_loss', 'ntf_mttkrp',
           'ntf_ccd_sweep']

MAX_RANK = 256
MAX_CONTRACTION = 1 << 30      # csrc/nmfmu_ntf.hip: the flat contraction steps of a mode are ints
_CHUNK = 1 << 22      # elements per slice of the one-time scans of the target: their temporaries stay small beside V


def _check_shape(shape, rank: int) -> None:
    """The limits of the C entries, refused here before anything is scanned, allocated or launched."""
    if rank > MAX_RANK:
        raise NotImplementedError(f'NTF: rank {rank} > {MAX_RANK}, the limit of the exact-fp32 kernels')
    I, J, K = shape
    if max(J * K, I * K, I * J) > MAX_CONTRACTION:
        raise NotImplementedError(f'NTF: a mode of {tuple(shape)} contracts over more than 2^30 entries, the limit of the kernels')


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class NtfTarget:
    """A dense 3-way target with optional weights, prepared once: contiguous fp32 ``V`` (and ``M``), the two flags of
    nmf.py:329-336 (over the weighted entries only when weights are given) and the terms of the loss that hold ``v`` alone
    per beta.  The scans run over slices of the flat tensor, so nothing of ``V``'s size is allocated.  ``checked``: the
    weights already went through ``wmu.check_weights`` (``fit`` validates them before it asks for the device)."""

    def __init__(self, V: Tensor, weights=None, checked: bool = False):
        if not isinstance(V, Tensor) or V.is_sparse or V.dim() != 3:
            raise ValueError('an NTF target is a dense 3-D tensor')
        self.M = weights if weights is None or checked else check_weights(V, weights)
        self.V = V.detach().float().contiguous()
        self.shape, self.device = tuple(V.shape), V.device
        self._v_term = {}
        bad = torch.zeros((), dtype=torch.bool, device=self.device)
        zero = torch.zeros((), dtype=torch.bool, device=self.device)
        for v, m in self._slices():
            if m is not None:
                v = torch.where(m > 0, v, torch.ones((), device=self.device))
            bad |= ~(v >= 0).all()                                     # negative or NaN where it counts
            zero |= (v == 0).any()
        self.bad, self.has_zero = bool(bad.item()), bool(zero.item())

    def _slices(self):
        v, m = self.V.view(-1), None if self.M is None else self.M.view(-1)
        for at in range(0, v.numel(), _CHUNK):
            yield v[at:at + _CHUNK], None if m is None else m[at:at + _CHUNK]

    def v_term(self, beta: float) -> float:
        """``sum m * (the terms of metrics.beta_div that hold v alone)`` (metrics.py:22, 39, 57, 85-96) in float64 -- what
        ``nmfmu_ntf_loss`` takes as ``v_term``.  Once per (target, beta); a Python float."""
        if beta not in self._v_term:
            tot = torch.zeros((), dtype=torch.float64, device=self.device)
            for v, m in self._slices() if beta != 2.0 else ():
                vd = (v if m is None else torch.where(m > 0, v, torch.ones((), device=self.device))).double()
                if beta == 1.0:
                    t = vd * (vd + eps).log() - vd
                elif beta == 0.0:
                    t = -(vd + eps).log() - 1.0
                else:
                    t = (vd + eps if beta < 0 else vd).pow(beta)
                tot += (t if m is None else m.double() * t).sum()
            self._v_term[beta] = float(tot.item())
        return self._v_term[beta]


def _check_tile(tile) -> None:
    if tile not in (None, 'wide', 'short'):
        raise ValueError(f"tile must be None, 'wide' or 'short', got {tile!r}")


def _tile_entries(lib, tile, rows: int, contraction: int, r_pad: int):
    """(workspace rule, terms entry, step entry, the step's name) of the mode's tile: the 128-row tile of csrc/nmfmu_ntf.hip
    or the 32-row tile of csrc/nmfmu_ntf_short.hip.  ``tile`` None: the library's choice, ``nmfmu_ntf_tile``."""
    short = lib.nmfmu_ntf_tile(rows, contraction, r_pad) == 1 if tile is None else tile == 'short'
    if short:
        return lib.nmfmu_ntf_short_ws, lib.nmfmu_ntf_short_terms, lib.nmfmu_ntf_short_step, 'nmfmu_ntf_short'
    return lib.nmfmu_ntf_ws, lib.nmfmu_ntf_terms, lib.nmfmu_ntf_step, 'nmfmu_ntf'


def _ntf_call(T: NtfTarget, factors: Sequence[Tensor], mode: int, beta: float, step=None, nsplit: int = 0, _fill=None,
              _ws=None, tile=None):
    """``nmfmu_ntf_terms`` (``step`` None: returns (num, den), fp32 ``[dim_mode, r_pad]``) or ``nmfmu_ntf_step`` (``step`` =
    (l1, l2, gamma): ``factors[mode]`` updated in place).  ``factors``: three contiguous fp32 ``[dim_n, R]``.  Enqueued only.
    ``_fill``: tests pre-fill the outputs and the workspace with it.  ``tile``: None (the library's choice for this mode),
    'wide' or 'short' -- the ``nmfmu_ntf_short_*`` entries."""
    _check_tile(tile)
    lib = _capi.load()
    I, J, K = T.shape
    owner = factors[mode]
    pa, pb = (f for n, f in enumerate(factors) if n != mode)
    rows, R = owner.shape
    assert tuple(f.shape for f in factors) == ((I, R), (J, R), (K, R))
    r_pad = lib.nmfmu_pad_rank(R)
    contraction = I * J * K // rows
    ws_rule, terms_entry, step_entry, name = _tile_entries(lib, tile, rows, contraction, r_pad)
    n_float = ws_rule(rows, contraction, r_pad, nsplit)
    ws = _ws if _ws is not None else torch.empty(max(n_float, 1), dtype=torch.float32, device=T.device)
    assert ws.numel() >= n_float
    if _fill is not None:
        ws.fill_(_fill)
    head = (T.V.data_ptr(), None if T.M is None else T.M.data_ptr(), I, J, K, mode, owner.data_ptr(), pa.data_ptr(),
            pb.data_ptr(), R, r_pad, beta)
    if step is not None:
        l1, l2, gamma = step
        _capi.check(step_entry(*head, l1, l2, gamma, nsplit, ws.data_ptr(), _stream()), name + '_step')
        return None
    num = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    den = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    _capi.check(terms_entry(*head, nsplit, ws.data_ptr(), num.data_ptr(), den.data_ptr(), _stream()), name + '_terms')
    return num, den


def _ntf_loss(T: NtfTarget, factors: Sequence[Tensor], beta: float, part=None, out=None) -> Tensor:
    """The loss as a 1-element float64 device tensor.  Enqueued only (the terms of v alone are cached on the target)."""
    lib = _capi.load()
    I, J, K = T.shape
    A, B, Cf = factors
    if part is None:
        part = torch.empty(lib.nmfmu_ntf_loss_parts(I, J, K), dtype=torch.float64, device=T.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=T.device)
    _capi.check(lib.nmfmu_ntf_loss(T.V.data_ptr(), None if T.M is None else T.M.data_ptr(), I, J, K, A.data_ptr(), B.data_ptr(),
                                   Cf.data_ptr(), A.shape[1], beta, T.v_term(beta), part.data_ptr(), out.data_ptr(), _stream()),
                'nmfmu_ntf_loss')
    return out


def _prepare(V, weights, factors):
    """The refusals first (shape limits, the device), then the target's scans and the fp32 factors."""
    _check_shape(tuple(V.shape), factors[0].shape[1])
    for t in (V.V if isinstance(V, NtfTarget) else V, *factors):
        _require_device(t, 'NTF')
    T = V if isinstance(V, NtfTarget) else NtfTarget(V, weights)
    return T, [f.detach().float().contiguous() for f in factors]


def ntf_terms(V, weights, factors: Sequence[Tensor], mode: int, beta: float, nsplit: int = 0, tile=None):
    """``(num, den)`` of the half-step of ``mode`` (0, 1 or 2), fp32 ``[dim_mode, r_pad]`` with zeros in the padded rank
    columns; ``den - num`` is the gradient of the loss with respect to ``factors[mode]``.  ``V``: a dense ``[I, J, K]`` device
    tensor with ``weights`` of its shape or None, or an ``NtfTarget`` prepared once.  ``tile``: None -- the library chooses
    (the 32-row tile for a mode of at most 32 rows over a long contraction, else the 128-row tile) -- or 'wide' / 'short'."""
    _check_tile(tile)
    T, fs = _prepare(V, weights, factors)
    return _ntf_call(T, fs, int(mode), float(beta), nsplit=nsplit, tile=tile)


def ntf_loss(V, weights, factors: Sequence[Tensor], beta: float) -> Tensor:
    """``sum weights * d_beta(V | reconstruction)`` with the reference's ``beta_div`` terms, without the reconstruction: a
    0-dim float64 device tensor.  Arguments as for ``ntf_terms``."""
    T, fs = _prepare(V, weights, factors)
    return _ntf_loss(T, fs, float(beta))[0]


def _check_precision(precision) -> None:
    if precision not in ('fp32', 'bf16x3'):
        raise ValueError(f"precision must be 'fp32' or 'bf16x3', got {precision!r}")


def _mttkrp_call(T: NtfTarget, factors: Sequence[Tensor], mode: int, nsplit: int = 0, tile=None, _fill=None, _ws=None,
                 out=None, precision: str = 'fp32') -> Tensor:
    """``nmfmu_ntf_mttkrp`` (``precision='bf16x3'``: ``nmfmu_ntf_mttkrp_x3``) of ``mode``: fp32 ``[dim_mode, r_pad]`` (``out`` or a
    new tensor).  ``factors``: three contiguous fp32 ``[dim_n, R]``.  Enqueued only.  ``tile``: None (``nmfmu_ntf_tile``'s choice
    for this mode), 'wide' or 'short'.  ``_fill``: tests pre-fill the output and the workspace with it."""
    _check_tile(tile)
    _check_precision(precision)
    lib = _capi.load()
    I, J, K = T.shape
    pa, pb = (f for n, f in enumerate(factors) if n != mode)
    rows, R = factors[mode].shape
    assert tuple(f.shape for f in factors) == ((I, R), (J, R), (K, R))
    r_pad = lib.nmfmu_pad_rank(R)
    contraction = I * J * K // rows
    short = int(lib.nmfmu_ntf_tile(rows, contraction, r_pad) == 1 if tile is None else tile == 'short')
    n_float = lib.nmfmu_ntf_mttkrp_ws(rows, contraction, r_pad, nsplit, short)
    ws = _ws if _ws is not None else torch.empty(max(n_float, 1), dtype=torch.float32, device=T.device)
    assert ws.numel() >= n_float
    num = out if out is not None else torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    if _fill is not None:
        ws.fill_(_fill)
        num.fill_(_fill)
    name = 'nmfmu_ntf_mttkrp' if precision == 'fp32' else 'nmfmu_ntf_mttkrp_x3'
    _capi.check(getattr(lib, name)(T.V.data_ptr(), I, J, K, mode, pa.data_ptr(), pb.data_ptr(), R, r_pad, nsplit, short,
                                   ws.data_ptr(), num.data_ptr(), _stream()), name)
    return num


class _Dense:
    """What ``ntf_mttkrp`` needs of a dense tensor: contiguous fp32 ``V``, none of ``NtfTarget``'s scans."""

    def __init__(self, V: Tensor):
        self.V, self.shape, self.device = V.detach().float().contiguous(), tuple(V.shape), V.device


def ntf_mttkrp(V, factors: Sequence[Tensor], mode: int, nsplit: int = 0, tile=None, precision: str = 'fp32') -> Tensor:
    """The MTTKRP of ``mode`` (0, 1 or 2): ``num[o, r] = sum_(a, b) V(o, a, b) Pa[a, r] Pb[b, r]`` over the other two modes, fp32
    ``[dim_mode, r_pad]`` with zeros in the padded rank columns -- the numerator of a Frobenius half-step, one pass over ``V``
    on the exact-fp32 MFMA kernel of csrc/nmfmu_ntf_mttkrp.hip.  ``V``: a dense ``[I, J, K]`` device tensor or an unweighted
    ``NtfTarget``.  ``nsplit``: parts of the contraction (0: the library's rule).  ``tile``: as for ``ntf_terms``.
    ``precision``: 'fp32', or 'bf16x3' -- the split-bf16 kernel of csrc/nmfmu_ntf_mttkrp_x3.hip: ``V`` and the Khatri-Rao rows
    as bf16 hi and lo planes, three bf16 MFMAs per product, every element within ``3 2^-18 (1 + 2^-8) + (3 L + 64) 2^-24``
    relative of the exact sum (``L``: the contraction length) at 16/3 of the fp32 MFMA rate."""
    _check_tile(tile)
    _check_precision(precision)
    if isinstance(V, NtfTarget):
        if V.M is not None:
            raise ValueError('ntf_mttkrp takes an unweighted target')
    elif not isinstance(V, Tensor) or V.is_sparse or V.dim() != 3:
        raise ValueError('ntf_mttkrp takes a dense 3-D tensor or an NtfTarget')
    _check_shape(tuple(V.shape), factors[0].shape[1])
    for t in (V.V if isinstance(V, NtfTarget) else V, *factors):
        _require_device(t, 'NTF')
    T = V if isinstance(V, NtfTarget) else _Dense(V)
    return _mttkrp_call(T, [f.detach().float().contiguous() for f in factors], int(mode), nsplit=nsplit, tile=tile,
                        precision=precision)


# ---- sparse targets: the stored entries only ------------------------------------------------------------------------------------
def plan_sparse_ntf(indices: Tensor, vals: Tensor, shape, chunk: int):
    """The three sorted copies of a coalesced 3-D COO tensor and their work lists (pure torch, any device).  ``indices``:
    int64 ``[3, nnz]`` in lexicographic order, as ``coalesce`` leaves them.  Per mode ``n`` a dict with ``rowptr``
    ``[dim_n + 1]``, ``idx_a`` / ``idx_b`` (int32 rows of the other two factors, ascending mode number), ``vals`` -- all sorted
    by (owner index, a, b): a stable sort by the owner index of the lexicographic order -- and ``seg`` / ``multi`` / ``n_ws``
    of ``sparse_autograd.plan_worklist``."""
    modes = []
    for n, dim in enumerate(shape):
        order = None if n == 0 else torch.sort(indices[n], stable=True)[1]
        own, (ia, ib) = indices[n], (indices[m] for m in range(3) if m != n)
        if order is not None:
            own, ia, ib = own[order], ia[order], ib[order]
        rowptr = torch.zeros(dim + 1, dtype=torch.int64, device=indices.device)
        rowptr[1:] = torch.cumsum(torch.bincount(own, minlength=dim), 0)
        rowptr = rowptr.to(torch.int32)
        seg, multi, n_ws = SA.plan_worklist(rowptr, chunk)
        modes.append(dict(rowptr=rowptr, idx_a=ia.to(torch.int32).contiguous(), idx_b=ib.to(torch.int32).contiguous(),
                          vals=(vals if order is None else vals[order]).contiguous(), seg=seg, multi=multi, n_ws=n_ws))
    return modes


class SparseNtfTarget:
    """A 3-D sparse-COO target prepared once on the device: coalesced, one copy per mode sorted by (owner index, a, b) with
    its segment work lists (``plan_sparse_ntf``), the two flags of nmf.py:329-336 over the STORED values and the float64
    terms of the loss that hold ``v`` alone per (beta, unstored).  ``chunk``: stored entries per segment (``None``: no row is
    split).  ``nnz`` and every dimension stay below 2^31; the 2^30 contraction limit of the dense kernels does not apply."""

    def __init__(self, V: Tensor, chunk=SA.DEFAULT_CHUNK):
        if not isinstance(V, Tensor) or not V.is_sparse or V.dim() != 3:
            raise ValueError('a sparse NTF target is a 3-D sparse COO tensor')
        if V.device.type != 'cuda':
            raise _capi.NmfmuError('SparseNtfTarget: the target must live on the ROCm device (no CPU fallback)')
        V = V.detach().coalesce()
        if not (V._nnz() < 2 ** 31 and max(V.shape) < 2 ** 31 and min(V.shape) > 0):
            raise ValueError(f'SparseNtfTarget: nnz ({V._nnz()}) and every dimension of {tuple(V.shape)} must be below 2^31, '
                             f'and no dimension empty')
        self.shape, self.device, self.nnz = tuple(V.shape), V.device, int(V._nnz())
        self.vals = V.values().float()
        if chunk is None:
            chunk = max(int(torch.bincount(V.indices()[n], minlength=1).max()) for n in range(3)) if self.nnz else 1
        self.chunk = int(chunk)
        self.modes = plan_sparse_ntf(V.indices(), self.vals, self.shape, self.chunk)
        self.spare = torch.zeros(4, dtype=torch.float32, device=V.device)      # sparse_autograd.entries
        self.bad = bool((~(self.vals >= 0)).any().item()) if self.nnz else False
        self.has_zero = bool((self.vals == 0).any().item()) if self.nnz else False
        self._v_term = {}

    def v_term(self, beta: float, unstored: str) -> float:
        """What ``nmfmu_sp_ntf_loss`` takes as ``v_term``, in float64.  'missing': the terms of ``metrics.beta_div`` that hold
        v alone.  'zero': the same at beta 1 (an unstored zero adds nothing), 1/2 sum v^2 at beta 2, where the kernel sums
        -v s and the positive part carries 1/2 s^2.  Once per (target, beta, unstored); a Python float."""
        key = (beta, unstored)
        if key not in self._v_term:
            if unstored == 'zero' and beta == 2.0:
                vd = self.vals.double()
                self._v_term[key] = float((vd @ vd).item() * 0.5)
            else:
                self._v_term[key] = SA.masked_v_term(self.vals, beta)
        return self._v_term[key]


def _check_sparse(shape, factors, beta: float, unstored, weights=None) -> None:
    """The refusals of the sparse path in their documented order, all before the device is asked."""
    if unstored not in ('zero', 'missing'):
        raise ValueError(f"unstored must be 'zero' or 'missing', got {unstored!r}")
    if len(shape) != 3:
        raise NotImplementedError(f'NTF factorises tensors of order 3, got order {len(shape)}')
    if tuple(shape) != tuple(f.shape[0] for f in factors):
        raise ValueError(f'target {tuple(shape)} does not match the factors {tuple(f.shape[0] for f in factors)}')
    if weights is not None:
        raise NotImplementedError('NTF.fit on a sparse target takes no weights: the stored set is the mask')
    if unstored == 'zero' and float(beta) not in (1.0, 2.0):
        raise NotImplementedError(f"unstored='zero' supports beta in {{1, 2}}, got {float(beta):g}: for any other beta the "
                                  f"positive term runs over every entry of the tensor; use unstored='missing'")
    rank = factors[0].shape[1]
    if rank > MAX_RANK:
        raise NotImplementedError(f'NTF: rank {rank} > {MAX_RANK}, the limit of the sparse kernels')


def _colsum(lib, f: Tensor) -> Tensor:
    R = f.shape[1]
    part = torch.empty(R * 128, dtype=torch.float32, device=f.device)
    cs = torch.empty(R, dtype=torch.float32, device=f.device)
    _capi.check(lib.nmfmu_rank_sums(f.data_ptr(), f.shape[0], R, 1, part.data_ptr(), cs.data_ptr(), _stream()), 'nmfmu_rank_sums')
    return cs


def _gram(lib, f: Tensor) -> Tensor:
    R = f.shape[1]
    part = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device=f.device)
    g = torch.empty(R * R, dtype=torch.float32, device=f.device)
    _capi.check(lib.nmfmu_gram(f.data_ptr(), f.shape[0], R, part.data_ptr(), g.data_ptr(), _stream()), 'nmfmu_gram')
    return g


def _zero_pos(lib, owner: Tensor, pa: Tensor, pb: Tensor, beta: float, r_pad: int):
    """(pos, pos_plane) of ``nmfmu_sp_ntf_*`` under unstored = 'zero': the denominator over EVERY entry of the tensor from
    the small per-factor terms -- colsum(Pa) o colsum(Pb) (beta 1) or owner @ (Gram(Pa) o Gram(Pb)) (beta 2)."""
    rows, R = owner.shape
    if beta == 1.0:
        pos = torch.zeros(r_pad, dtype=torch.float32, device=owner.device)
        pos[:R] = _colsum(lib, pa) * _colsum(lib, pb)
        return pos, 0
    g = _gram(lib, pa) * _gram(lib, pb)
    pos = torch.empty(rows * r_pad, dtype=torch.float32, device=owner.device)
    _capi.check(lib.nmfmu_rowmat(owner.data_ptr(), rows, R, g.data_ptr(), pos.data_ptr(), r_pad, _stream()), 'nmfmu_rowmat')
    return pos, 1


def _sparse_call(T: SparseNtfTarget, factors: Sequence[Tensor], mode: int, beta: float, unstored: str, step=None,
                 stage: int = 0, _fill=None, _ws=None):
    """``nmfmu_sp_ntf_terms`` (``step`` None: returns (num, den), fp32 ``[dim_mode, r_pad]``) or ``nmfmu_sp_ntf_step``
    (``step`` = (l1, l2, gamma): ``factors[mode]`` updated in place).  ``factors``: three contiguous fp32 ``[dim_n, R]``.
    Enqueued only.  ``stage``: 0 the library's rule, 1 no panel in LDS, 2 every panel that fits.  ``_fill``: tests pre-fill
    the outputs and the workspace with it."""
    lib = _capi.load()
    owner = factors[mode]
    pa, pb = (f for n, f in enumerate(factors) if n != mode)
    rows, R = owner.shape
    assert tuple(f.shape for f in factors) == tuple((d, R) for d in T.shape)
    r_pad = lib.nmfmu_pad_rank(R)
    m = T.modes[mode]
    n_float = lib.nmfmu_sp_ntf_ws(m['n_ws'], r_pad)
    ws = _ws if _ws is not None else torch.empty(max(n_float, 1), dtype=torch.float32, device=T.device)
    assert ws.numel() >= n_float
    if _fill is not None:
        ws.fill_(_fill)
    zero = unstored == 'zero'
    pos, plane = _zero_pos(lib, owner, pa, pb, beta, r_pad) if zero else (None, 0)
    head = (m['seg'].data_ptr(), m['seg'].shape[0], m['multi'].data_ptr() if m['multi'].shape[0] else None, m['multi'].shape[0],
            SA.entries(m['idx_a'], T.spare), SA.entries(m['idx_b'], T.spare), SA.entries(m['vals'], T.spare), T.nnz,
            owner.data_ptr(), pa.data_ptr(), pa.shape[0], pb.data_ptr(), pb.shape[0], R, beta, int(zero),
            pos.data_ptr() if zero else None, plane)
    if step is not None:
        l1, l2, gamma = step
        _capi.check(lib.nmfmu_sp_ntf_step(*head, l1, l2, gamma, ws.data_ptr(), r_pad, stage, _stream()), 'nmfmu_sp_ntf_step')
        return None
    num = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    den = torch.empty(rows, r_pad, dtype=torch.float32, device=T.device)
    if _fill is not None:
        num.fill_(_fill)
        den.fill_(_fill)
    _capi.check(lib.nmfmu_sp_ntf_terms(*head, ws.data_ptr(), num.data_ptr(), den.data_ptr(), r_pad, stage, _stream()),
                'nmfmu_sp_ntf_terms')
    return num, den


def _sparse_loss(T: SparseNtfTarget, factors: Sequence[Tensor], beta: float, unstored: str, stage: int = 0, part=None,
                 out=None) -> Tensor:
    """The loss as a 1-element float64 device tensor.  Enqueued only.  Under 'zero' the positive part over every entry of
    the tensor is added here: ``sum_r csA csB csC`` (beta 1) or ``1/2 sum G_A o G_B o G_C`` (beta 2), float64 on the device."""
    lib = _capi.load()
    A, B, Cf = factors
    m = T.modes[0]
    n_seg = m['seg'].shape[0]
    if part is None:
        part = torch.empty((n_seg + 3) // 4, dtype=torch.float64, device=T.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=T.device)
    zero = unstored == 'zero'
    _capi.check(lib.nmfmu_sp_ntf_loss(m['seg'].data_ptr(), n_seg, SA.entries(m['idx_a'], T.spare), SA.entries(m['idx_b'], T.spare),
                                      SA.entries(m['vals'], T.spare), T.nnz, A.data_ptr(), B.data_ptr(), B.shape[0], Cf.data_ptr(),
                                      Cf.shape[0], A.shape[1], beta, int(zero), T.v_term(beta, unstored), part.data_ptr(),
                                      out.data_ptr(), stage, _stream()), 'nmfmu_sp_ntf_loss')
    if not zero:
        return out
    small = [(_colsum if beta == 1.0 else _gram)(lib, f).double() for f in factors]
    pos = (small[0] * small[1] * small[2]).sum()
    return out + (pos if beta == 1.0 else 0.5 * pos)


def _prepare_sparse(T, factors, beta, unstored):
    shape = tuple(T.shape)
    _check_sparse(shape, factors, beta, unstored)
    for f in factors:
        _require_device(f, 'NTF')
    if not isinstance(T, SparseNtfTarget):
        if not (isinstance(T, Tensor) and T.is_sparse):
            raise ValueError('the target must be a 3-D sparse COO tensor or a SparseNtfTarget')
        T = SparseNtfTarget(T)
    return T, [f.detach().float().contiguous() for f in factors]


def sparse_ntf_terms(T, factors: Sequence[Tensor], mode: int, beta: float, unstored: str, stage: int = 0):
    """``(num, den)`` of the half-step of ``mode`` over the stored entries of ``T`` (a 3-D sparse COO device tensor or a
    ``SparseNtfTarget`` prepared once), fp32 ``[dim_mode, r_pad]`` with zeros in the padded rank columns; ``den - num`` is
    the gradient of the loss with respect to ``factors[mode]``.  ``unstored``: 'missing' -- the unstored entries are unknown,
    every beta; 'zero' -- they are observed zeros, beta in {1, 2}, and ``den`` is the factorised denominator."""
    T, fs = _prepare_sparse(T, factors, beta, unstored)
    return _sparse_call(T, fs, int(mode), float(beta), unstored, stage=stage)


def sparse_ntf_loss(T, factors: Sequence[Tensor], beta: float, unstored: str, stage: int = 0) -> Tensor:
    """The beta-divergence between ``T`` and the reconstruction, over the stored entries ('missing') or with every unstored
    entry an observed zero ('zero', beta in {1, 2}), without the reconstruction: a 0-dim float64 device tensor."""
    T, fs = _prepare_sparse(T, factors, beta, unstored)
    return _sparse_loss(T, fs, float(beta), unstored, stage)[0]


class _HalsNtf:
    """The half-steps and the loss of ``NTF.fit(beta=2, solver='hals')`` on the contiguous fp32 masters ``fs``, updated in place.

    A half-step of mode n: the numerator (dense: ``nmfmu_ntf_mttkrp``; sparse 'zero': the ``num`` plane of
    ``nmfmu_sp_ntf_terms`` at beta 2, the MTTKRP over the stored entries), ``G = Gram(Pa) o Gram(Pb)`` (symmetric) and one
    ``nmfmu_hals_sweep`` on the owner.  Before the first half-step or loss the trainable factors are scaled once, as
    ``HalsEngine`` does: ``a = <V, Y> / <Y, Y>`` with ``<V, Y> = sum num_0 o A`` and ``<Y, Y> = sum G_A o G_B o G_C`` (float64 dots),
    each of the t trainable factors times ``a^(1/t)`` (skipped unless a is finite and positive), then clamped to >= eps.

    The dense loss is ``1/2 |V|^2 - <V, Y> + 1/2 sum G_A o G_B o G_C`` in float64; ``<V, Y>`` is the dot of the last half-step's
    numerator with its owner after the sweep (that numerator came from the two factors that have not changed since), so a
    checkpoint costs no pass over ``V``.  Like ``HalsEngine``'s, the value loses digits when the fit is nearly exact: it is a
    difference of numbers of the size of ``|V|^2``.  The sparse loss is ``_sparse_loss``."""

    def __init__(self, T, fs, train, l1: float, l2: float, tile=None, precision: str = 'fp32'):
        self.T, self.fs, self.train, self.l1, self.l2, self.tile = T, fs, [bool(t) for t in train], l1, l2, tile
        self.precision = precision      # of every dense numerator: the half-steps', the initial scale's and the loss's
        self.sparse = isinstance(T, SparseNtfTarget)
        self.lib = lib = _capi.load()
        self.rank = R = fs[0].shape[1]
        self._scaled, self._fresh = False, None      # _fresh: the mode whose numerator is num of the current factors
        self.num = None
        if self.sparse:
            self.part = torch.empty((T.modes[0]['seg'].shape[0] + 3) // 4, dtype=torch.float64, device=T.device)
            self.out = torch.zeros(1, dtype=torch.float64, device=T.device)
            self.ws = torch.empty(max(1, *(lib.nmfmu_sp_ntf_ws(m['n_ws'], lib.nmfmu_pad_rank(R)) for m in T.modes)),
                                  dtype=torch.float32, device=T.device)
            return
        I, J, K = T.shape
        r_pad = lib.nmfmu_pad_rank(R)
        n_ws = 1
        for d in T.shape:      # per mode by the tile that mode takes
            c = I * J * K // d
            short = int(lib.nmfmu_ntf_tile(d, c, r_pad) == 1 if tile is None else tile == 'short')
            n_ws = max(n_ws, lib.nmfmu_ntf_mttkrp_ws(d, c, r_pad, 0, short))
        self.ws = torch.empty(n_ws, dtype=torch.float32, device=T.device)
        self.bufs = [torch.empty(d, r_pad, dtype=torch.float32, device=T.device) for d in T.shape]
        part = torch.empty(1024, dtype=torch.float64, device=T.device)
        out = torch.zeros(2, dtype=torch.float64, device=T.device)
        _capi.check(lib.nmfmu_norms(T.V.data_ptr(), T.V.numel(), part.data_ptr(), out.data_ptr(), _stream()), 'nmfmu_norms')
        self.half_v2 = 0.5 * float(out[1].item())

    def _numerator(self, mode: int) -> Tensor:
        if self.sparse:
            return _sparse_call(self.T, self.fs, mode, 2.0, 'zero', _ws=self.ws)[0]
        return _mttkrp_call(self.T, self.fs, mode, tile=self.tile, _ws=self.ws, out=self.bufs[mode], precision=self.precision)

    def _vy(self) -> Tensor:
        """``<V, Y>`` of the current factors, a 0-dim float64 device tensor."""
        if self._fresh is None:
            self.num, self._fresh = self._numerator(0), 0
        return (self.num[:, :self.rank].double() * self.fs[self._fresh].double()).sum()

    def _yy(self) -> Tensor:
        g = [_gram(self.lib, f).double() for f in self.fs]
        return (g[0] * g[1] * g[2]).sum()

    def _ensure_scaled(self) -> None:
        if self._scaled:
            return
        self._scaled = True
        t = sum(self.train)
        if t:
            vy, yy = float(self._vy().item()), float(self._yy().item())
            a = vy / yy if yy != 0 else float('nan')
            if a > 0 and a != float('inf'):
                for f, on in zip(self.fs, self.train):
                    if on:
                        f.mul_(a ** (1.0 / t))
                self._fresh = None
        for f, on in zip(self.fs, self.train):
            if on:
                f.clamp_(min=eps)
                self._fresh = None

    def half_step(self, mode: int) -> None:
        if not self.train[mode]:
            return
        self._ensure_scaled()
        pa, pb = (f for n, f in enumerate(self.fs) if n != mode)
        self.num = self._numerator(mode)
        g = _gram(self.lib, pa) * _gram(self.lib, pb)
        _sweep(self.fs[mode], self.num, self.num.stride(0), g, self.l1, self.l2)
        self._fresh = mode

    def divergence(self) -> float:
        """The plain Frobenius loss (no regularisation terms).  One host sync."""
        self._ensure_scaled()
        if self.sparse:
            return float(_sparse_loss(self.T, self.fs, 2.0, 'zero', part=self.part, out=self.out).item())
        return self.half_v2 - float(self._vy().item()) + 0.5 * float(self._yy().item())


def _ccd_order(m) -> Tensor:
    """The hand-out list of a mode's rows, longest first (a stable device sort of the counts)."""
    return torch.argsort(torch.diff(m['rowptr']), descending=True, stable=True).to(torch.int32)


def _ccd_call(T: SparseNtfTarget, factors: Sequence[Tensor], mode: int, l1: float, l2: float, order: Tensor, scratch: Tensor,
              limit: int = 0, wg_rows: int = 0, vec: int = 0) -> None:
    """``nmfmu_sp_ntf_ccd_sweep`` on ``factors[mode]``, in place.  ``factors``: three contiguous fp32 ``[dim_n, R]``; ``order``:
    int32, the rows to sweep (all ``dim_mode`` of them, or the rows the normal-equations route leaves); ``scratch``: at least
    ``nnz`` floats.  Enqueued only."""
    owner = factors[mode]
    pa, pb = (f for n, f in enumerate(factors) if n != mode)
    m = T.modes[mode]
    assert tuple(f.shape for f in factors) == tuple((d, owner.shape[1]) for d in T.shape)
    assert 0 < order.numel() <= owner.shape[0] and scratch.numel() >= T.nnz
    _capi.check(_capi.load().nmfmu_sp_ntf_ccd_sweep(
        m['rowptr'].data_ptr(), SA.entries(m['idx_a'], T.spare), SA.entries(m['idx_b'], T.spare), SA.entries(m['vals'], T.spare),
        order.data_ptr(), order.numel(), owner.data_ptr(), pa.data_ptr(), pa.shape[0], pb.data_ptr(), pb.shape[0],
        owner.shape[1], l1, l2, scratch.data_ptr(), int(limit), int(wg_rows), int(vec), _stream()), 'nmfmu_sp_ntf_ccd_sweep')


GRAM_CAP = 1 << 26      # floats: the workspace cap of nmfmu_sp_ntf_ccd_gram_part (256 MiB)


def _check_gram_rows(gram_rows, what: str) -> None:
    if gram_rows is not None and (isinstance(gram_rows, bool) or not isinstance(gram_rows, int) or gram_rows < 0):
        raise ValueError(f'{what}: gram_rows must be None or an integer >= 0, got {gram_rows!r}')


def _gram_plan(T: SparseNtfTarget, mode: int, gram_rows: int, part: int, rank: int) -> dict:
    """The parts plan of the normal-equations route for one mode, built once per (target, mode, gram_rows, part, rank) and kept
    on the target: the rows with more than ``gram_rows`` stored entries, longest first, in batches whose workspace stays under
    ``GRAM_CAP`` -- per batch ``(rows, row_part, part_row, n_long, n_parts)`` as ``nmfmu_sp_ntf_ccd_gram`` takes them -- the part
    length (``part`` == 0: the library's rule), the workspace floats of the largest batch, and ``rest``: the other rows in the
    sweep's order.  Building it reads the row counts back once; a half-step with a plan enqueues only."""
    plans = T.__dict__.setdefault('_gram_plans', {})
    key = (mode, gram_rows, part, rank)
    if key in plans:
        return plans[key]
    lib, m = _capi.load(), T.modes[mode]
    counts, order = torch.diff(m['rowptr']), _ccd_order(m)
    n_long = int((counts > gram_rows).sum().item())
    plan = dict(rest=order[n_long:].contiguous(), batches=[], ws=0, part=part)
    if n_long:
        rows = order[:n_long].contiguous()
        c = counts[rows.long()].cpu().long()      # descending
        if part == 0:
            part = lib.nmfmu_sp_ntf_ccd_gram_part(int(c.sum()), n_long, int(c[0]), rank,
                                                  torch.cuda.get_device_properties(T.device).multi_processor_count)
        most = GRAM_CAP // lib.nmfmu_sp_ntf_ccd_gram_ws(1, 1, rank)      # parts of a batch, each counted with a row's image
        n_parts = (c + (part - 1)) // part
        if int(n_parts[0]) > most:
            raise ValueError(f'ntf_ccd_sweep: parts of {part} entries cut the longest row ({int(c[0])} entries) into '
                             f'{int(n_parts[0])} parts, more than the {most} the workspace cap admits at rank {rank}')
        ends = torch.cat([torch.zeros(1, dtype=n_parts.dtype), torch.cumsum(n_parts, 0)])      # row r: parts ends[r] .. ends[r+1]-1
        at = 0
        while at < n_long:
            end = int(torch.searchsorted(ends, int(ends[at]) + most, right=True)) - 1      # rows at .. end-1 hold <= most parts
            row_part = (ends[at:end + 1] - ends[at]).to(torch.int32)
            part_row = torch.repeat_interleave(torch.arange(end - at, dtype=torch.int32), n_parts[at:end])
            k = int(row_part[-1])
            plan['batches'].append((rows[at:end].contiguous(), row_part.to(T.device), part_row.to(T.device), end - at, k))
            plan['ws'] = max(plan['ws'], lib.nmfmu_sp_ntf_ccd_gram_ws(k, end - at, rank))
            at = end
        plan['part'] = part
    plans[key] = plan
    return plan


def _gram_call(T: SparseNtfTarget, factors: Sequence[Tensor], mode: int, l1: float, l2: float, plan: dict, ws: Tensor,
               vec: int = 0) -> None:
    """``nmfmu_sp_ntf_ccd_gram`` on the long rows of ``plan``, batch after batch through one workspace.  Enqueued only."""
    owner = factors[mode]
    pa, pb = (f for n, f in enumerate(factors) if n != mode)
    m = T.modes[mode]
    assert tuple(f.shape for f in factors) == tuple((d, owner.shape[1]) for d in T.shape) and ws.numel() >= plan['ws']
    for rows, row_part, part_row, n_long, n_parts in plan['batches']:
        _capi.check(_capi.load().nmfmu_sp_ntf_ccd_gram(
            m['rowptr'].data_ptr(), m['idx_a'].data_ptr(), m['idx_b'].data_ptr(), m['vals'].data_ptr(), rows.data_ptr(),
            row_part.data_ptr(), part_row.data_ptr(), n_long, n_parts, plan['part'], owner.data_ptr(), pa.data_ptr(),
            pa.shape[0], pb.data_ptr(), pb.shape[0], owner.shape[1], l1, l2, ws.data_ptr(), int(vec), _stream()),
            'nmfmu_sp_ntf_ccd_gram')


@torch.no_grad()
def ntf_ccd_sweep(T, factors: Sequence[Tensor], mode: int, l1: float = 0.0, l2: float = 0.0, *, _limit: int = 0,
                  _order: Tensor = None, _wg_rows: int = 0, _vec: int = 0, gram_rows: Optional[int] = None,
                  _part: int = 0) -> Tensor:
    """One coordinate-descent pass over the rank on ``factors[mode]`` (contiguous fp32 ``[dim_mode, R]`` on the ROCm device), in
    place, over the stored entries of ``T`` alone -- the half-step of ``NTF.fit(solver='ccd')``.  With
    ``q_e,k = fp32(Pa[a_e, k] Pb[b_e, k])`` from the rows of the other two factors an entry names, every owner row with entries runs

        r_e = v_e - sum_k F[i, k] q_e,k
        for k = 0 .. R-1:   d = sum_e q_e,k^2      n = sum_e r_e q_e,k
                            f' = max(eps, (n + F[i, k] d - l1) / (d + l2 + eps))
                            r_e -= (f' - F[i, k]) q_e,k;   F[i, k] = f'

    and a row without entries is not touched.  ``T``: a ``SparseNtfTarget`` or a 3-D sparse-COO device tensor.  The other two
    factors are not written.  Returns ``factors[mode]``.  Raises ``NmfmuError`` for CPU tensors, ``NotImplementedError`` above
    rank 256.  Bit for bit ``ccd.ccd_sweep`` on the ``dim_mode x nnz`` matrix whose entry e names row e of the panel ``q``.

    ``_limit`` / ``_order`` / ``_wg_rows`` are ``ccd.ccd_sweep``'s, for the tests and the benchmark; ``_vec``: 0 -- the library's
    rule, 1 -- 4-byte loads of the panel values, 2 -- the rank in groups of four with 16-byte loads where ``R % 4 == 0``.  A
    row's bits depend on none of ``_limit``, ``_order`` and ``_vec``; ``_wg_rows`` moves rows between two summation orders.

    ``gram_rows``: None (the default: every row through the sweep above) or an integer >= 0 -- the rows with MORE than
    ``gram_rows`` stored entries are updated through their own normal equations instead (``nmfmu_sp_ntf_ccd_gram``,
    csrc/nmfmu_sparse_ntf_ccd_gram.hip): ``Q = sum_e q_e q_e^T`` and ``b = sum_e v_e q_e`` on an exact-fp32 MFMA kernel that cuts
    a row into parts across the whole device, then ``f_k = max(eps, (b_k - l1 - sum_(j != k) f_j Q[j, k]) / (Q[k, k] + l2 + eps))``
    for k = 0 .. R-1 -- the same coordinate minimiser at ``O(count R^2)`` instead of ``O(count R)`` work, for rows far longer
    than the rank that would otherwise keep one workgroup busy alone.  Those rows get OTHER BITS than the sweep's (another
    summation order; the same minimiser within the bound of DESIGN.md section 41); the rows at or below ``gram_rows`` keep the
    sweep's bits, and 0 sends every row with entries through the normal equations.  ``_part``: entries per part for the tests
    and the benchmark, a multiple of 32; 0 -- the library's rule."""
    what = 'ntf_ccd_sweep'
    if mode not in (0, 1, 2):
        raise ValueError(f'{what}: mode must be 0, 1 or 2, got {mode!r}')
    if not isinstance(T, SparseNtfTarget) and not (isinstance(T, Tensor) and T.is_sparse and T.dim() == 3):
        raise ValueError(f'{what}: T must be a SparseNtfTarget or a 3-D sparse-COO tensor')
    factors = list(factors)
    if len(factors) != 3 or not all(isinstance(f, Tensor) for f in factors):
        raise ValueError(f'{what}: factors must be three tensors [dim_n, R]')
    _check_gram_rows(gram_rows, what)
    names = ('factors[0]', 'factors[1]', 'factors[2]')
    for t, name in (*zip(factors, names), (T, 'T')):
        if t.device.type != 'cuda':
            raise _capi.NmfmuError(f'{what}: {name} lives on {t.device}; torchnmf_amd computes on an MI355X only -- move '
                                   f'the tensors with .cuda() (there is no CPU fallback)')
    F = factors[mode]
    for t, name in zip(factors, names):
        if t.dtype != torch.float32:
            raise TypeError(f'{what}: {name} must be float32, got {t.dtype}')
        if t.device != F.device:
            raise ValueError(f'{what}: {name} lives on {t.device}, factors[{mode}] on {F.device}')
    if F.dim() != 2 or not F.is_contiguous():
        raise ValueError(f'{what}: factors[{mode}] must be a contiguous 2-D tensor (it is updated in place)')
    R = F.shape[1]
    want = tuple((int(d), R) for d in T.shape)
    if any(f.dim() != 2 for f in factors) or tuple(tuple(f.shape) for f in factors) != want:
        raise ValueError(f'{what}: a {tuple(T.shape)} target needs factors {want}, got {[tuple(f.shape) for f in factors]}')
    if not 0 <= int(_limit) <= 512:
        raise ValueError(f'{what}: _limit must lie in 0 .. 512, got {_limit!r}')
    if int(_wg_rows) < 0:
        raise ValueError(f'{what}: _wg_rows must be >= 0, got {_wg_rows!r}')
    if int(_vec) not in (0, 1, 2):
        raise ValueError(f'{what}: _vec must be 0, 1 or 2, got {_vec!r}')
    if int(_part) < 0 or int(_part) % 32:
        raise ValueError(f'{what}: _part must be 0 or a positive multiple of 32, got {_part!r}')
    if R > MAX_RANK:
        raise NotImplementedError(f'{what}: rank {R} > {MAX_RANK}, the limit of the sparse kernels')
    if R == 0:
        return F
    if not isinstance(T, SparseNtfTarget):
        T = SparseNtfTarget(T)
    if T.nnz == 0:
        return F
    if _order is None:
        order = _ccd_order(T.modes[mode])
    else:
        order = _order.to(device=F.device, dtype=torch.int32).contiguous()
        if order.dim() != 1 or not torch.equal(torch.sort(order.long())[0], torch.arange(F.shape[0], device=F.device)):
            raise ValueError(f'{what}: _order must be a permutation of the {F.shape[0]} rows of mode {mode}')
    fs = [f.detach() if n == mode else f.detach().contiguous() for n, f in enumerate(factors)]
    if gram_rows is not None:
        plan = _gram_plan(T, int(mode), gram_rows, int(_part), R)
        if plan['batches']:
            ws = torch.empty(plan['ws'], dtype=torch.float32, device=F.device)
            _gram_call(T, fs, int(mode), float(l1), float(l2), plan, ws, int(_vec))
        # the sweep takes the other rows, in the order it was given
        order = plan['rest'] if _order is None else order[torch.diff(T.modes[mode]['rowptr'])[order.long()] <= gram_rows]
        if order.numel() == 0:
            return F
    scratch = torch.empty(max(T.nnz, 4), dtype=torch.float32, device=F.device)
    _ccd_call(T, fs, int(mode), float(l1), float(l2), order, scratch, int(_limit), int(_wg_rows), int(_vec))
    return F


class _CcdNtf:
    """The half-steps and the loss of ``NTF.fit(beta=2, solver='ccd', unstored='missing')`` on the contiguous fp32 masters ``fs``,
    updated in place.  A half-step of mode n is one ``nmfmu_sp_ntf_ccd_sweep`` call over that mode's sorted copy of the entries;
    the loss is ``_sparse_loss`` over the stored entries.  Before the first half-step or loss the trainable factors are scaled
    once, as ``CcdEngine`` does: ``a = sum_e v_e s_e / sum_e s_e^2`` over the stored entries -- ``<num, A> / <den, A>`` of mode 0's
    beta = 2 'missing' terms, float64 dots -- each of the t trainable factors times ``a^(1/t)`` (skipped unless a is finite and
    positive), then clamped to >= eps."""

    def __init__(self, T: SparseNtfTarget, fs, train, l1: float, l2: float, gram_rows: Optional[int] = None):
        self.T, self.fs, self.train, self.l1, self.l2 = T, fs, [bool(t) for t in train], float(l1), float(l2)
        self.rank = fs[0].shape[1]
        self.orders = [_ccd_order(m) if on and T.nnz else None for m, on in zip(T.modes, self.train)]
        # gram_rows: the rows above it go through their normal equations (_gram_plan), the sweep keeps the rest
        self.plans = [None] * 3
        if gram_rows is not None and self.rank:
            self.plans = [_gram_plan(T, n, gram_rows, 0, self.rank) if o is not None else None for n, o in enumerate(self.orders)]
            self.orders = [p['rest'] if p is not None else None for p in self.plans]
            self.ws = torch.empty(max(1, *(p['ws'] for p in self.plans if p is not None), 1), dtype=torch.float32,
                                  device=T.device)                                          # one for the three modes
        self.scratch = torch.empty(max(T.nnz, 4), dtype=torch.float32, device=T.device)      # one for the three modes
        self.part = torch.empty((T.modes[0]['seg'].shape[0] + 3) // 4, dtype=torch.float64, device=T.device)
        self.out = torch.zeros(1, dtype=torch.float64, device=T.device)
        self._scaled = False

    def _ensure_scaled(self) -> None:
        if self._scaled:
            return
        self._scaled = True
        t = sum(self.train)
        if t and self.T.nnz:
            num, den = _sparse_call(self.T, self.fs, 0, 2.0, 'missing')
            A = self.fs[0].double()
            vs = float((num[:, :self.rank].double() * A).sum().item())
            ss = float((den[:, :self.rank].double() * A).sum().item())
            a = vs / ss if ss != 0 else float('nan')
            if a > 0 and a != float('inf'):
                for f, on in zip(self.fs, self.train):
                    if on:
                        f.mul_(a ** (1.0 / t))
        for f, on in zip(self.fs, self.train):
            if on:
                f.clamp_(min=eps)

    def half_step(self, mode: int) -> None:
        if not self.train[mode]:
            return
        self._ensure_scaled()
        if self.plans[mode] is not None and self.plans[mode]['batches']:
            _gram_call(self.T, self.fs, mode, self.l1, self.l2, self.plans[mode], self.ws)
        if self.orders[mode] is not None and self.orders[mode].numel():
            _ccd_call(self.T, self.fs, mode, self.l1, self.l2, self.orders[mode], self.scratch)

    def divergence(self) -> float:
        """1/2 sum over the stored entries of (v - s)^2 (no regularisation terms).  One host sync."""
        self._ensure_scaled()
        return float(_sparse_loss(self.T, self.fs, 2.0, 'missing', part=self.part, out=self.out).item())


class NTF(nn.Module):
    """Non-negative CP factorisation ``V (I, J, K) ~ sum_r A[:, r] x B[:, r] x C[:, r]``.

    ``factors`` is a ``ParameterList`` of three ``[dim_n, rank]`` tensors, drawn from ``|N(0, 1)|`` like ``NMF``'s or given;
    ``trainable[n]`` False freezes factor ``n``.  ``fit`` is the multiplicative update on the HIP kernels; ``forward`` is a
    plain ``torch.einsum`` and there is no autograd support for the fit's kernels."""

    def __init__(self, Vshape=None, rank: Optional[int] = None, factors=None, trainable=(True, True, True)):
        super().__init__()
        if factors is not None:
            factors = list(factors)
            assert len(factors) == 3 and all(isinstance(f, Tensor) and f.dim() == 2 for f in factors), \
                'factors: three [dim_n, rank] tensors'
            assert len({f.shape[1] for f in factors}) == 1, 'the factors must share their rank'
            assert all(bool(torch.all(f >= 0.)) for f in factors), 'the factors should be non-negative.'
            assert rank is None or rank == factors[0].shape[1], 'rank does not match the factors'
            assert Vshape is None or tuple(Vshape) == tuple(f.shape[0] for f in factors), 'Vshape does not match the factors'
            data = [f.detach().clone() for f in factors]
        else:
            shape = tuple(Vshape)
            if len(shape) != 3:
                raise NotImplementedError(f'NTF factorises tensors of order 3, got order {len(shape)}')
            assert rank is not None and rank > 0, 'NTF needs a rank (or the factors)'
            data = [torch.randn(d, rank).abs() for d in shape]
        self.factors = nn.ParameterList([nn.Parameter(d, requires_grad=bool(t)) for d, t in zip(data, trainable)])
        self.rank = self.factors[0].shape[1]

    def forward(self) -> Tensor:
        """The reconstruction ``[I, J, K]`` (a ``torch.einsum`` on the factors; not the hot path, not differentiable through
        the HIP kernels -- ``fit`` never calls it)."""
        A, B, Cf = self.factors
        return torch.einsum('ir,jr,kr->ijk', A, B, Cf)

    def fit(self, V: Tensor, beta: float = 1, tol: float = 1e-4, max_iter: int = 200, verbose: bool = False, alpha: float = 0,
            l1_ratio: float = 0, weights=None, unstored: Optional[str] = None, tile: Optional[str] = None,
            solver: str = 'mu', precision: str = 'fp32', gram_rows: Optional[int] = None) -> int:
        """Fit the trainable factors to ``V`` by multiplicative updates: one iteration updates modes 0, 1, 2 in that order.
        Loss checkpoints and the stop rule are ``NMF.fit``'s (after iterations 9, 19, ...: stop when
        ``(previous - loss) / loss_init < tol``); returns the number of iterations.  ``weights``: None, or a dense tensor of
        ``V``'s shape (bool, integer or floating, >= 0); entries of weight 0 count for nothing whatever ``V`` holds there.
        ``alpha`` / ``l1_ratio`` regularise as in ``NMF.fit``.  Rank <= 256, exact fp32, device tensors only.  ``tile``: None --
        per mode the library's choice between the 128-row tile and the 32-row tile for short modes (at most 32 rows over a
        contraction of at least 65536) -- or 'wide' / 'short' for every mode; dense targets only.

        A 3-D sparse COO ``V`` (or a ``SparseNtfTarget``) is fitted over its stored entries when ``unstored`` says how to
        read the others: ``'missing'`` -- unknown (ratings, unsampled triples; every beta, beta <= 0 needs positive stored
        values), ``'zero'`` -- observed zeros (count tensors; beta in {1, 2}).  Nothing of the dense tensor's size exists.

        ``solver``: 'mu' (the multiplicative update), 'hals' or 'ccd'.  'hals' -- cyclic coordinate descent on the Frobenius objective
        (Cichocki & Phan 2009), beta = 2 only, dense unweighted targets and sparse ones with ``unstored='zero'``: a half-step is
        one MTTKRP of ``V`` (``ntf_mttkrp``, ``V`` read once, no reconstruction), two Gram matrices and one sweep over the
        rank (``hals.hals_sweep``); it reaches in a few iterations the loss MU needs hundreds for.  Before the first half-step
        the trainable factors are scaled once by the scalar that fits ``V`` best and clamped to >= eps; an MU fit can
        continue from the result.  The dense loss of a checkpoint comes from the last numerator and the Gram matrices
        (no pass over ``V``); it is a difference of numbers of the size of ``|V|^2`` and loses digits when the fit is
        nearly exact.  ``tile`` chooses the MTTKRP's wave arrangement as it chooses MU's tile.  'ccd' -- the same coordinate
        descent for a sparse target with ``unstored='missing'`` (beta = 2, no weights), where every owner row has its own
        quadratic: a half-step is one sweep over the stored entries with a maintained residual (``ntf_ccd_sweep``), at the
        order of one multiplicative half-step; the same once-only scale and clamp, over the stored entries.  A dense target
        or ``unstored='zero'`` has ``solver='hals'``.  ``gram_rows`` (``solver='ccd'`` only; None, the default, or an integer
        >= 0): the owner rows with more than ``gram_rows`` stored entries are updated through their own normal equations on
        an MFMA kernel that spreads a row over the whole device (``ntf_ccd_sweep(gram_rows=)``) -- for a mode of few, long rows
        (a context or channel mode), which the sweep leaves to as many workgroups as it has rows.  Those rows get other bits
        than the sweep's, the same minimiser; the other rows and the default are unchanged bit for bit.

        ``precision``: 'fp32' (exact fp32, the default) or 'bf16x3' -- ``solver='hals'`` on a dense target only: every MTTKRP
        of the fit (all modes, the initial scale's and the loss's) runs on the split-bf16 kernel (``ntf_mttkrp(...,
        precision='bf16x3')``, about 1.2e-5 relative per element); the Gram matrices and the sweep stay fp32.  The checkpoint
        loss inherits the numerator's error: it is already a difference of numbers of the size of ``|V|^2``, so its absolute
        error grows to about 1.2e-5 ``<V, Y>``."""
        if solver not in ('mu', 'hals', 'ccd'):
            raise ValueError(f"solver must be 'mu' or 'hals', or 'ccd' on a sparse target with unstored='missing'; got {solver!r}")
        if solver == 'ccd':
            if float(beta) != 2.0:
                raise NotImplementedError(f"solver='ccd' minimises the Frobenius objective over the stored entries: beta = 2, "
                                          f"got {float(beta):g}")
            if weights is not None:
                raise NotImplementedError("solver='ccd' takes no weights: the stored set of a sparse target is the mask; "
                                          "use solver='mu'")
            if unstored != 'missing':
                raise NotImplementedError("solver='ccd' fits the stored entries of a sparse target read with "
                                          "unstored='missing'; for a dense target or unstored='zero' use solver='hals'")
        if solver == 'hals':
            if float(beta) != 2.0:
                raise NotImplementedError(f"solver='hals' minimises the Frobenius objective: beta = 2, got {float(beta):g}")
            if weights is not None:
                raise NotImplementedError("solver='hals' takes no weights: every owner row would need its own Gram matrix; "
                                          "use solver='mu'")
            if unstored == 'missing':
                raise NotImplementedError("solver='hals' cannot read unstored entries as missing: every owner row would "
                                          "need its own Gram matrix; use solver='mu' or solver='ccd'")
        _check_gram_rows(gram_rows, 'NTF.fit')
        if gram_rows is not None and solver != 'ccd':
            raise NotImplementedError(f"gram_rows= is the normal-equations route of solver='ccd'; solver={solver!r} has none")
        _check_precision(precision)
        if precision != 'fp32':
            if solver != 'hals':
                raise NotImplementedError("precision='bf16x3' is the MTTKRP of solver='hals'; solver='mu' is exact fp32 only")
            if unstored is not None or isinstance(V, SparseNtfTarget) or (isinstance(V, Tensor) and V.is_sparse):
                raise NotImplementedError("precision='bf16x3' is the dense MTTKRP of solver='hals'; sparse targets are exact "
                                          "fp32 only")
        _check_tile(tile)
        if unstored is not None:
            if tile is not None:
                raise NotImplementedError('tile= chooses between the dense kernels; a sparse target has one kernel')
            return self._fit_sparse(V, float(beta), tol, max_iter, verbose, alpha, l1_ratio, weights, unstored, solver,
                                    gram_rows)
        if not isinstance(V, Tensor):
            raise ValueError(f'NTF.fit takes a dense 3-D tensor, got {type(V).__name__}')
        if V.is_sparse:
            raise NotImplementedError("NTF.fit takes a dense tensor; missing entries are given by weights=, and a sparse "
                                      "matrix is fitted over its stored entries by NMF.fit(..., unstored='missing').  A "
                                      "sparse 3-D tensor needs the keyword too: NTF.fit(V, unstored='missing' | 'zero')")
        if V.dim() != 3:
            raise NotImplementedError(f'NTF factorises tensors of order 3, got order {V.dim()}')
        if tuple(V.shape) != tuple(f.shape[0] for f in self.factors):
            raise ValueError(f'target {tuple(V.shape)} does not match the factors '
                             f'{tuple(f.shape[0] for f in self.factors)}')
        _check_shape(tuple(V.shape), self.rank)
        if weights is not None:
            weights = check_weights(V, weights)
        _require_device(V, 'NTF.fit')
        for f in self.factors:
            _require_device(f, 'NTF.fit')
        if any(f.dtype != torch.float32 for f in self.factors):
            # fitted on fp32 working copies and stored back in the module's dtype, as NMF.fit does
            if not all(f.dtype.is_floating_point for f in self.factors):
                raise NotImplementedError(f'factors must be floating point; got {[f.dtype for f in self.factors]}')
            keep = [f.data for f in self.factors]
            for f in self.factors:
                f.data = f.data.float().contiguous()
            try:
                return self.fit(V, beta, tol, max_iter, verbose, alpha, l1_ratio, weights, tile=tile, solver=solver,
                                precision=precision, gram_rows=gram_rows)
            finally:
                for f, k in zip(self.factors, keep):
                    f32, f.data = f.data, k
                    f.data.copy_(f32)
        beta = float(beta)
        step = (float(alpha * l1_ratio), float(alpha * (1 - l1_ratio)), mu_gamma(beta))     # nmf.py:348-349
        T = NtfTarget(V, weights, checked=True)
        assert not T.bad, "Target should be non-negative."
        if T.has_zero and beta <= 0:
            raise ValueError("When beta <= 0 and V contains zeros, the training process may diverge. "
                             "Please add small values to V, or use a positive beta value.")
        for f in self.factors:
            if not f.data.is_contiguous():
                f.data = f.data.contiguous()
        fs = [f.data for f in self.factors]
        if solver == 'hals':
            eng = _HalsNtf(T, fs, [f.requires_grad for f in self.factors], step[0], step[1], tile, precision)
            divergence, half_step = eng.divergence, eng.half_step
        else:
            lib, (I, J, K) = _capi.load(), T.shape
            r_pad = lib.nmfmu_pad_rank(self.rank)
            ws = torch.empty(max(_tile_entries(lib, tile, d, I * J * K // d, r_pad)[0](d, I * J * K // d, r_pad, 0)
                                 for d in T.shape), dtype=torch.float32, device=T.device)      # per mode by the tile that mode takes
            part = torch.empty(lib.nmfmu_ntf_loss_parts(I, J, K), dtype=torch.float64, device=T.device)
            out = torch.zeros(1, dtype=torch.float64, device=T.device)

            def divergence() -> float:
                return float(_ntf_loss(T, fs, beta, part, out).item())

            def half_step(mode: int) -> None:
                _ntf_call(T, fs, mode, beta, step=step, _ws=ws, tile=tile)

        loss_init = previous = _sqrt2(divergence())      # nmf.py:355-363
        pbar = None
        if verbose:
            from tqdm import tqdm
            pbar = tqdm(total=max_iter)
        n_iter = -1
        try:
            for n_iter in range(max_iter):
                for mode, f in enumerate(self.factors):
                    if f.requires_grad:
                        half_step(mode)
                if n_iter % 10 == 9:
                    loss = _sqrt2(divergence())
                    if pbar is not None:
                        pbar.set_postfix(loss=loss)
                        pbar.update(10)
                    if (previous - loss) / loss_init < tol:      # nmf.py:402-407
                        break
                    previous = loss
        finally:
            if pbar is not None:
                pbar.close()
        return n_iter + 1

    def _fit_sparse(self, V, beta, tol, max_iter, verbose, alpha, l1_ratio, weights, unstored, solver='mu',
                    gram_rows=None) -> int:
        """``fit`` on a sparse target: the refusals in their order, then ``fit``'s loop on ``nmfmu_sp_ntf_step``."""
        if unstored not in ('zero', 'missing'):
            raise ValueError(f"unstored must be 'zero' or 'missing', got {unstored!r}")
        if not isinstance(V, SparseNtfTarget) and not (isinstance(V, Tensor) and V.is_sparse):
            raise ValueError('unstored= reads a sparse COO target (or a SparseNtfTarget); a dense tensor stores every entry')
        _check_sparse(tuple(V.shape), list(self.factors), beta, unstored, weights)
        _require_device(V, 'NTF.fit')
        for f in self.factors:
            _require_device(f, 'NTF.fit')
        if any(f.dtype != torch.float32 for f in self.factors):
            # fitted on fp32 working copies and stored back in the module's dtype, as the dense fit does
            if not all(f.dtype.is_floating_point for f in self.factors):
                raise NotImplementedError(f'factors must be floating point; got {[f.dtype for f in self.factors]}')
            keep = [f.data for f in self.factors]
            for f in self.factors:
                f.data = f.data.float().contiguous()
            try:
                return self._fit_sparse(V, beta, tol, max_iter, verbose, alpha, l1_ratio, weights, unstored, solver,
                                        gram_rows)
            finally:
                for f, k in zip(self.factors, keep):
                    f32, f.data = f.data, k
                    f.data.copy_(f32)
        step = (float(alpha * l1_ratio), float(alpha * (1 - l1_ratio)), mu_gamma(beta))     # nmf.py:348-349
        T = V if isinstance(V, SparseNtfTarget) else SparseNtfTarget(V)
        assert not T.bad, "Target should be non-negative."
        if T.has_zero and beta <= 0:
            raise ValueError("When beta <= 0 and V contains zeros, the training process may diverge. "
                             "Please add small values to V, or use a positive beta value.")
        for f in self.factors:
            if not f.data.is_contiguous():
                f.data = f.data.contiguous()
        fs = [f.data for f in self.factors]
        if solver == 'hals':
            eng = _HalsNtf(T, fs, [f.requires_grad for f in self.factors], step[0], step[1])
            divergence, half_step = eng.divergence, eng.half_step
        elif solver == 'ccd':
            eng = _CcdNtf(T, fs, [f.requires_grad for f in self.factors], step[0], step[1], gram_rows)
            divergence, half_step = eng.divergence, eng.half_step
        else:
            lib = _capi.load()
            r_pad = lib.nmfmu_pad_rank(self.rank)
            ws = torch.empty(max(1, *(lib.nmfmu_sp_ntf_ws(m['n_ws'], r_pad) for m in T.modes)), dtype=torch.float32,
                             device=T.device)
            part = torch.empty((T.modes[0]['seg'].shape[0] + 3) // 4, dtype=torch.float64, device=T.device)
            out = torch.zeros(1, dtype=torch.float64, device=T.device)

            def divergence() -> float:
                return float(_sparse_loss(T, fs, beta, unstored, part=part, out=out).item())

            def half_step(mode: int) -> None:
                _sparse_call(T, fs, mode, beta, unstored, step=step, _ws=ws)

        loss_init = previous = _sqrt2(divergence())      # nmf.py:355-363
        pbar = None
        if verbose:
            from tqdm import tqdm
            pbar = tqdm(total=max_iter)
        n_iter = -1
        try:
            for n_iter in range(max_iter):
                for mode, f in enumerate(self.factors):
                    if f.requires_grad:
                        half_step(mode)
                if n_iter % 10 == 9:
                    loss = _sqrt2(divergence())
                    if pbar is not None:
                        pbar.set_postfix(loss=loss)
                        pbar.update(10)
                    if (previous - loss) / loss_init < tol:      # nmf.py:402-407
                        break
                    previous = loss
        finally:
            if pbar is not None:
                pbar.close()
        return n_iter + 1
