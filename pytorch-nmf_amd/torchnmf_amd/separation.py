"""Source separation with a fitted model: per-group soft masks, optionally times the mixture.

``separate(H, W, V=None, groups=None, *, power=1.0, select=None)`` splits the rank into groups of components (one per source or
instrument; by default every component alone) and returns, stacked along a new first axis, for every selected group ``g``

    mask_g = Y_g^p / (sum_g' Y_g'^p + eps)          Y_g = reconstruct(H[:, idx_g], W[:, idx_g]),  p = power

or ``V * mask_g`` when the mixture ``V`` is given (real, or the ``complex64`` STFT: the real mask multiplies both parts).  For
``p == 1`` the denominator is the one reconstruction over all components.  ``W.dim() == 2`` is an ``NMF`` model (``H (N, R)``,
``W (C, R)``, planes ``(N, C)``); ``W.dim()`` in 3 .. 5 is ``NMFD / NMF2D / NMF3D`` (``H (B, R, *Lh)``, ``W (C, R, *T)``, planes
``(B, C, *L)``).

Two routes:

* ``'fused'`` -- dense models up to rank 256: one exact-fp32 MFMA kernel (``nmfmu_separate``) forms every ``Y_g`` and the
  denominator in registers and writes the output planes; nothing else of size ``N x C`` exists.
* ``'planes'`` -- every model: one ``reconstruct`` per non-empty group into the stacked buffer that becomes the output, then one
  elementwise kernel (``nmfmu_separate_planes``) in place; ``power == 1`` adds one plane for the denominator.  With a
  ``select`` that is not the identity only the ``S`` output planes, the denominator and one scratch plane exist.

The result is detached; there is no autograd here.  The argument checks run before any device work, in the order of
``_check_args``.  The factors' signs are not scanned.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from collections.abc import Sequence

import torch
from torch import Tensor

from . import _capi
from .constants import eps as _EPS

MAX_FUSED_RANK = 256          # csrc/nmfmu_separate.hip: kSepMaxRank
V_NONE, V_REAL, V_COMPLEX = 0, 1, 2


# ---- host tables (plain Python; tests/separate_emulation.py restates them) --------------------------------------------------------
def normalise_groups(groups, R: int) -> list:
    """The length-``R`` list of labels >= 0.  ``None``: every component its own group."""
    if groups is None:
        return list(range(R))
    if isinstance(groups, Tensor):
        if groups.dtype.is_floating_point or groups.dtype.is_complex or groups.dtype == torch.bool or groups.dim() != 1:
            raise TypeError(f'separate: groups must be a sequence or a 1-D integer tensor of labels, got {groups.dtype} '
                            f'with {groups.dim()} dimensions')
        labels = [int(x) for x in groups.tolist()]
    elif isinstance(groups, Sequence) and not isinstance(groups, (str, bytes)):
        labels = []
        for x in groups:
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise TypeError(f'separate: groups must hold integer labels, got {x!r}')
            labels.append(int(x))
    else:
        raise TypeError(f'separate: groups must be None, a sequence or a 1-D integer tensor, got {type(groups).__name__}')
    if len(labels) != R:
        raise ValueError(f'separate: groups has {len(labels)} labels for rank {R}')
    if labels and min(labels) < 0:
        raise ValueError(f'separate: group labels must be >= 0, got {min(labels)}')
    return labels


def group_tables(labels: list):
    """``(G, members, cols, gstart)``: the number of groups ``max + 1``; per group the component indices in their original
    order (the stable sort by label); ``cols`` [R'] the component behind every column of the permuted factors, -1 for a zero
    column that pads a group to an even count; ``gstart`` [G + 1] the groups' first columns (even, ascending)."""
    G = max(labels) + 1
    members = [[] for _ in range(G)]
    for r, g in enumerate(labels):
        members[g].append(r)
    cols, gstart = [], [0]
    for m in members:
        cols.extend(m)
        if len(m) & 1:
            cols.append(-1)
        gstart.append(len(cols))
    return G, members, cols, gstart


def slot_table(G: int, select) -> tuple:
    """``(slot [G], S, copies)``: the output plane of every group (-1: none; the first position of the group in ``select``),
    the number of planes, and ``(dst, src)`` for every repeated entry of ``select``."""
    if select is None:
        return list(range(G)), G, []
    slot, copies = [-1] * G, []
    for s, g in enumerate(select):
        if slot[g] < 0:
            slot[g] = s
        else:
            copies.append((s, slot[g]))
    return slot, len(select), copies


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def _check_power(power) -> float:
    if isinstance(power, bool) or not isinstance(power, numbers.Real):
        raise TypeError(f'separate: power must be a real number, got {power!r}')
    p = float(power)
    if math.isnan(p) or p <= 0 or math.isinf(p):
        raise ValueError(f'separate: power must be a finite number > 0, got {power!r}')
    return ctypes.c_float(p).value          # the fp32 value the kernels compute with


def _check_select(select, G: int):
    if select is None:
        return None
    if isinstance(select, Tensor):
        if select.dtype.is_floating_point or select.dtype.is_complex or select.dtype == torch.bool or select.dim() != 1:
            raise TypeError('separate: select must be a sequence or a 1-D integer tensor of group indices')
        sel = [int(x) for x in select.tolist()]
    elif isinstance(select, Sequence) and not isinstance(select, (str, bytes)):
        sel = []
        for x in select:
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise TypeError(f'separate: select must hold integer group indices, got {x!r}')
            sel.append(int(x))
    else:
        raise TypeError(f'separate: select must be None, a sequence or a 1-D integer tensor, got {type(select).__name__}')
    for g in sel:
        if not 0 <= g < G:
            raise IndexError(f'separate: select holds group {g}, outside [0, {G})')
    return sel


def _target_shape(H: Tensor, W: Tensor) -> tuple:
    if W.dim() == 2:
        if not (H.dim() == 2 and H.shape[1] == W.shape[1] and min(tuple(H.shape) + tuple(W.shape)) > 0):
            raise ValueError('separate: a dense model needs H (N, R) and W (C, R) with N, C, R >= 1, got '
                             f'{tuple(H.shape)} and {tuple(W.shape)}')
        if max(H.shape[0], W.shape[0]) >= 2 ** 31:
            raise ValueError('separate: N and C must be below 2^31')
        return (H.shape[0], W.shape[0])
    if not (3 <= W.dim() <= 5 and H.dim() == W.dim() and H.shape[1] == W.shape[1]
            and min(tuple(H.shape) + tuple(W.shape)) > 0):
        raise ValueError('separate: a convolutive model needs H (B, R, *Lh) and W (C, R, *T) with one to three shift axes, got '
                         f'{tuple(H.shape)} and {tuple(W.shape)}')
    return (H.shape[0], W.shape[0]) + tuple(lh + t - 1 for lh, t in zip(H.shape[2:], W.shape[2:]))


def _check_args(H, W, V, groups, power, select, route):
    """Cheapest first; nothing here touches the device (a ``groups`` / ``select`` given as a device tensor is read back)."""
    R = W.shape[1] if isinstance(W, Tensor) and W.dim() >= 2 else (H.shape[1] if isinstance(H, Tensor) and H.dim() >= 2 else None)
    if R is not None or groups is not None:
        labels = normalise_groups(groups, R if R is not None else len(groups))
    else:
        labels = None
    p = _check_power(power)
    G = max(labels) + 1 if labels else 0
    sel = _check_select(select, G)
    if route not in (None, 'fused', 'planes'):
        raise ValueError(f"separate: _route must be None, 'fused' or 'planes', got {route!r}")
    if not (isinstance(H, Tensor) and isinstance(W, Tensor)):
        raise ValueError('separate: H and W must be tensors')
    if W.dim() < 2 or H.dim() < 2:
        raise ValueError(f'separate: H and W need a rank axis, got {tuple(H.shape)} and {tuple(W.shape)}')
    shape = _target_shape(H, W)
    if V is not None:
        if not isinstance(V, Tensor) or tuple(V.shape) != shape:
            got = tuple(V.shape) if isinstance(V, Tensor) else type(V).__name__
            raise ValueError(f'separate: V must be a tensor of the target shape {shape}, got {got}')
        if not (V.dtype.is_floating_point or V.dtype == torch.complex64):
            raise TypeError(f'separate: V must be real floating point or complex64, got {V.dtype}')
    for t in (H, W, V):
        if t is not None and t.device.type != 'cuda':
            raise _capi.NmfmuError('separate: tensors must live on the ROCm device (no CPU fallback)')
    devs = {t.device for t in (H, W, V) if t is not None}
    if len(devs) > 1:
        raise _capi.NmfmuError(f'separate: tensors must live on the same device, got {sorted(map(str, devs))}')
    if not (H.dtype.is_floating_point and W.dtype.is_floating_point):
        raise TypeError(f'separate: factors must be floating point; got H {H.dtype}, W {W.dtype}')
    if route == 'fused' and (W.dim() != 2 or W.shape[1] > MAX_FUSED_RANK or G > MAX_FUSED_RANK):
        raise NotImplementedError(f"separate: the fused route serves dense models up to rank {MAX_FUSED_RANK} with at most "
                                  f"{MAX_FUSED_RANK} groups (empty ones included)")
    return labels, p, sel, shape


def choose_route(dense: bool, G: int, R: int, power: float = 1.0, kind: int = V_NONE, identity: bool = True) -> str:
    """The library's route.  Convolutive models, dense ranks above ``MAX_FUSED_RANK`` and more than ``MAX_FUSED_RANK`` groups
    (labels may leave any number of empty ones) go by planes: the fused kernel does not hold them.  For the others the
    fused kernel is the choice wherever it was not measured to lose (profiles/separate.json, rank 128):
    it walks the rank twice whatever ``G`` is, the planes route walks it once and pays about three more passes over HBM per
    plane, and with a real mixture, ``power != 1`` and all planes wanted the planes were faster up to ``G = 4``.  At
    ``power == 1`` they tie at ``G = 2`` and lose above, and they hold one more plane, so fused it is; with a complex mixture
    fused is faster everywhere; masks without a mixture were not measured and go fused.  That the crossover scales with
    ``R`` follows from the cost model, not from a measurement."""
    if not dense or R > MAX_FUSED_RANK or G > MAX_FUSED_RANK:
        return 'planes'
    if kind != V_REAL or not identity or power == 1.0:
        return 'fused'
    return 'planes' if G * 32 <= R else 'fused'


# ---- device work ------------------------------------------------------------------------------------------------------------------
def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _i32_array(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def _mixture(V):
    """(fp32 tensor the kernels read, its kind): a real target converted once, a complex one viewed as interleaved floats."""
    if V is None:
        return None, V_NONE
    if V.dtype == torch.complex64:
        return torch.view_as_real(V.detach().contiguous()), V_COMPLEX
    return V.detach().float().contiguous(), V_REAL


def _new_planes(S: int, shape: tuple, kind: int, dev) -> Tensor:
    return torch.empty((S,) + shape, dtype=torch.complex64 if kind == V_COMPLEX else torch.float32, device=dev)


def _floats(t: Tensor) -> Tensor:
    return torch.view_as_real(t) if t.is_complex() else t


def _fused(H, W, Vf, kind, labels, p, sel, shape, fill):
    lib = _capi.load()
    dev = H.device
    N, C = shape
    R = W.shape[1]
    G, _, cols, gstart = group_tables(labels)
    slot, S, copies = slot_table(G, sel)
    out = _new_planes(S, shape, kind, dev)
    if fill is not None:
        _floats(out).fill_(fill)
    if S == 0:
        return out
    # the permuted, padded factors: column R of the widened copy is the zero column
    idx = torch.tensor([R if c < 0 else c for c in cols], dtype=torch.int64, device=dev)
    Hc, Wc = H.detach().float(), W.detach().float()
    Hp = torch.cat([Hc, Hc.new_zeros(N, 1)], 1).index_select(1, idx).contiguous()
    Wp = torch.cat([Wc, Wc.new_zeros(C, 1)], 1).index_select(1, idx).contiguous()
    tables = torch.tensor(gstart + slot, dtype=torch.int32, device=dev)       # the kernel's copy of both tables
    assert tables.numel() * 4 == lib.nmfmu_separate_tables_bytes(G)
    _capi.check(lib.nmfmu_separate(Hp.data_ptr(), N, Wp.data_ptr(), C, len(cols), _i32_array(gstart), _i32_array(slot), G, S,
                                   tables.data_ptr(), Vf.data_ptr() if Vf is not None else None, kind, C, p, _EPS,
                                   out.data_ptr(), C, _stream()), 'nmfmu_separate')
    for dst, src in copies:
        out[dst].copy_(out[src])
    return out


def _reconstruct_into(dst: Tensor, Hs: Tensor, Ws: Tensor) -> None:
    """``dst`` (the target shape, any strides) = reconstruct(Hs, Ws); a dense model writes a contiguous plane directly."""
    if Ws.dim() == 2:
        if dst.is_contiguous():
            _capi.check(_capi.load().nmfmu_reconstruct(Hs.data_ptr(), Hs.shape[0], Ws.data_ptr(), Ws.shape[0], Hs.shape[1],
                                                       dst.data_ptr(), dst.stride(0), _stream()), 'nmfmu_reconstruct')
            return
        from .nmf import _reconstruct_forward
        dst.copy_(_reconstruct_forward(Hs, Ws))
        return
    from .nmfd_engine import reconstruct
    dst.copy_(reconstruct(Hs, Ws))


def _planes_kernel(ys0, G, y_stride, y_elem, dplane, Vf, kind, n, p, slot, S, out_ptr) -> None:
    slot_dev = torch.tensor(slot, dtype=torch.int32, device=ys0.device)
    _capi.check(_capi.load().nmfmu_separate_planes(ys0.data_ptr(), G, y_stride, y_elem,
                                                   dplane.data_ptr() if dplane is not None else None,
                                                   Vf.data_ptr() if Vf is not None else None, kind, n, p, _EPS,
                                                   _i32_array(slot), S, slot_dev.data_ptr(), out_ptr, n, _stream()),
                'nmfmu_separate_planes')


def _sub_factors(Hc, Wc, idx):
    it = torch.tensor(idx, dtype=torch.int64, device=Hc.device)
    return Hc.index_select(1, it).contiguous(), Wc.index_select(1, it).contiguous()


def _planes(H, W, Vf, kind, labels, p, sel, shape, fill):
    dev = H.device
    n = math.prod(shape)
    G, members, _, _ = group_tables(labels)
    slot, S, copies = slot_table(G, sel)
    if S == 0:
        return _new_planes(0, shape, kind, dev)
    Hc, Wc = H.detach().float().contiguous(), W.detach().float().contiguous()
    if sel is None or sel == list(range(G)):
        out = _planes_all(Hc, Wc, Vf, kind, G, members, p, shape, n, fill)
    else:
        out = _planes_selected(Hc, Wc, Vf, kind, G, members, p, slot, S, shape, n, fill)
    for dst, src in copies:
        out[dst].copy_(out[src])
    return out


def _planes_all(Hc, Wc, Vf, kind, G, members, p, shape, n, fill):
    """Every plane in order: the stacked reconstructions become the output in place."""
    dev = Hc.device
    given_d = p == 1.0                        # the denominator is the one reconstruction over all components
    if kind != V_COMPLEX:
        buf = torch.empty((G + int(given_d),) + shape, dtype=torch.float32, device=dev)     # one more plane for a given D
        out, ys, y_elem, y_stride = buf[:G], [buf[g] for g in range(G)], 1, n
        dplane = buf[G] if given_d else None
    else:
        # complex planes: the reconstructions sit in the real slots of the output
        out = _new_planes(G, shape, kind, dev)
        real = torch.view_as_real(out)
        ys, y_elem, y_stride = [real[g][..., 0] for g in range(G)], 2, 2 * n
        dplane = torch.empty(shape, dtype=torch.float32, device=dev) if given_d else None
    if fill is not None:
        _floats(out).fill_(fill)
        if dplane is not None:
            dplane.fill_(fill)
    for g, idx in enumerate(members):
        if idx:
            _reconstruct_into(ys[g], *_sub_factors(Hc, Wc, idx))
        else:
            ys[g].zero_()
    if given_d:
        _reconstruct_into(dplane, Hc, Wc)
    _planes_kernel(ys[0], G, y_stride, y_elem, dplane, Vf, kind, n, p, list(range(G)), G, out.data_ptr())
    return out


def _planes_selected(Hc, Wc, Vf, kind, G, members, p, slot, S, shape, n, fill):
    """A ``select`` other than the identity: the ``S`` output planes, one plane for the denominator and (``power != 1``) one
    scratch plane that every unselected group's reconstruction passes through.  ``power == 1``: D is the full reconstruction
    and only the selected groups are reconstructed.  Otherwise D is accumulated plane by plane in ascending g by
    ``nmfmu_separate_accumulate`` -- the very operation the kernels sum with, so a plane has the bits of the identity call."""
    lib = _capi.load()
    dev = Hc.device
    out = _new_planes(S, shape, kind, dev)
    dplane = torch.empty(shape, dtype=torch.float32, device=dev)
    if fill is not None:
        _floats(out).fill_(fill)
        dplane.fill_(fill)
    y_elem = 2 if kind == V_COMPLEX else 1

    def target(g):            # where the reconstruction of a selected group goes: its output plane (the real slots of it)
        return torch.view_as_real(out[slot[g]])[..., 0] if kind == V_COMPLEX else out[slot[g]]

    if p == 1.0:
        _reconstruct_into(dplane, Hc, Wc)
        for g, idx in enumerate(members):
            if slot[g] >= 0:
                if idx:
                    _reconstruct_into(target(g), *_sub_factors(Hc, Wc, idx))
                else:
                    target(g).zero_()
    else:
        dplane.zero_()
        scratch = None
        for g, idx in enumerate(members):
            if not idx:               # y = 0 adds exactly nothing to D
                if slot[g] >= 0:
                    target(g).zero_()
                continue
            if slot[g] >= 0:
                y, ye = target(g), y_elem
            else:
                if scratch is None:
                    scratch = torch.empty(shape, dtype=torch.float32, device=dev)
                y, ye = scratch, 1
            _reconstruct_into(y, *_sub_factors(Hc, Wc, idx))
            _capi.check(lib.nmfmu_separate_accumulate(y.data_ptr(), ye, n, p, dplane.data_ptr(), _stream()),
                        'nmfmu_separate_accumulate')
    for g in range(G):
        if slot[g] >= 0:          # one plane at a time, in place, with the denominator given
            _planes_kernel(target(g), 1, y_elem * n, y_elem, dplane, Vf, kind, n, p, [0], 1, out[slot[g]].data_ptr())
    return out


def separate(H: Tensor, W: Tensor, V: Tensor = None, groups=None, *, power=1.0, select=None, _route=None) -> Tensor:
    """``[S, *target shape]``: the soft masks of the selected groups (``V=None``, fp32) or the mixture times them (fp32 for a
    real ``V`` of any floating dtype, ``complex64`` for a ``complex64`` ``V``).

    ``groups``: ``None`` (every component alone, ``G = R``) or ``R`` integer labels >= 0, in any order; ``G = max + 1``, and a
    label no component carries is an empty group whose plane is exactly zero.  ``power``: a real ``p > 0`` (1 and 2 need no
    transcendental).  ``select``: ``None`` for all ``G`` planes in order, or group indices -- order and repeats are honoured,
    the denominator still runs over all groups, and a plane's bits do not depend on it.  Where every ``Y_g`` is zero the mask
    is exactly 0.  ``V`` is only multiplied: it need not be non-negative, and a NaN in it stays in its own element.  A
    repeated call is bitwise identical.

    ``_route`` (tests and the benchmark): ``'fused'`` or ``'planes'`` instead of ``choose_route``."""
    return _separate(H, W, V, groups, power, select, _route, None)


def _separate(H, W, V, groups, power, select, route, fill):
    """``separate``; ``fill`` (the tests) pre-fills everything the kernels are to write."""
    labels, p, sel, shape = _check_args(H, W, V, groups, power, select, route)
    dense = W.dim() == 2
    Vf, kind = _mixture(V)
    G = max(labels) + 1
    if route is None:
        route = choose_route(dense, G, W.shape[1], p, kind, sel is None or sel == list(range(G)))
    with torch.no_grad():
        return (_fused if route == 'fused' else _planes)(H, W, Vf, kind, labels, p, sel, shape, fill)
