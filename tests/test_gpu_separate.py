"""``separation.separate`` per element on the device: the fused dense kernel (``nmfmu_separate``), the planes kernel
(``nmfmu_separate_planes``) through the C ABI, both routes against each other, the convolutive models, golden g26 and the module
method.  References and bounds are tests/separate_emulation.py's (its docstring derives the bound from the kernels' operation
order; tests/test_separate_emulation.py shows on the CPU that a seeded fault fails it).  Every element of every output is
compared; outputs start as NaN.

Worst error / bound per family is written with ``conftest.record`` (recorded, not used to set a bound); DESIGN.md section 33
holds the figures of the first MI355X run.
"""
import ctypes

import numpy as np
import pytest
import torch

import forward_reference as FR
import separate_emulation as SE
from conftest import load_golden, record
from test_gpu_conv_autograd import SHAPES_1D, SHAPES_2D, SHAPES_3D

pytestmark = pytest.mark.gpu

NAN = float('nan')
POWERS = [1.0, 2.0, 0.5, 1.7]
MIXTURES = ['none', 'real', 'complex']
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    yield torch.device('cuda:0')
    for family, w in sorted(_worst.items()):
        record('separate', family=family, worst_fraction_of_bound=w)
        print(f'separate {family}: worst |got - ref| / bound = {w:.3f}')


def separate(H, W, V=None, groups=None, *, power=1.0, select=None, _route=None, _fill=None):
    """``separation.separate`` with everything the kernels are to write pre-filled (the private entry the public one wraps)."""
    from torchnmf_amd.separation import _separate
    return _separate(H, W, V, groups, power, select, _route, _fill)


def _note(family, w):
    _worst[family] = max(_worst.get(family, 0.0), w)


def _labels(kind, R):
    """(labels or None, components whose H columns are zeroed)."""
    if kind == 'none':
        return None, []
    if kind == 'two_odd':                      # 3 + 4 of 7, 17 + 19 of 36
        k = (R // 2) | 1 if (R // 2) % 2 == 0 else R // 2
        return [0] * k + [1] * (R - k), []
    if kind == 'interleaved':
        return [r % 3 for r in range(R)], []
    if kind == 'empty':                        # label 1 is carried by no component
        return [(0, 2, 3)[r % 3] for r in range(R)], []
    if kind == 'zero_group':                   # every component of group 1 is silent
        lab = [r % 3 for r in range(R)]
        return lab, [r for r in range(R) if lab[r] == 1]
    raise KeyError(kind)


def _mixture(kind, shape, seed=0):
    g = torch.Generator().manual_seed(1234 + seed)
    if kind == 'none':
        return None
    if kind == 'complex':
        return torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    V = torch.randn(shape, generator=g)          # negatives; then zeros and one NaN
    flat = V.view(-1)
    flat[::7] = 0.0
    flat[flat.numel() // 2] = NAN
    return V


FUSED_CASES = ([((1, 1, 1), 'none')]
               + [((131, 70, 7), k) for k in ('none', 'two_odd', 'interleaved', 'empty', 'zero_group')]
               + [((129, 127, 36), k) for k in ('none', 'two_odd', 'interleaved', 'empty')]
               + [((257, 129, 64), k) for k in ('none', 'interleaved')]
               + [((200, 90, 256), 'none')])
_ids = lambda s: '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in s)

_factor_cache = {}


def _dense_case(shape, grouping):
    key = (shape, grouping)
    if key not in _factor_cache:
        H, W = FR.dense_factors(shape)
        labels, silent = _labels(grouping, shape[2])
        if silent:
            H = H.clone()
            H[:, silent] = 0.0
        _factor_cache[key] = (H, W, labels)
    return _factor_cache[key]


_ref_cache = {}


def _reference(key, H, W, V, labels, power):
    """The float64 reference of a case, computed once and shared by the tests that need it."""
    if key not in _ref_cache:
        _ref_cache[key] = SE.emulate(H.numpy(), W.numpy(), None if V is None else V.numpy(), labels, power)
    return _ref_cache[key]


# ---- the fused kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mix', MIXTURES)
@pytest.mark.parametrize('power', POWERS)
@pytest.mark.parametrize('case', FUSED_CASES, ids=_ids)
def test_fused_per_element(dev, case, power, mix):
    shape, grouping = case
    H, W, labels = _dense_case(shape, grouping)
    V = _mixture(mix, shape[:2])
    out = separate(H.to(dev), W.to(dev), None if V is None else V.to(dev), labels, power=power, _route='fused', _fill=NAN)
    G = shape[2] if labels is None else max(labels) + 1
    assert out.shape == (G,) + shape[:2] and out.is_contiguous() and not out.requires_grad
    assert out.dtype == (torch.complex64 if mix == 'complex' else torch.float32)
    ref, bound = _reference((case, power, mix), H, W, V, labels, power)
    w = SE.check(out.cpu().numpy(), ref, bound, f'fused {case} p={power} {mix}')
    _note(f'fused p={power:g}', w)
    got = out.cpu()
    if grouping == 'empty':
        assert not torch.view_as_real(got[1]).any() if mix == 'complex' else not got[1][~torch.isnan(got[1])].any()
    if grouping == 'zero_group' and mix == 'none':
        assert not got[1].any()


@pytest.mark.parametrize('mix', MIXTURES)
@pytest.mark.parametrize('power', POWERS)
def test_fused_select_and_repeat_are_bitwise(dev, power, mix):
    shape = (129, 127, 36)
    H, W, labels = _dense_case(shape, 'interleaved')
    V = _mixture(mix, shape[:2])
    Hd, Wd, Vd = H.to(dev), W.to(dev), None if V is None else V.to(dev)
    bits = lambda t: torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)
    full = separate(Hd, Wd, Vd, labels, power=power, _route='fused', _fill=NAN)
    again = separate(Hd, Wd, Vd, labels, power=power, _route='fused', _fill=NAN)
    assert torch.equal(bits(full), bits(again))
    part = separate(Hd, Wd, Vd, labels, power=power, select=[2, 0], _route='fused', _fill=NAN)
    assert part.shape[0] == 2 and torch.equal(bits(part), bits(full[[2, 0]]))
    rep = separate(Hd, Wd, Vd, labels, power=power, select=torch.tensor([1, 1, 2, 1]), _route='fused', _fill=NAN)
    assert torch.equal(bits(rep), bits(full[[1, 1, 2, 1]]))
    assert separate(Hd, Wd, Vd, labels, power=power, select=[], _route='fused').shape == (0, 129, 127)


@pytest.mark.parametrize('power', POWERS)
def test_all_zero_elements_are_exactly_zero(dev, power):
    """Row N // 2 of H and row C // 3 of W are zero: every Y_g vanishes there, and the mask is 0, never NaN."""
    shape = (131, 70, 7)
    H, W = FR.dense_factors(shape, 'zeros')
    for route in ('fused', 'planes'):
        out = separate(H.to(dev), W.to(dev), None, [0, 1, 0, 2, 1, 2, 0], power=power, _route=route, _fill=NAN).cpu()
        zero = torch.zeros(131, 70, dtype=torch.bool)
        zero[131 // 2] = True
        zero[:, 70 // 3] = True
        assert torch.isfinite(out).all()
        assert torch.equal(out == 0, zero.expand(3, -1, -1))


def test_other_floating_dtypes_are_converted_once(dev):
    shape = (131, 70, 7)
    H, W, labels = _dense_case(shape, 'two_odd')
    V = _mixture('real', shape[:2]).half()
    a = separate(H.to(dev), W.to(dev), V.to(dev), labels, power=2.0)
    b = separate(H.to(dev).double(), W.to(dev).double(), V.float().to(dev), labels, power=2.0)
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the planes kernel through the C ABI -------------------------------------------------------------------------------------------
def _run_planes(dev, Y, V, power, layout, D=None, select=None):
    """Y [G, n] fp32 CPU planes -> the output [S, n] of nmfmu_separate_planes in the given memory layout."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    G, n = Y.shape
    kind = 0 if V is None else (2 if V.is_complex() else 1)
    vw = 2 if kind == 2 else 1
    slot, S, _ = SE.slots(G, select)
    Vd = None if V is None else (torch.view_as_real(V.to(dev).contiguous()) if kind == 2 else V.to(dev).contiguous())
    if layout == 'inplace':
        assert select is None
        if kind == 2:
            out = torch.full((G, n, 2), NAN, device=dev)
            out[:, :, 0] = Y.to(dev)
            yt, y_stride, y_elem = out, 2 * n, 2
        else:
            out = Y.to(dev).clone()
            yt, y_stride, y_elem = out, n, 1
        ot, o_stride, res = out, n, out
    else:
        # 'outplace': strides rounded up to four floats, so the 16-byte accesses run and n % 4 elements are left to the scalar
        # tail; 'misaligned': a stride and a base that break 16-byte alignment
        pad = 1 if layout == 'misaligned' else 0
        n4 = -(-n // 4) * 4
        y_stride, y_elem = (n + 1, 1) if pad else (n4, 1)
        o_stride = n + 3 if pad else n4
        ybuf = torch.full((G * y_stride + pad,), NAN, device=dev)
        yt = ybuf[pad:]
        yt[:G * y_stride].view(G, y_stride)[:, :n] = Y.to(dev)
        obuf = torch.full((S * o_stride * vw + 2 * pad,), NAN, device=dev)
        ot = obuf[2 * pad:]
        res = ot[:S * o_stride * vw].view(S, o_stride, vw)[:, :n]
    Dd = None if D is None else D.to(dev).contiguous()
    slot_dev = torch.tensor(slot, dtype=torch.int32, device=dev)
    code = lib.nmfmu_separate_planes(yt.data_ptr(), G, y_stride, y_elem, Dd.data_ptr() if Dd is not None else None,
                                     Vd.data_ptr() if Vd is not None else None, kind, n, power, SE.EPS,
                                     (ctypes.c_int32 * G)(*slot), S, slot_dev.data_ptr(), ot.data_ptr(), o_stride,
                                     torch.cuda.current_stream().cuda_stream)
    _capi.check(code, 'nmfmu_separate_planes')
    torch.cuda.synchronize()
    if layout != 'inplace':
        # nothing outside the planes' elements was written
        tail = ot[:S * o_stride * vw].view(S, o_stride, vw)[:, n:]
        assert torch.isnan(tail).all() and torch.isnan(obuf[:2 * pad]).all()
        assert torch.isnan(ybuf[:pad]).all()
    res = res.cpu()
    if kind == 2:
        return torch.view_as_complex(res.reshape(S, n, 2).contiguous())
    return res.reshape(S, n)


def _planes_input(G, n):
    g = torch.Generator().manual_seed(G * 31 + n)
    Y = torch.rand(G, n, generator=g) * 3
    Y.view(-1)[::5] = 0.0
    if n > 3:
        Y[:, 3] = 0.0              # an element where every plane is zero
    return Y


@pytest.mark.parametrize('mix', ['real', 'complex'])
@pytest.mark.parametrize('power', POWERS)
@pytest.mark.parametrize('layout', ['inplace', 'outplace', 'misaligned'])
@pytest.mark.parametrize('n', [1, 1027, 1028])      # 1028: 16-byte accesses in place
@pytest.mark.parametrize('G', [1, 2, 3, 7])
def test_planes_kernel_per_element(dev, G, n, layout, power, mix):
    Y = _planes_input(G, n)
    V = _mixture(mix, (n,), seed=G)
    got = _run_planes(dev, Y, V, power, layout)
    ref, bound = SE.from_planes(Y.numpy(), V.numpy(), power)
    _note(f'planes kernel p={power:g}', SE.check(got.numpy(), ref, bound, f'planes G={G} n={n} {layout} p={power} {mix}'))
    if n > 3:
        z = got[:, 3]
        assert not (torch.view_as_real(z).any() if z.is_complex() else z.any())


@pytest.mark.parametrize('layout', ['outplace', 'misaligned'])
def test_planes_kernel_masks_select_and_given_denominator(dev, layout):
    Y = _planes_input(3, 1027)
    full = _run_planes(dev, Y, None, 1.7, layout)
    ref, bound = SE.from_planes(Y.numpy(), None, 1.7)
    SE.check(full.numpy(), ref, bound, 'planes masks')
    part = _run_planes(dev, Y, None, 1.7, layout, select=[2, 0])
    assert torch.equal(part.view(torch.int32), full[[2, 0]].view(torch.int32))
    D = Y.sum(0) * 1.5 + 0.25
    got = _run_planes(dev, Y, None, 1.0, layout, D=D)
    ref, bound = SE.from_planes(Y.numpy(), None, 1.0, D=D.numpy())
    SE.check(got.numpy(), ref, bound, 'planes with a given denominator')


# ---- routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mix', MIXTURES)
@pytest.mark.parametrize('power', POWERS)
def test_routes_agree(dev, power, mix):
    case = ((129, 127, 36), 'interleaved')
    H, W, labels = _dense_case(*case)
    V = _mixture(mix, (129, 127))
    Hd, Wd, Vd = H.to(dev), W.to(dev), None if V is None else V.to(dev)
    ref, bound = _reference((case, power, mix), H, W, V, labels, power)
    a = separate(Hd, Wd, Vd, labels, power=power, _route='fused', _fill=NAN).cpu().numpy()
    b = separate(Hd, Wd, Vd, labels, power=power, _route='planes', _fill=NAN).cpu().numpy()
    _note(f'planes route p={power:g}', SE.check(b, ref, bound, f'planes route p={power} {mix}'))
    # each is within its bound of the float64 reference, so they are within the sum of their bounds of each other
    SE.check(a, np.where(np.isnan(b), ref, b), 2 * bound, 'fused against planes')
    sel = separate(Hd, Wd, Vd, labels, power=power, select=[2, 0, 2], _route='planes', _fill=NAN).cpu().numpy()
    SE.check(sel, ref[[2, 0, 2]], bound[[2, 0, 2]], f'planes route with select p={power} {mix}')


def test_rank_above_the_fused_limit_takes_the_planes_route(dev):
    from torchnmf_amd.separation import choose_route
    shape = (40, 50, 260)
    H, W = FR.dense_factors(shape)
    labels = [r % 2 for r in range(260)]
    assert choose_route(True, 2, 260, 2.0) == 'planes'
    out = separate(H.to(dev), W.to(dev), None, labels, power=2.0, _fill=NAN)
    ref, bound = SE.emulate(H.numpy(), W.numpy(), None, labels, 2.0)
    SE.check(out.cpu().numpy(), ref, bound, 'rank 260')
    with pytest.raises(NotImplementedError):
        separate(H.to(dev), W.to(dev), None, labels, _route='fused')


def test_more_groups_than_the_fused_kernel_holds(dev):
    """Labels up to 300 on a rank-7 model: 301 groups, 294 of them empty.  The library goes by planes; every empty plane is
    exactly zero and the others are held to the bound."""
    from torchnmf_amd.separation import choose_route
    shape = (131, 70, 7)
    H, W = FR.dense_factors(shape)
    labels = [0, 300, 7, 0, 299, 7, 150]
    V = _mixture('real', shape[:2])
    assert choose_route(True, 301, 7, 2.0, 1) == 'planes'
    ref, bound = SE.emulate(H.numpy(), W.numpy(), V.numpy(), labels, 2.0)
    out = separate(H.to(dev), W.to(dev), V.to(dev), labels, power=2.0, _fill=NAN).cpu()
    assert out.shape == (301, 131, 70)
    _note('301 groups', SE.check(out.numpy(), ref, bound, '301 groups'))
    sel = [300, 5, 0]
    Vc = _mixture('complex', shape[:2])
    ref, bound = SE.emulate(H.numpy(), W.numpy(), Vc.numpy(), labels, 1.0, sel)
    part = separate(H.to(dev), W.to(dev), Vc.to(dev), labels, power=1.0, select=sel, _fill=NAN).cpu()
    SE.check(part.numpy(), ref, bound, '301 groups, three selected')
    assert not torch.view_as_real(part[1]).any()
    with pytest.raises(NotImplementedError):
        separate(H.to(dev), W.to(dev), None, labels, _route='fused')


@pytest.mark.parametrize('mix', MIXTURES)
@pytest.mark.parametrize('power', POWERS)
def test_planes_route_select_is_bitwise(dev, power, mix):
    """The planes route with a select: the denominator accumulated plane by plane has the bits of the one the kernel sums."""
    shape = (129, 127, 36)
    H, W, labels = _dense_case(shape, 'empty')
    V = _mixture(mix, shape[:2])
    Hd, Wd, Vd = H.to(dev), W.to(dev), None if V is None else V.to(dev)
    bits = lambda t: torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)
    full = separate(Hd, Wd, Vd, labels, power=power, _route='planes', _fill=NAN)
    part = separate(Hd, Wd, Vd, labels, power=power, select=[3, 1, 0, 3], _route='planes', _fill=NAN)
    assert torch.equal(bits(part), bits(full[[3, 1, 0, 3]]))


@pytest.mark.parametrize('power', [1.0, 2.0])
def test_selected_planes_do_not_cost_g_planes(dev, power):
    """An NMFD model with 12 groups, one selected: beyond what one ``reconstruct`` call itself needs, the planes route holds
    the S output planes, the denominator and (power != 1) one scratch plane -- S + 2 planes, not G."""
    from torchnmf_amd.nmf import NMFD
    B, C, R, Lh, T = 1, 64, 12, 4093, 4
    g = torch.Generator().manual_seed(5)
    H, W = torch.rand(B, R, Lh, generator=g).to(dev), torch.rand(C, R, T, generator=g).to(dev)
    V = torch.randn(B, C, Lh + T - 1, generator=g).to(dev)
    plane = 4 * B * C * (Lh + T - 1)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    one = peak(lambda: NMFD.reconstruct(H[:, :1].contiguous(), W[:, :1].contiguous()))      # its workspace + the plane it returns
    full = peak(lambda: NMFD.reconstruct(H, W))
    S = 1
    got = peak(lambda: separate(H, W, V, None, power=power, select=[5]))
    slack = 1 << 16                   # the tables, index tensors and sub-factors
    allowed = max(one, full) + (S + 2) * plane + slack
    print(f'selected planes p={power:g}: peak {got / plane:.2f} planes, allowed {allowed / plane:.2f}, G = {R}')
    assert got <= allowed, (got, allowed)
    assert allowed < R * plane


# ---- convolutive models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('power', [1.0, 2.0])
@pytest.mark.parametrize('shape', [SHAPES_1D[1], SHAPES_2D[0], SHAPES_3D[0]], ids=_ids)
def test_convolutive_per_element(dev, shape, power):
    H, W = FR.conv_factors(shape)
    R = shape[2]
    labels = [r % 2 for r in range(R)]
    tshape = (shape[0], shape[1]) + tuple(a + t - 1 for a, t in zip(shape[3], shape[4]))
    V = _mixture('real', tshape)
    out = separate(H.to(dev), W.to(dev), V.to(dev), labels, power=power, _fill=NAN)
    assert out.shape == (2,) + tshape and out.dtype == torch.float32
    ref, bound = SE.emulate(H.numpy(), W.numpy(), V.numpy(), labels, power)
    _note(f'convolutive p={power:g}', SE.check(out.cpu().numpy(), ref, bound, f'conv {shape} p={power}'))


# ---- golden ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nmf', 'nmfd'])
def test_golden_g26(dev, name):
    g = load_golden('g26_separate')
    H, W, groups = g[f'{name}_H'], g[f'{name}_W'], g[f'{name}_groups'].tolist()
    for i in range(int(g[f'{name}_cases'])):
        mix, power = str(g[f'{name}_case{i}_mixture']), float(g[f'{name}_case{i}_power'])
        sel = g[f'{name}_case{i}_select'].tolist()
        V = {'none': None, 'real': g[f'{name}_Vreal'], 'complex': g[f'{name}_Vcomplex']}[mix]
        _, bound = SE.emulate(H, W, V, groups, power, sel)
        routes = ('fused', 'planes') if name == 'nmf' else (None,)
        for route in routes:
            out = separate(torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev),
                           None if V is None else torch.from_numpy(V).to(dev), groups, power=power, select=sel, _route=route,
                           _fill=NAN)
            _note(f'golden {name}', SE.check(out.cpu().numpy(), g[f'{name}_case{i}_out'], bound, f'g26 {name} case {i} {route}'))


# ---- the module method -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['NMF', 'NMFD'])
def test_module_method(dev, model):
    from torchnmf_amd import metrics, nmf
    if model == 'NMF':
        H, W, labels = _dense_case((131, 70, 7), 'interleaved')
        tshape = (131, 70)
    else:
        H, W = FR.conv_factors(SHAPES_1D[1])
        labels, tshape = [r % 2 for r in range(7)], (2, 33, 54)
    m = getattr(nmf, model)(W=W, H=H).to(dev)
    h0, w0 = m.H.detach().clone(), m.W.detach().clone()
    V = _mixture('complex', tshape).to(dev)
    a = m.separate(V, labels, power=2.0, select=[1, 0])
    b = metrics.separate(m.H, m.W, V, labels, power=2.0, select=[1, 0])
    assert a.dtype == torch.complex64 and not a.requires_grad
    assert torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32))
    assert torch.equal(m.H.detach(), h0) and torch.equal(m.W.detach(), w0) and m.H.requires_grad and m.W.requires_grad
    masks = m.separate()
    assert masks.shape == (7,) + tshape and masks.dtype == torch.float32
