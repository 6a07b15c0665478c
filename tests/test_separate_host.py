"""The host side of ``separation.separate`` without a device: the argument errors of both C entries (answered before any
launch), the order of the Python checks, and the public surface."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

OK, ERR_UNSUPPORTED, ERR_ARG = 0, -2, -3
P = 0x1000          # a non-null address; no call below gets as far as reading it


@pytest.fixture(scope='module')
def lib():
    from torchnmf_amd import _capi
    return _capi.load()


def _i32(xs):
    return (C.c_int32 * len(xs))(*xs)


def _fused(lib, **kw):
    a = dict(Hp=P, n=5, Wp=P, c=4, cols=4, gstart=[0, 2, 4], slot=[0, 1], groups=2, planes=2, tables=P, V=None, v_kind=0,
             ldv=4, power=1.0, eps=2.0 ** -23, out=P, ld=4)
    a.update(kw)
    gs = _i32(a['gstart']) if a['gstart'] is not None else None
    sl = _i32(a['slot']) if a['slot'] is not None else None
    return lib.nmfmu_separate(a['Hp'], a['n'], a['Wp'], a['c'], a['cols'], gs, sl, a['groups'], a['planes'], a['tables'],
                              a['V'], a['v_kind'], a['ldv'], a['power'], a['eps'], a['out'], a['ld'], None)


FUSED_BAD = [dict(Hp=None), dict(Wp=None), dict(gstart=None), dict(slot=None), dict(tables=None), dict(out=None),
             dict(n=0), dict(c=0), dict(cols=0), dict(groups=0), dict(planes=0), dict(n=-3),
             dict(ld=3), dict(v_kind=1, V=None), dict(v_kind=1, V=P, ldv=3), dict(v_kind=2, V=P, ldv=3), dict(v_kind=3, V=P),
             dict(v_kind=-1), dict(power=0.0), dict(power=-1.0), dict(power=float('nan')), dict(eps=-1.0),
             dict(gstart=[0, 4, 2]), dict(gstart=[2, 2, 4]), dict(gstart=[0, 2, 6]), dict(gstart=[0, 1, 4]),
             dict(gstart=[0, 3, 4]), dict(v_kind=2, V=P + 4), dict(v_kind=2, V=P, out=P + 4), dict(out=P + 2), dict(slot=[0, 2]), dict(slot=[-2, 0]), dict(slot=[0, 1], planes=1)]


@pytest.mark.parametrize('bad', FUSED_BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_nmfmu_separate_refuses(lib, bad):
    assert _fused(lib, **bad) == ERR_ARG


def test_nmfmu_separate_limits(lib):
    assert lib.nmfmu_separate_max_rank() == 256
    assert [lib.nmfmu_separate_tables_bytes(g) for g in (-1, 0, 1, 3, 256)] == [0, 0, 12, 28, 2052]
    g = 257
    assert _fused(lib, cols=2 * g, gstart=list(range(0, 2 * g + 1, 2)), slot=[-1] * g, groups=g) == ERR_UNSUPPORTED
    assert _fused(lib, cols=514, gstart=[0, 2, 514]) == ERR_UNSUPPORTED


def _planes(lib, **kw):
    a = dict(Y=P, groups=2, y_stride=8, y_elem=1, D=None, V=None, v_kind=0, n=8, power=2.0, eps=2.0 ** -23, slot=[0, 1],
             planes=2, slot_dev=P, out=P, out_stride=8)
    a.update(kw)
    sl = _i32(a['slot']) if a['slot'] is not None else None
    return lib.nmfmu_separate_planes(a['Y'], a['groups'], a['y_stride'], a['y_elem'], a['D'], a['V'], a['v_kind'], a['n'],
                                     a['power'], a['eps'], sl, a['planes'], a['slot_dev'], a['out'], a['out_stride'], None)


PLANES_BAD = [dict(Y=None), dict(slot=None), dict(slot_dev=None), dict(out=None), dict(groups=0), dict(planes=0), dict(n=0),
              dict(n=-1), dict(y_elem=0), dict(y_elem=3), dict(y_stride=7), dict(y_elem=2, y_stride=15), dict(out_stride=7),
              dict(v_kind=1), dict(v_kind=2), dict(v_kind=3, V=P), dict(power=0.0), dict(power=-2.0),
              dict(power=float('nan')), dict(eps=-1.0), dict(slot=[0, 2]), dict(slot=[-2, 1]), dict(slot=[1, 0], planes=1)]


@pytest.mark.parametrize('bad', PLANES_BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_nmfmu_separate_planes_refuses(lib, bad):
    assert _planes(lib, **bad) == ERR_ARG


@pytest.mark.parametrize('bad', [dict(Y=None), dict(D=None), dict(n=0), dict(y_elem=0), dict(y_elem=3), dict(power=0.0),
                                 dict(power=float('nan'))], ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_nmfmu_separate_accumulate_refuses(lib, bad):
    a = dict(Y=P, y_elem=1, n=8, power=2.0, D=P)
    a.update(bad)
    assert lib.nmfmu_separate_accumulate(a['Y'], a['y_elem'], a['n'], a['power'], a['D'], None) == ERR_ARG


# ---- the Python checks, in order ---------------------------------------------------------------------------------------------------
def _args(**kw):
    a = dict(H=torch.rand(5, 3), W=torch.rand(4, 3), V=None, groups=None, power=1.0, select=None)
    a.update(kw)
    return a


def _call(**kw):
    from torchnmf_amd.separation import separate
    a = _args(**kw)
    return separate(a['H'], a['W'], a['V'], a['groups'], power=a['power'], select=a['select'])


# every entry: (what is wrong, the error it must raise); entry i is called with the faults of entries i .. end all present, so
# the error of entry i shows that its check runs before all later ones
ORDER = [(dict(groups=1.5), TypeError), (dict(groups=[0, 1]), ValueError), (dict(groups=[0, -1, 0]), ValueError),
         (dict(power='2'), TypeError), (dict(power=0.0), ValueError), (dict(power=float('nan')), ValueError),
         (dict(select=2.5), TypeError), (dict(select=[3]), IndexError),
         (dict(H=torch.rand(5, 3, 2)), ValueError),
         (dict(V=torch.rand(5, 5)), ValueError),
         (dict(V=torch.zeros(5, 4, dtype=torch.complex128)), TypeError),
         (dict(), None)]


def test_python_checks_come_in_order():
    from torchnmf_amd import _capi
    for i, (fault, err) in enumerate(ORDER):
        kw = {}
        for later, _ in reversed(ORDER[i:]):
            kw.update(later)          # the earliest fault of a key wins
        if err is None:
            err = _capi.NmfmuError     # CPU tensors: the device check, after everything above
        with pytest.raises(err):
            _call(**kw)


def test_each_python_check_alone():
    from torchnmf_amd import _capi
    for fault, err in ORDER[:-1]:
        with pytest.raises(err):
            _call(**fault)
    with pytest.raises(TypeError):
        _call(groups=[0, 1.0, 0])
    with pytest.raises(TypeError):
        _call(groups=torch.tensor([0.0, 1.0, 0.0]))
    with pytest.raises(TypeError):
        _call(power=True)
    with pytest.raises(ValueError):
        _call(power=float('inf'))
    with pytest.raises(IndexError):
        _call(select=[-1])
    with pytest.raises(TypeError):
        _call(select=[0, 1.0])
    with pytest.raises(ValueError):
        _call(W=torch.rand(4, 3, 2, 2, 2, 2), H=torch.rand(1, 3, 2, 2, 2, 2))
    with pytest.raises(TypeError):
        _call(V=torch.zeros(5, 4, dtype=torch.int32))
    # the device check precedes the factors' dtype, and the wording is the other entry points'
    with pytest.raises(_capi.NmfmuError, match=re.escape('tensors must live on the ROCm device (no CPU fallback)')):
        _call(H=torch.zeros(5, 3, dtype=torch.int32))
    # the signs of the factors are not scanned: a negative factor gets as far as the device check
    with pytest.raises(_capi.NmfmuError):
        _call(H=-torch.rand(5, 3))
    with pytest.raises(ValueError):
        from torchnmf_amd.separation import separate
        separate(torch.rand(5, 3), torch.rand(4, 3), _route='eager')


def test_factor_dtype_check(monkeypatch):
    """The last check: reached only by tensors that pass the device check."""
    from torchnmf_amd import separation
    real = torch.device

    class _OnDevice(torch.Tensor):
        @property
        def device(self):
            return real('cuda:0')
    H = torch.zeros(5, 3, dtype=torch.int32).as_subclass(_OnDevice)
    W = torch.rand(4, 3).as_subclass(_OnDevice)
    with pytest.raises(TypeError, match='factors must be floating point'):
        separation._check_args(H, W, None, None, 1.0, None, None)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_public_names():
    from torchnmf_amd import metrics, nmf, separation
    assert metrics.separate is separation.separate and 'separate' in metrics.__all__
    assert nmf.__all__ == ['BaseComponent', 'NMF', 'NMFD', 'NMF2D', 'NMF3D']
    for cls in (nmf.NMF, nmf.NMFD, nmf.NMF2D, nmf.NMF3D):
        assert cls.separate is nmf.BaseComponent.separate


def test_signatures():
    from torchnmf_amd import nmf, separation
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(separation.separate).parameters
    assert [(n, p.kind) for n, p in sig.items()] == [('H', POS), ('W', POS), ('V', POS), ('groups', POS), ('power', KW),
                                                         ('select', KW), ('_route', KW)]
    assert (sig['V'].default, sig['groups'].default, sig['power'].default, sig['select'].default,
            sig['_route'].default) == (None, None, 1.0, None, None)
    sig = inspect.signature(nmf.BaseComponent.separate).parameters
    assert [(n, p.kind) for n, p in sig.items()] == [('self', POS), ('V', POS), ('groups', POS), ('power', KW), ('select', KW)]
    assert (sig['V'].default, sig['groups'].default, sig['power'].default, sig['select'].default) == (None, None, 1.0, None)


def test_abi_and_header(lib):
    from torchnmf_amd import _capi
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    text = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    assert '#define NMFMU_ABI_VERSION 10 ' in text
    for name in ('nmfmu_separate', 'nmfmu_separate_planes', 'nmfmu_separate_accumulate', 'nmfmu_separate_max_rank',
                 'nmfmu_separate_tables_bytes'):
        assert re.search(r'\b' + name + r'\(', text), name
        assert name in _capi.SIGNATURES


def test_route_rule():
    """The rule of DESIGN section 33: planes for convolutive models, for ranks or group counts the fused kernel does not hold,
    and where they were measured to win (a real mixture, power != 1, every plane wanted, few groups of a long rank)."""
    from torchnmf_amd.separation import V_COMPLEX, V_NONE, V_REAL, choose_route
    assert choose_route(False, 2, 8) == 'planes' and choose_route(True, 2, 257) == 'planes'
    assert choose_route(True, 256, 256) == 'fused' and choose_route(True, 16, 128, 2.0, V_REAL) == 'fused'
    # more groups than the kernel's tables hold (labels may leave empty groups), whatever else
    for kind in (V_NONE, V_REAL, V_COMPLEX):
        for identity in (True, False):
            assert choose_route(True, 257, 4, 1.0, kind, identity) == 'planes'
            assert choose_route(True, 256, 4, 1.0, kind, identity) == 'fused'
    assert [choose_route(True, G, 128, 2.0, V_REAL) for G in (2, 4, 5, 16)] == ['planes', 'planes', 'fused', 'fused']
    # a tie (power 1, G = 2) does not cost a plane; what was not measured (no mixture) goes fused
    assert [choose_route(True, G, 128, 1.0, V_REAL) for G in (2, 4)] == ['fused', 'fused']
    assert choose_route(True, 2, 128, 2.0, V_NONE) == 'fused'
    assert choose_route(True, 2, 128, 2.0, V_COMPLEX) == 'fused'
    assert choose_route(True, 2, 128, 2.0, V_REAL, identity=False) == 'fused'


def test_fused_route_refuses_what_it_does_not_hold():
    """``_route='fused'`` with more than 256 groups: refused in the checks (the last of them), before anything is allocated."""
    from torchnmf_amd import separation

    class _OnDevice(torch.Tensor):
        @property
        def device(self):
            return torch.device('cuda:0')
    H, W = torch.rand(5, 4).as_subclass(_OnDevice), torch.rand(6, 4).as_subclass(_OnDevice)
    with pytest.raises(NotImplementedError):
        separation._check_args(H, W, None, [0, 1, 2, 300], 1.0, None, 'fused')
    assert separation._check_args(H, W, None, [0, 1, 2, 255], 1.0, None, 'fused')[0] == [0, 1, 2, 255]
