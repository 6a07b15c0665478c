"""Weighted NMF without a GPU: the argument errors of the new C entries (every call returns before a launch), the workspace
and split-count rules against their Python statement in tests/weighted_emulation.py, the validation order of ``weights`` on
CPU tensors, and the signature of ``fit``."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import weighted_emulation as WE
from torchnmf_amd import _capi, metrics, wmu
from torchnmf_amd.nmf import NMF, NMFD, BaseComponent

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _terms(lib, **kw):
    a = dict(V=P, M=P, ld=70, n=131, c=70, side=0, owner=P, panel=P + 64, rank=5, r_pad=32, beta=1.0, nsplit=0, ws=P, num=P,
             den=P)
    a.update(kw)
    return lib.nmfmu_wmu_terms(a['V'], a['M'], a['ld'], a['n'], a['c'], a['side'], a['owner'], a['panel'], a['rank'],
                               a['r_pad'], a['beta'], a['nsplit'], a['ws'], a['num'], a['den'], None)


def _step(lib, **kw):
    a = dict(V=P, M=P, ld=70, n=131, c=70, side=0, owner=P, panel=P + 64, rank=5, r_pad=32, beta=1.0, nsplit=0, ws=P)
    a.update(kw)
    return lib.nmfmu_wmu_step(a['V'], a['M'], a['ld'], a['n'], a['c'], a['side'], a['owner'], a['panel'], a['rank'],
                              a['r_pad'], a['beta'], 0.0, 0.0, 1.0, a['nsplit'], a['ws'], None)


def _loss(lib, **kw):
    a = dict(V=P, M=P, ld=70, n=131, c=70, owner=P, panel=P + 64, rank=5, beta=1.0, part=P, out=P)
    a.update(kw)
    return lib.nmfmu_wmu_loss(a['V'], a['M'], a['ld'], a['n'], a['c'], a['owner'], a['panel'], a['rank'], a['beta'], 0.0,
                              a['part'], a['out'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('V', 'M', 'owner', 'panel', 'ws', 'num', 'den')),
                                           (_step, ('V', 'M', 'owner', 'panel', 'ws')),
                                           (_loss, ('V', 'M', 'owner', 'panel', 'part', 'out'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    assert call(lib, rank=0) == _capi.ERR_ARG and call(lib, rank=-3) == _capi.ERR_ARG
    assert call(lib, n=0) == _capi.ERR_ARG and call(lib, c=-1) == _capi.ERR_ARG and call(lib, ld=69) == _capi.ERR_ARG
    assert call(lib, rank=257, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    for beta in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0):                      # no beta is refused -- only the rank
        assert call(lib, rank=300, beta=beta, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    if call is not _loss:
        for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
            assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
        assert call(lib, nsplit=-1) == _capi.ERR_ARG
        assert call(lib, side=2) == _capi.ERR_ARG and call(lib, side=-1) == _capi.ERR_ARG
        assert call(lib, nsplit=-1, rank=300, r_pad=256) == _capi.ERR_ARG      # the arguments are judged before the rank


def test_step_refuses_aliased_factors():
    assert _step(_capi.load(), owner=P, panel=P) == _capi.ERR_ARG


def test_workspace_and_split_rules():
    lib = _capi.load()
    shapes = [(131, 70), (70, 131), (132, 72), (515, 1030), (1030, 515), (4096, 65536), (65536, 4096), (1, 1), (128, 32),
              (129, 33), (100000, 100)]
    for rows, contraction in shapes:
        for r_pad in (32, 64, 128, 256):
            auto = lib.nmfmu_wmu_nsplit(rows, contraction, r_pad)
            assert auto == WE.split(rows, contraction, r_pad) >= 1
            assert auto <= 64 and (auto == 1 or WE.part_len(contraction, auto) >= 128)     # the library's parts: >= 4 stages
            for nsplit in (0, 1, 2, 3, 7, 1000):
                want = WE.workspace_floats(rows, contraction, r_pad, nsplit)
                assert lib.nmfmu_wmu_ws(rows, contraction, r_pad, nsplit) == want == wmu.workspace_floats(rows, contraction,
                                                                                                         r_pad, nsplit)
                parts = want // (2 * rows * r_pad)
                assert 1 <= parts <= WE.stages(contraction)
                # no empty part, only the last one short
                assert (parts - 1) * WE.part_len(contraction, parts) < contraction <= parts * WE.part_len(contraction, parts)
        assert lib.nmfmu_wmu_loss_parts(rows, contraction) == WE.loss_parts(rows, contraction) >= -(-rows // 128)
    assert lib.nmfmu_wmu_nsplit(4096, 65536, 128) == 16 and lib.nmfmu_wmu_nsplit(65536, 4096, 128) == 1
    assert lib.nmfmu_wmu_nsplit(4096, 65536, 256) == 8               # two rank tiles: half the parts
    for bad in ((0, 70, 32, 0), (131, 0, 32, 0), (131, 70, 0, 0), (131, 70, 32, -1)):
        assert lib.nmfmu_wmu_ws(*bad) == 0
    assert lib.nmfmu_wmu_nsplit(0, 70, 32) == _capi.ERR_ARG and lib.nmfmu_wmu_loss_parts(131, 0) == _capi.ERR_ARG


def test_abi_is_additive():
    lib = _capi.load()
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in ('nmfmu_wmu_nsplit', 'nmfmu_wmu_ws', 'nmfmu_wmu_terms', 'nmfmu_wmu_step', 'nmfmu_wmu_loss_parts',
                 'nmfmu_wmu_loss'):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)
    assert lib.nmfmu_wmu_ws.restype is C.c_int64
    assert len(_capi.SIGNATURES['nmfmu_wmu_terms'][1]) == 16 and len(_capi.SIGNATURES['nmfmu_wmu_step'][1]) == 17
    assert len(_capi.SIGNATURES['nmfmu_wmu_loss'][1]) == 13 and _capi.SIGNATURES['nmfmu_wmu_loss'][1][9] is C.c_double


def test_signature():
    par = inspect.signature(BaseComponent.fit).parameters
    assert par['weights'].default is None and par['weights'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[-2:] == ['weights', 'solver'] and par['solver'].default == 'mu'
    assert list(inspect.signature(wmu.WeightedMU.__init__).parameters)[:10] == ['self', 'V', 'M', 'W', 'H', 'beta', 'l1', 'l2',
                                                                                'update_W', 'update_H']
    for name in ('target_flags', 'w_step', 'h_step', 'divergence'):
        assert callable(getattr(wmu.WeightedMU, name))
    assert wmu.WeightedMU.precision_name == 'fp32' and wmu.MAX_RANK == 256
    assert metrics.weighted_beta_div is wmu.weighted_beta_div and 'weighted_beta_div' in metrics.__all__
    assert list(inspect.signature(wmu.weighted_beta_div).parameters) == ['H', 'W', 'V', 'weights', 'beta']


def _sparse(N=6, Cc=5):
    i = torch.tensor([[0, 1, 1, 4], [0, 2, 3, 4]])
    return torch.sparse_coo_tensor(i, torch.tensor([1.0, 2.0, 0.5, 3.0]), (N, Cc)).coalesce()


def test_weights_validation_comes_first():
    """On CPU tensors: every error of the keyword is raised before the device check (which raises NmfmuError)."""
    m = NMF((6, 5), rank=2)
    V = torch.rand(6, 5) + 0.1
    ok = torch.ones(6, 5)
    with pytest.raises(NotImplementedError, match="unstored='missing'"):
        m.fit(_sparse(), weights=ok)
    with pytest.raises(NotImplementedError, match='NMF only'):
        NMFD((1, 5, 6), rank=2, T=2).fit(torch.rand(1, 5, 6), weights=torch.ones(1, 5, 6))
    with pytest.raises(NotImplementedError, match='not sharded'):
        m.fit(V, weights=ok, process_group=object())
    for solver in ('hals', 'ccd'):
        with pytest.raises(NotImplementedError, match="solver='mu' only"):
            m.fit(V, beta=2, weights=ok, solver=solver)
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        NMF((6, 5), rank=300).fit(V, weights=ok)
    for bad in (torch.ones(5, 6), torch.ones(6, 5, 1), torch.ones(30)):
        with pytest.raises(ValueError, match='shape of V'):
            m.fit(V, weights=bad)
    with pytest.raises(ValueError, match='shape of V'):
        m.fit(V, weights=ok.to_sparse())
    with pytest.raises(ValueError, match='must be a tensor'):
        m.fit(V, weights=ok.numpy())
    with pytest.raises(ValueError, match='bool, integer or floating'):
        m.fit(V, weights=ok.to(torch.complex64))
    for value in (-1.0, float('nan'), float('inf')):
        w = ok.clone()
        w[2, 3] = value
        with pytest.raises(ValueError, match='finite and non-negative'):
            m.fit(V, weights=w)
    # past the validation: the device check; bool, integer, half and double weights are all admitted
    for w in (ok, ok > 0, ok.to(torch.int32), ok.to(torch.uint8), ok.half(), ok.double()):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, weights=w)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):     # the default is untouched
        m.fit(V)
    with pytest.raises(TypeError):                                     # keyword-only
        m.fit(V, 1, 1e-4, 200, False, 0, 0, ok)
    # the order among them: the cheap refusals before the scan of the values
    w = ok.clone()
    w[0, 0] = -1
    with pytest.raises(NotImplementedError, match='not sharded'):
        m.fit(V, weights=w, process_group=object())


def test_check_weights_converts_once():
    V = torch.rand(4, 3)
    for w in (torch.tensor([[True, False, True]] * 4), torch.arange(12).reshape(4, 3), torch.rand(4, 3).double()):
        out = wmu.check_weights(V, w)
        assert out.dtype == torch.float32 and out.is_contiguous() and torch.equal(out, w.float())
    w = torch.rand(3, 4).t()                                           # not contiguous: copied
    assert wmu.check_weights(V, w).is_contiguous()


def test_weighted_target_flags_and_v_term():
    """The flags look at weighted entries only; the terms of v alone are those of weighted_emulation."""
    V, M, _, _ = WE.make_problem(14, 24, 3)
    T = wmu.WeightedTarget(torch.from_numpy(V), torch.from_numpy(M))
    assert (T.bad, T.has_zero) == (False, False)                       # NaN, Inf, -1 under zero weights do not count
    for beta in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0):
        assert T.v_term(beta) == pytest.approx(WE.v_term(V, M, beta), rel=1e-13)
    i, j = (int(x) for x in np.argwhere(M > 0)[0])
    for value, flags in ((0.0, (False, True)), (-0.5, (True, False)), (float('nan'), (True, False))):
        V2 = V.copy()
        V2[i, j] = value
        T2 = wmu.WeightedTarget(torch.from_numpy(V2), torch.from_numpy(M))
        assert (T2.bad, T2.has_zero) == flags, value


def test_weighted_beta_div_validation():
    H, W, V = torch.rand(6, 2), torch.rand(5, 2), torch.rand(6, 5) + 0.1
    with pytest.raises(ValueError, match='shape of V'):
        wmu.weighted_beta_div(H, W, V, torch.ones(5, 6), 1)
    with pytest.raises(ValueError, match='finite and non-negative'):
        wmu.weighted_beta_div(H, W, V, -torch.ones(6, 5), 1)
    with pytest.raises(NotImplementedError, match="unstored='missing'"):
        wmu.weighted_beta_div(H, W, V.to_sparse(), torch.ones(6, 5), 1)
    for beta in (-1, 0, 0.5, 1, 2):                                    # every beta is admitted, then the device is needed
        with pytest.raises(_capi.NmfmuError, match='ROCm device'):
            wmu.weighted_beta_div(H, W, V, torch.ones(6, 5), beta)
