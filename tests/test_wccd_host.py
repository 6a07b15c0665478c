"""Host side of ``fit(solver='ccd', unstored=omega)`` (torchnmf_amd/wccd.py, the solver branch of BaseComponent.fit, the C
entry of csrc/nmfmu_sparse_wccd.hip): the signatures, the routing and the refusals in their order on CPU tensors, the exported
symbol with its header text and the status codes the C entry answers before any device work.  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from torchnmf_amd import _capi, wccd
from torchnmf_amd import sparse_autograd as SA
from torchnmf_amd.fold_in import fold_in
from torchnmf_amd.nmf import NMF, NMFD, BaseComponent


def _sparse(n, C):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor([1.0, 0.5]), (n, C))


def test_signatures():
    par = inspect.signature(BaseComponent.fit).parameters
    assert par['unstored'].default == 'zero' and par['unstored'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[-1] == 'solver' and par['solver'].default == 'mu'
    assert wccd.__all__ == ['wccd_sweep', 'WeightedCcdEngine'] and wccd.MAX_RANK == 256
    sw = inspect.signature(wccd.wccd_sweep).parameters
    assert list(sw) == ['F', 'panel', 'T', 'side', 'omega', 'l1', 'l2', 'G', '_limit', '_order', '_wg_rows']
    assert sw['omega'].default is inspect.Parameter.empty and sw['l1'].default == 0.0 and sw['l2'].default == 0.0
    assert sw['G'].default is None and sw['_limit'].default == 0 and sw['_order'].default is None and sw['_wg_rows'].default == 0
    assert all(sw[name].kind is inspect.Parameter.KEYWORD_ONLY for name in ('G', '_limit', '_order', '_wg_rows'))
    assert list(inspect.signature(wccd.WeightedCcdEngine.__init__).parameters) == ['self', 'V', 'W', 'H', 'omega', 'l1', 'l2',
                                                                                    'update_W', 'update_H']
    for name in ('target_flags', 'w_step', 'h_step', 'divergence'):
        assert callable(getattr(wccd.WeightedCcdEngine, name))
    assert wccd.WeightedCcdEngine.precision_name == 'fp32'
    assert 'strictly between 0 and 1' in BaseComponent.fit.__doc__ and 'WeightedCcdEngine' in BaseComponent.fit.__doc__


# ---- the routing and the refusals, in order (every call below holds the later faults as well) ------------------------------
def test_a_weight_reaches_the_weighted_engine(monkeypatch):
    """On CPU tensors an admitted call ends at the device check; with that check out of the way, at the engine's constructor."""
    m = NMF((6, 9), rank=4)
    for w in (0.05, 0.5, np.float32(0.3), np.float64(0.999), 1e-6):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored=w)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.double().fit(_sparse(6, 9), beta=2.0, solver='ccd', unstored=0.05, precision='bf16')
    m = NMF((6, 9), rank=4)
    seen = []

    class Stop(Exception):
        pass

    def engine(V, W, H, omega, l1, l2, update_W, update_H):
        seen.append((omega, l1, l2, update_W, update_H))
        raise Stop
    from torchnmf_amd import nmf
    monkeypatch.setattr(nmf, '_require_device', lambda *a, **k: None)
    monkeypatch.setattr(wccd, 'WeightedCcdEngine', engine)
    with pytest.raises(Stop):
        m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored=0.25, alpha=0.5, l1_ratio=0.5)
    assert seen == [(0.25, 0.25, 0.25, True, True)]


def test_the_refusals_of_missing_keep_their_class_and_order():
    g = object()
    conv = NMFD((1, 6, 20), rank=300, T=3)
    for beta in (1, 0, 0.5, 2.5):                                              # beta first
        with pytest.raises(NotImplementedError, match='closed-form only for beta = 2'):
            conv.fit(torch.rand(1, 6, 20), beta=beta, solver='ccd', unstored=0.05, process_group=g)
    with pytest.raises(NotImplementedError, match='NMF only'):                # then the model
        conv.fit(torch.rand(1, 6, 20), beta=2, solver='ccd', unstored=0.05, process_group=g)
    big = NMF((6, 9), rank=300)
    for V in (_sparse(6, 9), torch.rand(6, 9)):
        with pytest.raises(NotImplementedError, match='not sharded'):         # then the group
            big.fit(V, beta=2, solver='ccd', unstored=0.05, process_group=g)
        with pytest.raises(NotImplementedError, match='rank 300 > 256'):      # then the rank
            big.fit(V, beta=2, solver='ccd', unstored=7.0)
    m = NMF((6, 9), rank=256)
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan'), float('inf'), 0, 1, 2):   # then the value, before the target
        with pytest.raises(ValueError, match="^unstored must be 'zero' or 'missing'") as e:
            m.fit(torch.rand(6, 9), beta=2, solver='ccd', unstored=bad)
        assert 'strictly between 0 and 1' in str(e.value)
    with pytest.raises(ValueError, match='sparse-COO'):                       # a dense target stores every entry
        m.fit(torch.rand(6, 9), beta=2, solver='ccd', unstored=0.05)


def test_a_bool_is_not_a_weight():
    m = NMF((6, 9), rank=4)
    for bad in (True, False):
        with pytest.raises(NotImplementedError, match="needs unstored='missing'"):      # as any other non-name: solver='ccd'
            m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored=bad)
        with pytest.raises(ValueError, match="^unstored must be 'zero' or 'missing'"):
            m.fit(_sparse(6, 9), beta=2, unstored=bad)


def test_mu_and_hals_point_at_ccd():
    m = NMF((6, 9), rank=4)
    for solver in ('mu', 'hals'):
        for V in (_sparse(6, 9), torch.rand(6, 9)):
            with pytest.raises(NotImplementedError, match="solver='ccd'"):
                m.fit(V, beta=2, solver=solver, unstored=0.05)
            with pytest.raises(ValueError, match="^unstored must be 'zero' or 'missing'"):    # the value is judged first
                m.fit(V, beta=2, solver=solver, unstored=1.5)
    with pytest.raises(NotImplementedError, match="solver='ccd'"):
        m.fit(_sparse(6, 9), unstored=0.05)                                    # (the defaults: beta = 1, solver='mu')


def test_the_names_are_answered_as_before():
    m = NMF((6, 9), rank=4)
    with pytest.raises(ValueError, match="^unstored must be 'zero' or 'missing'"):
        m.fit(_sparse(6, 9), unstored='0.05')
    with pytest.raises(NotImplementedError, match="needs unstored='missing'"):
        m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored='zero')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored='missing')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(_sparse(6, 9), beta=2, solver='hals')


def test_the_other_entry_points_keep_refusing_a_weight():
    m = NMF((6, 9), rank=4)
    with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
        fold_in(m.W.data, _sparse(6, 9), 2, unstored=0.05)
    with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
        m.transform(_sparse(6, 9), 2, unstored=0.05)
    with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
        SA.sparse_beta_div(torch.rand(6, 4), torch.rand(9, 4), _sparse(6, 9), 2, unstored=0.05)
    with pytest.raises(TypeError):
        m.sparse_fit(_sparse(6, 9), unstored=0.05)


def test_wccd_has_no_cpu_path_and_checks_omega():
    V = _sparse(6, 9)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        wccd.wccd_sweep(torch.rand(6, 3), torch.rand(9, 3), V, 'h', 0.05)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        wccd.wccd_sweep(torch.rand(9, 3), torch.rand(6, 3), V, 'w', 0.05, G=torch.rand(3, 3))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        wccd.WeightedCcdEngine(V, torch.rand(9, 3), torch.rand(6, 3), 0.05)
    with pytest.raises(ValueError, match='side'):
        wccd.wccd_sweep(torch.rand(6, 3), torch.rand(9, 3), V, 'H', 0.05)
    for bad in (0.0, 1.0, -1.0, 2, float('nan'), True, '0.05', None, 1e-60):   # (1e-60 is 0 in fp32)
        with pytest.raises(ValueError, match='omega'):
            wccd.wccd_sweep(torch.rand(6, 3), torch.rand(9, 3), V, 'h', bad)


# ---- the C entry ---------------------------------------------------------------------------------------------------------
def test_symbol_and_header():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    C = ctypes
    assert 'nmfmu_sp_wccd_sweep' in _capi.SIGNATURES and hasattr(raw, 'nmfmu_sp_wccd_sweep')
    res, args = _capi.SIGNATURES['nmfmu_sp_wccd_sweep']
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                    C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert ('int nmfmu_sp_wccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, '
            'int n_rows,\n                        float* owner, const float* panel, int n_panel, int rank, const float* gram, '
            'float omega, float l1,\n                        float l2, float* scratch, int limit, int wg_rows, void* stream);') in hdr
    assert '#define NMFMU_ABI_VERSION 10' in hdr
    assert "nmfmu_sp_wccd_sweep (NMF.fit(solver='ccd', unstored=omega)" in hdr
    mk = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'nmfmu_sparse_wccd.hip' in mk.split('SRCS', 1)[1].split('\n', 1)[0]


def test_c_entry_refuses_before_device_work():
    lib = _capi.load()
    bufs = [ctypes.create_string_buffer(64) for _ in range(8)]
    ptr, idx, vals, order, own, pan, gram, scr = (ctypes.addressof(b) for b in bufs)   # never dereferenced
    ok = dict(rowptr=ptr, idx=idx, vals=vals, order=order, n_rows=3, owner=own, panel=pan, n_panel=5, rank=4, gram=gram,
              omega=0.25, l1=0.0, l2=0.0, scratch=scr, limit=0, wg_rows=0, stream=None)

    def call(**kw):
        return lib.nmfmu_sp_wccd_sweep(*{**ok, **kw}.values())
    for kw in (dict(rowptr=None), dict(idx=None), dict(vals=None), dict(owner=None), dict(panel=None), dict(gram=None),
               dict(scratch=None), dict(panel=own), dict(n_rows=-1), dict(n_panel=0), dict(n_panel=-3), dict(rank=0),
               dict(rank=-2), dict(limit=-1), dict(limit=513), dict(wg_rows=-1), dict(omega=0.0), dict(omega=1.0),
               dict(omega=-0.5), dict(omega=1.5), dict(omega=float('nan')), dict(omega=float('inf')),
               dict(omega=float('-inf')), dict(rank=300, owner=None), dict(rank=257, limit=600), dict(rank=257, omega=1.0)):
        assert call(**kw) == _capi.ERR_ARG, kw
    assert call(rank=257) == _capi.ERR_UNSUPPORTED
    assert call(rank=1 << 20, order=None) == _capi.ERR_UNSUPPORTED
    assert call(n_rows=0) == _capi.OK                                    # nothing to do: answered without a launch
    assert all(bytes(b) == bytes(64) for b in bufs)
