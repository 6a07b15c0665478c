"""Host side of solver='ccd' (torchnmf_amd/ccd.py, the solver branch of BaseComponent.fit, the C entry of
csrc/nmfmu_sparse_ccd.hip): the signature, the refusals in their order on CPU tensors, the exported symbols with their header
text and the status codes the C entry answers before any device work.  No GPU."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import ROOT
from torchnmf_amd import _capi, ccd
from torchnmf_amd.nmf import NMF, NMFD, BaseComponent


def _sparse(n, C):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor([1.0, 0.5]), (n, C))


def test_signature():
    par = inspect.signature(BaseComponent.fit).parameters
    assert par['solver'].default == 'mu' and par['solver'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[-1] == 'solver'
    assert ccd.__all__ == ['ccd_sweep', 'CcdEngine', 'RESIDENT_LIMIT', 'WG_WAVES'] and ccd.MAX_RANK == 256
    sw = inspect.signature(ccd.ccd_sweep).parameters
    assert list(sw)[:6] == ['F', 'panel', 'T', 'side', 'l1', 'l2'] and sw['l1'].default == 0.0 and sw['l2'].default == 0.0
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in sw.items() if name.startswith('_'))
    assert list(inspect.signature(ccd.CcdEngine.__init__).parameters) == ['self', 'V', 'W', 'H', 'l1', 'l2', 'update_W',
                                                                           'update_H']
    for name in ('target_flags', 'w_step', 'h_step', 'divergence'):
        assert callable(getattr(ccd.CcdEngine, name))
    assert ccd.CcdEngine.precision_name == 'fp32'
    assert "'ccd'" in BaseComponent.fit.__doc__


def test_the_residency_limit_is_the_librarys():
    lib = _capi.load()
    assert ccd.RESIDENT_LIMIT == lib.nmfmu_sp_ccd_limit() == 512 and ccd.RESIDENT_LIMIT % 64 == 0
    assert ccd.WG_WAVES == lib.nmfmu_sp_ccd_wg_waves() == 16
    for rank in (1, 3, 64, 100, 256):
        rows = lib.nmfmu_sp_ccd_lds_rows(rank)
        assert rows == ccd.lds_rows(rank) >= 1 and (rows + 1) * (rank | 1) > 10240 >= rows * (rank | 1)
    assert lib.nmfmu_sp_ccd_lds_rows(0) == 0 and lib.nmfmu_sp_ccd_lds_rows(257) == 0


# ---- the refusals, in order (every call below holds the later faults as well) -----------------------------------------------
def test_solver_name_comes_first():
    m = NMFD((1, 6, 20), rank=300, T=3)
    for bad in ('CCD', 'cd', 'ccd ', None, 0):
        with pytest.raises(ValueError, match='solver'):
            m.fit(torch.rand(1, 6, 20), beta=1, solver=bad, unstored='zero', process_group=object())


def test_beta_before_model():
    m = NMFD((1, 6, 20), rank=300, T=3)
    for beta in (1, 0, 0.5, 2.5):
        with pytest.raises(NotImplementedError, match='closed-form only for beta = 2'):
            m.fit(torch.rand(1, 6, 20), beta=beta, solver='ccd', unstored='zero', process_group=object())


def test_model_before_unstored():
    m = NMFD((1, 6, 20), rank=300, T=3)
    with pytest.raises(NotImplementedError, match='NMF only'):
        m.fit(torch.rand(1, 6, 20), beta=2, solver='ccd', unstored='zero', process_group=object())


def test_unstored_before_group():
    m = NMF((6, 9), rank=300)
    for V in (_sparse(6, 9), torch.rand(6, 9)):
        for kw in (dict(), dict(unstored='zero'), dict(unstored='nothing')):
            with pytest.raises(NotImplementedError, match="solver='hals'") as e:
                m.fit(V, beta=2, solver='ccd', process_group=object(), **kw)
            assert "unstored='missing'" in str(e.value)


def test_group_before_rank():
    m = NMF((6, 9), rank=300)
    with pytest.raises(NotImplementedError, match='not sharded'):
        m.fit(_sparse(6, 9), beta=2, solver='ccd', unstored='missing', process_group=object())


def test_rank_before_the_existing_checks():
    with pytest.raises(NotImplementedError, match='rank 257 > 256'):
        NMF((6, 9), rank=257).fit(torch.rand(6, 9), beta=2, solver='ccd', unstored='missing')
    m = NMF((6, 9), rank=256)
    W0, H0 = m.W.detach().clone(), m.H.detach().clone()
    with pytest.raises(ValueError, match='sparse-COO'):                       # a dense V with 'missing'
        m.fit(torch.rand(6, 9), beta=2, solver='ccd', unstored='missing')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):           # admitted: the device check answers
        m.fit(_sparse(6, 9), beta=2.0, solver='ccd', unstored='missing', precision='bf16')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.double().fit(_sparse(6, 9), beta=2, solver='ccd', unstored='missing')
    assert torch.equal(m.W.float(), W0) and torch.equal(m.H.float(), H0)


def test_hals_points_at_ccd_for_missing_data():
    with pytest.raises(NotImplementedError, match="unstored = 'zero'") as e:
        NMF((6, 9), rank=4).fit(_sparse(6, 9), beta=2, solver='hals', unstored='missing')
    assert "solver='ccd'" in str(e.value)


def test_ccd_has_no_cpu_path():
    V = _sparse(6, 9)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ccd.ccd_sweep(torch.rand(6, 3), torch.rand(9, 3), V, 'h')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ccd.ccd_sweep(torch.rand(9, 3), torch.rand(6, 3), V, 'w')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ccd.CcdEngine(V, torch.rand(9, 3), torch.rand(6, 3))
    with pytest.raises(ValueError, match='side'):
        ccd.ccd_sweep(torch.rand(6, 3), torch.rand(9, 3), V, 'H')


# ---- the C entry ---------------------------------------------------------------------------------------------------------
def test_symbols_and_header():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    C = ctypes
    for name in ('nmfmu_sp_ccd_sweep', 'nmfmu_sp_ccd_limit', 'nmfmu_sp_ccd_wg_waves', 'nmfmu_sp_ccd_lds_rows'):
        assert name in _capi.SIGNATURES and hasattr(raw, name)
    res, args = _capi.SIGNATURES['nmfmu_sp_ccd_sweep']
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                    C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert _capi.SIGNATURES['nmfmu_sp_ccd_limit'] == _capi.SIGNATURES['nmfmu_sp_ccd_wg_waves'] == (C.c_int, [])
    assert _capi.SIGNATURES['nmfmu_sp_ccd_lds_rows'] == (C.c_int, [C.c_int])
    assert ('int nmfmu_sp_ccd_sweep(const int32_t* rowptr, const int32_t* idx, const float* vals, const int32_t* order, '
            'int n_rows,\n                       float* owner, const float* panel, int n_panel, int rank, float l1, float l2, '
            'float* scratch,\n                       float* panel_t, int limit, int lds_rows, int wg_rows, void* stream);') in hdr
    for decl in ('int nmfmu_sp_ccd_limit(void);', 'int nmfmu_sp_ccd_wg_waves(void);', 'int nmfmu_sp_ccd_lds_rows(int rank);'):
        assert decl in hdr
    assert '#define NMFMU_ABI_VERSION 10' in hdr
    assert ("nmfmu_sp_ccd_sweep / nmfmu_sp_ccd_limit / nmfmu_sp_ccd_wg_waves / nmfmu_sp_ccd_lds_rows "
            "(NMF.fit(solver='ccd')") in hdr
    mk = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'nmfmu_sparse_ccd.hip' in mk.split('SRCS', 1)[1].split('\n', 1)[0]


def test_c_entry_refuses_before_device_work():
    lib = _capi.load()
    bufs = [ctypes.create_string_buffer(64) for _ in range(8)]
    ptr, idx, vals, order, own, pan, scr, pt = (ctypes.addressof(b) for b in bufs)   # never dereferenced
    ok = dict(rowptr=ptr, idx=idx, vals=vals, order=order, n_rows=3, owner=own, panel=pan, n_panel=5, rank=4, l1=0.0, l2=0.0,
              scratch=scr, panel_t=pt, limit=0, lds_rows=0, wg_rows=0, stream=None)

    def call(**kw):
        return lib.nmfmu_sp_ccd_sweep(*{**ok, **kw}.values())
    for kw in (dict(rowptr=None), dict(idx=None), dict(vals=None), dict(owner=None), dict(panel=None), dict(scratch=None),
               dict(panel=own), dict(n_rows=-1), dict(n_panel=0), dict(n_panel=-3), dict(rank=0), dict(rank=-2),
               dict(limit=-1), dict(limit=513), dict(lds_rows=-1), dict(wg_rows=-1), dict(rank=300, owner=None),
               dict(rank=257, limit=600)):
        assert call(**kw) == _capi.ERR_ARG, kw
    assert call(rank=257) == _capi.ERR_UNSUPPORTED
    assert call(rank=1 << 20, order=None, panel_t=None) == _capi.ERR_UNSUPPORTED
    assert call(n_rows=0) == _capi.OK                                    # nothing to do: answered without a launch
    assert all(bytes(b) == bytes(64) for b in bufs)
