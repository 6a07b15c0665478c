"""Host side of solver='hals' (torchnmf_amd/hals.py, the solver branch of BaseComponent.fit, the C entry of
csrc/nmfmu_hals.hip): the refusals in their order on CPU tensors, the untouched default path, the exported symbols and the
status codes the C entry answers before any device work.  No GPU."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import ROOT
from torchnmf_amd import _capi, hals
from torchnmf_amd.nmf import NMF, NMFD, BaseComponent
from torchnmf_amd.plca import PLCA


def _sparse(n, C):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor([1.0, 0.5]), (n, C))


def test_signature():
    par = inspect.signature(BaseComponent.fit).parameters
    assert par['solver'].default == 'mu' and par['solver'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[-1] == 'solver'                       # appended: every earlier argument keeps its place
    assert hals.__all__ == ['hals_sweep', 'HalsEngine'] and hals.MAX_RANK == 256
    assert list(inspect.signature(hals.hals_sweep).parameters) == ['F', 'A', 'G', 'l1', 'l2']
    assert list(inspect.signature(hals.HalsEngine.__init__).parameters) == ['self', 'V', 'W', 'H', 'l1', 'l2', 'update_W',
                                                                             'update_H']
    for name in ('target_flags', 'w_step', 'h_step', 'divergence'):
        assert callable(getattr(hals.HalsEngine, name))
    assert hals.HalsEngine.precision_name == 'fp32'
    assert not hasattr(PLCA, 'solver')


# ---- the refusals, in order (every call below holds the later faults as well) -----------------------------------------------
def test_solver_name_comes_first():
    m = NMFD((1, 6, 20), rank=300, T=3)                    # not NMF, rank too large, beta != 2, missing, a group
    for bad in ('HALS', 'cd', None, 0):
        with pytest.raises(ValueError, match='solver'):
            m.fit(torch.rand(1, 6, 20), beta=1, solver=bad, unstored='missing', process_group=object())


def test_beta_before_model():
    m = NMFD((1, 6, 20), rank=300, T=3)
    for beta in (1, 0, 0.5, 2.5):
        with pytest.raises(NotImplementedError, match='closed-form only for beta = 2'):
            m.fit(torch.rand(1, 6, 20), beta=beta, solver='hals', unstored='missing', process_group=object())


def test_model_before_unstored():
    m = NMFD((1, 6, 20), rank=300, T=3)
    with pytest.raises(NotImplementedError, match='NMF only'):
        m.fit(torch.rand(1, 6, 20), beta=2, solver='hals', unstored='missing', process_group=object())


def test_unstored_before_group():
    m = NMF((6, 9), rank=300)
    with pytest.raises(NotImplementedError, match="unstored = 'zero'"):
        m.fit(_sparse(6, 9), beta=2, solver='hals', unstored='missing', process_group=object())


def test_group_before_rank():
    m = NMF((6, 9), rank=300)
    with pytest.raises(NotImplementedError, match='not sharded'):
        m.fit(torch.rand(6, 9), beta=2, solver='hals', process_group=object())


def test_rank_before_device():
    with pytest.raises(NotImplementedError, match='rank 257 > 256'):
        NMF((6, 9), rank=257).fit(torch.rand(6, 9), beta=2, solver='hals')
    m = NMF((6, 9), rank=256)
    W0, H0 = m.W.detach().clone(), m.H.detach().clone()
    for V in (torch.rand(6, 9), _sparse(6, 9)):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):       # admitted: the device check answers
            m.fit(V, beta=2.0, solver='hals', precision='bf16')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.double().fit(torch.rand(6, 9), beta=2, solver='hals')
    assert torch.equal(m.W.float(), W0) and torch.equal(m.H.float(), H0)


def test_default_solver_reaches_the_existing_device_check():
    m = NMF((6, 9), rank=4)
    for kw in (dict(), dict(solver='mu'), dict(solver='mu', beta=1), dict(solver='mu', unstored='missing')):
        V = _sparse(6, 9) if 'unstored' in kw else torch.rand(6, 9)
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, **{'beta': 2, **kw})
    with pytest.raises(ValueError, match='unstored'):                        # the existing checks still answer in their place
        m.fit(torch.rand(6, 9), beta=2, solver='mu', unstored='nothing')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        NMFD((1, 6, 20), rank=3, T=3).fit(torch.rand(1, 6, 20), solver='mu')


def test_hals_sweep_has_no_cpu_path():
    F, A, G = torch.rand(5, 3), torch.rand(5, 3), torch.eye(3)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        hals.hals_sweep(F, A, G)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        hals.HalsEngine(torch.rand(5, 4), torch.rand(4, 3), torch.rand(5, 3))


# ---- the C entry ---------------------------------------------------------------------------------------------------------
def test_symbol_and_abi():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    assert 'nmfmu_hals_sweep' in _capi.SIGNATURES and hasattr(raw, 'nmfmu_hals_sweep')
    res, args = _capi.SIGNATURES['nmfmu_hals_sweep']
    C = ctypes
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    assert ('int nmfmu_hals_sweep(float* f, int rows, int rank, const float* a, int64_t lda, const float* gram, float l1, '
            'float l2,\n                     void* stream);') in hdr
    assert '#define NMFMU_ABI_VERSION 10' in hdr and 'nmfmu_hals_sweep (NMF.fit(solver=\'hals\')' in hdr
    mk = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'nmfmu_hals.hip' in mk.split('SRCS', 1)[1].split('\n', 1)[0]


def test_c_entry_refuses_before_device_work():
    lib = _capi.load()
    buf, buf2, buf3 = (ctypes.create_string_buffer(64) for _ in range(3))
    f, a, g = (ctypes.addressof(b) for b in (buf, buf2, buf3))     # never dereferenced: every call is answered on its arguments
    ok = dict(f=f, rows=3, rank=4, a=a, lda=4, gram=g, l1=0.0, l2=0.0, stream=None)

    def call(**kw):
        return lib.nmfmu_hals_sweep(*{**ok, **kw}.values())
    for kw in (dict(f=None), dict(a=None), dict(gram=None), dict(rows=0), dict(rows=-1), dict(rank=0), dict(rank=-2),
               dict(lda=3), dict(lda=0), dict(lda=-4), dict(rank=257, lda=256), dict(rank=300, f=None, lda=300)):
        assert call(**kw) == _capi.ERR_ARG, kw
    assert call(rank=257, lda=257) == _capi.ERR_UNSUPPORTED
    assert call(rank=1 << 20, lda=1 << 20) == _capi.ERR_UNSUPPORTED
    assert bytes(buf) == bytes(64)
