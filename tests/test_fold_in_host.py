"""Host side of the fold-in (torchnmf_amd/fold_in.py, the C entries of csrc/nmfmu_fold_in.hip): the argument checks in their
order on CPU tensors (the checks behind the device check need the device: tests/test_gpu_fold_in.py), the exported symbols,
the status codes the C entry answers before any device work, and which models carry ``transform``.  No GPU."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import ROOT
import fold_in_emulation as E
from torchnmf_amd import _capi, fold_in as FI, metrics
from torchnmf_amd.nmf import NMF, NMF2D, NMF3D, NMFD
from torchnmf_amd.plca import PLCA, SIPLCA


def _w(C=9, R=4, dtype=torch.float32):
    return torch.rand(C, R, generator=torch.Generator().manual_seed(0)).to(dtype)


def _sparse(n, C, vals=(1.0, 0.5)):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor(vals), (n, C))


def test_exports():
    assert metrics.fold_in is FI.fold_in and 'fold_in' in metrics.__all__
    assert FI.MODES == {'missing': 0, 'zero': 1}
    want = ['W', 'target', 'beta', 'max_iter', 'tol', 'alpha', 'l1_ratio', 'unstored', 'H0', 'generator', 'return_n_iter']
    par = inspect.signature(FI.fold_in).parameters
    assert [p for p in par if not p.startswith('_')] == want
    assert [par[p].default for p in want[2:]] == [1, 200, 1e-4, 0, 0, 'zero', None, None, False]
    assert all(par[p].kind is inspect.Parameter.KEYWORD_ONLY for p in want[7:])
    tpar = inspect.signature(NMF.transform).parameters
    assert list(tpar) == ['self', 'V_new'] + want[2:]
    assert [tpar[p].default for p in want[2:]] == [par[p].default for p in want[2:]]


# ---- the checks, in order -----------------------------------------------------------------------------------------------------
def test_unstored_comes_first():
    for bad in ('Missing', None, 0, 'nan'):
        with pytest.raises(ValueError, match='unstored'):
            FI.fold_in(_w(), torch.zeros(3, 9), max_iter=-1, unstored=bad)       # dense and a bad max_iter as well


def test_dense_target_before_max_iter():
    for bad in (torch.zeros(3, 9), [[1.0]], None):
        with pytest.raises(ValueError, match=r'sparse_mask\(mask\).*trainable_W=False'):
            FI.fold_in(_w(), bad, max_iter=-1, unstored='missing')


def test_max_iter_and_tol_before_shapes():
    V = _sparse(3, 8)                                                            # the columns disagree as well
    for bad in (-1, 2.0, '3', None, True):
        with pytest.raises(ValueError, match='max_iter'):
            FI.fold_in(_w(), V, max_iter=bad)
    for bad in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='tol'):
            FI.fold_in(_w(), V, tol=bad)


def test_shapes_before_rank():
    W = _w(R=300)                                                                # rank too large as well
    with pytest.raises(ValueError, match='columns'):
        FI.fold_in(W, _sparse(3, 8))
    with pytest.raises(ValueError, match='H0'):
        FI.fold_in(W, _sparse(3, 9), H0=torch.zeros(3, 299))
    with pytest.raises(ValueError, match='H0'):
        FI.fold_in(W, _sparse(3, 9), H0=torch.zeros(4, 300))
    with pytest.raises(ValueError):
        FI.fold_in(W[0], _sparse(3, 9))


def test_rank_before_device():
    with pytest.raises(NotImplementedError, match='256'):
        FI.fold_in(_w(R=257), _sparse(3, 9))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):               # admitted: the next check answers
        FI.fold_in(_w(R=256), _sparse(3, 9))


def test_no_cpu_fallback_before_the_data_is_read():
    W = _w()
    neg = _sparse(3, 9, (-1.0, 0.0))            # a negative and a zero stored value: not looked at before the device check
    for kw in (dict(beta=-1, unstored='missing'), dict(beta=0), dict(beta=0.5), dict(H0=-torch.ones(3, 4)), dict(max_iter=0)):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            FI.fold_in(W, neg, **kw)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        FI.fold_in(W.double(), _sparse(3, 9), unstored='missing')


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in ('nmfmu_fold_in', 'nmfmu_fold_in_block'):
        assert name in _capi.SIGNATURES and hasattr(raw, name) and name + '(' in hdr
    res, args = _capi.SIGNATURES['nmfmu_fold_in']
    assert res is ctypes.c_int and len(args) == 21
    assert [i for i, a in enumerate(args) if a is ctypes.c_float] == [8, 11, 12, 13, 15]
    assert 'NMFMU_FOLD_MISSING 0' in hdr and 'NMFMU_FOLD_ZERO 1' in hdr
    assert '#define NMFMU_ABI_VERSION 10' in hdr and 'nmfmu_fold_in / nmfmu_fold_in_block' in hdr


def test_default_block():
    lib = _capi.load()
    for bad in (0, -1, 257):
        assert lib.nmfmu_fold_in_block(bad) == 0
    prev = 64
    for R in range(1, 257):
        b = lib.nmfmu_fold_in_block(R)
        rl = 1 if R <= 64 else (2 if R <= 128 else 4)
        per_wave = (b * ((R | 1) + 2) + 64 * rl + 3) & ~3
        assert 1 <= b <= 64 and 4 * per_wave + 4 * 2 * 64 * rl <= 16384           # the workgroup's 64 KiB of LDS
        assert b <= prev or R in (65, 129)                                        # (a new RL moves the fixed part)
        assert b == E.default_block(R) == FI.default_block(R)                     # the tests' model of the thresholds
        prev = b
    assert lib.nmfmu_fold_in_block(3) == 64 and lib.nmfmu_fold_in_block(33) == 64
    assert lib.nmfmu_fold_in_block(256) >= 8


def test_c_entry_refuses_before_device_work():
    lib = _capi.load()
    buf = ctypes.create_string_buffer(64)
    buf2 = ctypes.create_string_buffer(64)
    p, q = ctypes.addressof(buf), ctypes.addressof(buf2)      # never dereferenced: every call below is answered on its arguments
    ok = dict(rowptr=p, colidx=p, vals=p, n_rows=3, H=p, W=q, n_cols=9, rank=8, beta=1.0, mode=0, aux=None, l1=0.0, l2=0.0,
              gamma=1.0, max_iter=5, tol=0.0, n_iter=None, order=None, block=0, long_rows=0, stream=None)

    def call(**kw):
        return lib.nmfmu_fold_in(*{**ok, **kw}.values())
    for kw in (dict(rowptr=None), dict(colidx=None), dict(vals=None), dict(H=None), dict(W=None), dict(rank=0), dict(rank=-3),
               dict(n_rows=-1), dict(n_cols=0), dict(max_iter=-1), dict(tol=-1e-3), dict(tol=float('nan')), dict(mode=2),
               dict(mode=-1), dict(block=-1), dict(long_rows=-1), dict(mode=1), dict(mode=1, beta=2.0)):
        assert call(**kw) == _capi.ERR_ARG, kw                                    # (zero mode without aux: a null pointer)
    assert call(rank=257) == _capi.ERR_UNSUPPORTED
    for beta in (0.5, 3.0, 0.0, -1.0):
        assert call(mode=1, aux=p, beta=beta) == _capi.ERR_UNSUPPORTED
        assert call(mode=0, beta=beta, n_rows=0) == _capi.OK                      # missing: every beta
    assert call(rank=257, H=None) == _capi.ERR_ARG
    # nothing to do: no launch, H untouched
    before = bytes(buf)
    for kw in (dict(n_rows=0), dict(max_iter=0), dict(n_rows=0, mode=1, aux=p), dict(max_iter=0, mode=1, aux=p, beta=2.0)):
        assert call(**kw) == _capi.OK, kw
    assert bytes(buf) == before
    assert call(n_rows=0, rank=257) == _capi.ERR_UNSUPPORTED                      # the refusals come first


# ---- the models ---------------------------------------------------------------------------------------------------------------
def test_which_models_transform():
    assert callable(getattr(NMF, 'transform'))
    for cls in (NMFD, NMF2D, NMF3D, PLCA, SIPLCA):
        assert not hasattr(cls, 'transform')


def test_module_untouched_by_refused_calls():
    m = NMF((6, 9), rank=4)
    W0, H0 = m.W.detach().clone(), m.H.detach().clone()
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.transform(_sparse(3, 9), unstored='missing')
    with pytest.raises(ValueError, match='unstored'):
        m.transform(_sparse(3, 9), unstored='nothing')
    with pytest.raises(ValueError, match='columns'):
        m.transform(_sparse(3, 8))
    assert torch.equal(m.W, W0) and torch.equal(m.H, H0)
    assert m.W.requires_grad and m.H.requires_grad and m.W.grad is None and sorted(dict(m.named_parameters())) == ['H', 'W']
