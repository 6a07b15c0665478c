"""Host side of fold-in by coordinate descent (``fold_in_cd`` in torchnmf_amd/fold_in.py, the C entries of
csrc/nmfmu_fold_in_cd.hip): every refusal with its class, its text and its place in the order, on CPU tensors; that
``fold_in`` answers as it did before; the exported symbols and the status codes the C entry answers
before any device work.  No GPU (the checks that read the data need the device: tests/test_gpu_fold_in_cd.py)."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import ROOT
import fold_in_cd_emulation as E
from torchnmf_amd import _capi, fold_in as FI, metrics
from torchnmf_amd.nmf import NMF, NMF2D, NMF3D, NMFD
from torchnmf_amd.plca import PLCA, SIPLCA

CPU = 'no CPU fallback'


def _w(C=9, R=4):
    return torch.rand(C, R, generator=torch.Generator().manual_seed(0))


def _sparse(n=3, C=9, vals=(1.0, 0.5)):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor(vals), (n, C))


def test_signature():
    """The coordinate-descent route has entry points of its own; ``fold_in`` and ``NMF.transform`` keep their signatures."""
    assert metrics.fold_in_cd is FI.fold_in_cd and 'fold_in_cd' in metrics.__all__ and metrics.fold_in is FI.fold_in
    old = ['beta', 'max_iter', 'tol', 'alpha', 'l1_ratio', 'unstored', 'H0', 'generator', 'return_n_iter']
    new = old[:6] + ['solver'] + old[6:]
    defaults = [2, 200, 1e-4, 0, 0, 'missing', 'ccd', None, None, False]
    par = inspect.signature(FI.fold_in_cd).parameters
    assert [p for p in par if not p.startswith('_')] == ['W', 'target'] + new
    assert [p for p in par if p.startswith('_')] == ['_block', '_long_rows', '_fill']
    tpar = inspect.signature(NMF.transform_cd).parameters
    assert list(tpar) == ['self', 'V_new'] + new
    for q in (par, tpar):
        assert [q[n].default for n in new] == defaults
        assert all(q[n].kind is inspect.Parameter.KEYWORD_ONLY for n in new[5:])
    assert [p for p in inspect.signature(FI.fold_in).parameters if not p.startswith('_')] == ['W', 'target'] + old
    assert list(inspect.signature(NMF.transform).parameters) == ['self', 'V_new'] + old
    assert FI.SOLVERS == ('mu', 'hals', 'ccd')
    for cls in (NMFD, NMF2D, NMF3D, PLCA, SIPLCA):                       # they stay out
        assert not hasattr(cls, 'transform') and not hasattr(cls, 'transform_cd')
    assert 'NO initial scaling' in FI.fold_in_cd.__doc__ and 'no initial scaling' in FI.__doc__


# ---- the refusals, in order ---------------------------------------------------------------------------------------------------
def test_solver_name_comes_first():
    for bad in ('MU', 'cd', None, 2, ''):
        with pytest.raises(ValueError, match="solver must be 'mu', 'hals' or 'ccd'"):
            FI.fold_in_cd(_w(), torch.zeros(3, 9), 1, max_iter=-1, unstored='nothing', solver=bad)   # everything else is bad too


@pytest.mark.parametrize('solver', ['ccd', 'hals'])
def test_beta_before_the_reading_of_the_unstored_entries(solver):
    for beta in (1, 0.5, 0, -1, 2.5):
        for unstored in ('zero', 'missing', 0.05, 7.0, 'nothing'):
            with pytest.raises(NotImplementedError, match=f"solver='{solver}': .*closed-form only for beta = 2"):
                FI.fold_in_cd(_w(), torch.zeros(3, 9), beta, max_iter=-1, unstored=unstored, solver=solver)
    with pytest.raises(_capi.NmfmuError, match=CPU):                     # beta's default is 2: admitted as far as the device
        FI.fold_in_cd(_w(), _sparse(), solver=solver, unstored='zero' if solver == 'hals' else 'missing')


def test_ccd_refuses_zero_and_names_hals():
    for unstored in ('zero', 'nothing', None, True, False):              # (a bool is not a number: fit's rule)
        with pytest.raises(NotImplementedError, match="needs unstored='missing'.*use solver='hals'"):
            FI.fold_in_cd(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored=unstored, solver='ccd')


def test_hals_refuses_missing_and_a_weight_and_names_ccd():
    with pytest.raises(NotImplementedError, match="solver='hals'.*use solver='ccd'"):
        FI.fold_in_cd(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored='missing', solver='hals')
    for w in (0.05, 0.5):
        with pytest.raises(NotImplementedError, match="fitted by solver='ccd' only.*not by solver='hals'"):
            FI.fold_in_cd(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored=w, solver='hals')
    for bad in ('nothing', None, True):
        with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
            FI.fold_in_cd(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored=bad, solver='hals')


@pytest.mark.parametrize('solver', ['ccd', 'hals'])
def test_a_weight_outside_the_open_interval(solver):
    for bad in (0.0, 1.0, -0.1, 2, 1.5, float('nan'), float('inf'), 1e-60, 1 - 1e-12):   # (the last two are 0 and 1 in fp32)
        with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing', or \\(solver='ccd'\\) the weight of the "
                                             "unstored zeros, a real number strictly between 0 and 1"):
            FI.fold_in_cd(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored=bad, solver=solver)


@pytest.mark.parametrize('solver,unstored', [('ccd', 'missing'), ('ccd', 0.05), ('hals', 'zero')])
def test_the_shared_checks_follow_in_the_order_of_mu(solver, unstored):
    kw = dict(unstored=unstored, solver=solver)
    for bad in (torch.zeros(3, 9), [[1.0]], None):                       # the target's type before max_iter
        with pytest.raises(ValueError, match=r'sparse_mask\(mask\).*trainable_W=False'):
            FI.fold_in_cd(_w(), bad, 2, max_iter=-1, **kw)
    for bad in (-1, 2.0, None, True):                                    # max_iter and tol before the shapes
        with pytest.raises(ValueError, match='max_iter'):
            FI.fold_in_cd(_w(), _sparse(3, 8), 2, max_iter=bad, **kw)
    for bad in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='tol'):
            FI.fold_in_cd(_w(), _sparse(3, 8), 2, tol=bad, **kw)
    with pytest.raises(ValueError, match='columns'):                     # the shapes before the rank
        FI.fold_in_cd(_w(R=300), _sparse(3, 8), 2, **kw)
    with pytest.raises(ValueError, match='H0'):
        FI.fold_in_cd(_w(R=300), _sparse(), 2, H0=torch.zeros(3, 299), **kw)
    with pytest.raises(NotImplementedError, match='rank 257 > 256'):     # the rank before the device
        FI.fold_in_cd(_w(R=257), _sparse(), 2, **kw)
    neg = _sparse(vals=(-1.0, 0.0))                                      # the data is not read before the device check
    for more in (dict(), dict(H0=-torch.ones(3, 4)), dict(max_iter=0), dict(alpha=0.1, l1_ratio=0.3)):
        with pytest.raises(_capi.NmfmuError, match=CPU):
            FI.fold_in_cd(_w(), neg, 2, **more, **kw)
    with pytest.raises(_capi.NmfmuError, match=CPU):
        FI.fold_in_cd(_w(R=256), _sparse(), 2, **kw)
    with pytest.raises(_capi.NmfmuError, match=CPU):
        metrics.fold_in_cd(_w().double(), _sparse(), 2.0, **kw)


def test_transform_passes_the_solver_through():
    m = NMF((6, 9), rank=4)
    W0, H0 = m.W.detach().clone(), m.H.detach().clone()
    with pytest.raises(ValueError, match='solver must be'):
        m.transform_cd(_sparse(), 2, solver='als')
    with pytest.raises(NotImplementedError, match='closed-form only for beta = 2'):
        m.transform_cd(_sparse(), 1, solver='ccd', unstored=0.05)
    with pytest.raises(NotImplementedError, match="use solver='hals'"):
        m.transform_cd(_sparse(), 2, solver='ccd', unstored='zero')
    with pytest.raises(NotImplementedError, match="use solver='ccd'"):
        m.transform_cd(_sparse(), 2, solver='hals', unstored='missing')
    with pytest.raises(ValueError, match='strictly between 0 and 1'):
        m.transform_cd(_sparse(), 2, solver='ccd', unstored=1.0)
    for kw in (dict(solver='ccd', unstored=0.05), dict(solver='ccd', unstored='missing'), dict(solver='hals', unstored='zero')):
        with pytest.raises(_capi.NmfmuError, match=CPU):
            m.transform_cd(_sparse(), 2, **kw)
    assert torch.equal(m.W, W0) and torch.equal(m.H, H0) and m.W.grad is None


# ---- solver='mu' answers as before ----------------------------------------------------------------------------------------------
def test_mu_is_unchanged():
    """``fold_in`` / ``transform`` take no solver and answer as before: the refusals of tests/test_fold_in_host.py, in their
    order and words -- a number for ``unstored`` among them (tests/test_wccd_host.py pins that one).  ``fold_in_cd`` with
    ``solver='mu'`` is the same route."""
    with pytest.raises(TypeError):
        FI.fold_in(_w(), _sparse(), 2, solver='ccd')
    with pytest.raises(TypeError):
        NMF((6, 9), rank=4).transform(_sparse(), 2, solver='ccd')
    for f, kw in ((FI.fold_in, dict()), (FI.fold_in_cd, dict(solver='mu'))):
        for bad in (0.05, 0.5, 1, 0, True, None, 'Missing'):
            with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing', got") as e:
                f(_w(), torch.zeros(3, 9), 2, max_iter=-1, unstored=bad, **kw)
            assert 'strictly between' not in str(e.value)
        with pytest.raises(ValueError, match=r'sparse_mask\(mask\)'):
            f(_w(), torch.zeros(3, 9), 1, max_iter=-1, unstored='missing', **kw)
        with pytest.raises(ValueError, match='max_iter'):
            f(_w(), _sparse(3, 8), 1, max_iter=-1, unstored='zero', **kw)
        with pytest.raises(ValueError, match='columns'):
            f(_w(R=300), _sparse(3, 8), 1, unstored='zero', **kw)
        with pytest.raises(NotImplementedError, match='256'):
            f(_w(R=257), _sparse(), 1, unstored='zero', **kw)
        for more in (dict(beta=-1, unstored='missing'), dict(beta=0, unstored='zero'), dict(beta=0.5, unstored='zero'),
                     dict(beta=2, unstored='zero'), dict(beta=3, unstored='zero')):
            with pytest.raises(_capi.NmfmuError, match=CPU):                # any beta reaches the device check
                f(_w(), _sparse(vals=(-1.0, 0.0)), **more, **kw)
    with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing', got 0.05"):
        NMF((6, 9), rank=4).transform(_sparse(), 2, unstored=0.05)


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in ('nmfmu_fold_in_cd', 'nmfmu_fold_in_cd_block', 'nmfmu_fold_in_cd_long_rows'):
        assert name in _capi.SIGNATURES and hasattr(raw, name) and name + '(' in hdr
    C = ctypes
    res, args = _capi.SIGNATURES['nmfmu_fold_in_cd']
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                    C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert ('int nmfmu_fold_in_cd(const int32_t* rowptr, const int32_t* colidx, const float* vals, int n_rows, float* H, '
            'const float* W,\n                     int n_cols, int rank, const float* gram, float omega, float l1, float l2, '
            'int max_iter, float tol,\n                     int32_t* n_iter_rows, const int32_t* order, int block, '
            'int long_rows, void* stream);') in hdr
    assert '#define NMFMU_ABI_VERSION 10' in hdr and 'nmfmu_fold_in_cd / nmfmu_fold_in_cd_block' in hdr


def test_thresholds():
    lib = _capi.load()
    for bad in (0, -1, 257):
        assert lib.nmfmu_fold_in_cd_block(bad) == 0 and lib.nmfmu_fold_in_cd_long_rows(bad) == 0
    for R in range(1, 257):
        b, lr = lib.nmfmu_fold_in_cd_block(R), lib.nmfmu_fold_in_cd_long_rows(R)
        assert b == E.default_block(R) == FI.default_block_cd(R) and lr == E.default_long_rows(R) == FI.default_long_rows_cd(R)
        assert 1 <= lr <= b and lr <= 128
        # the wave's share of the workgroup's 40 KiB: h, D and n, the residuals, the staged W rows
        assert 3 * ((R + 63) & ~63) + ((b + 3) & ~3) + b * (R | 1) <= E.PER_WAVE and 4 * E.PER_WAVE + 16 <= 10240


def test_c_entry_refuses_before_device_work():
    lib = _capi.load()
    buf = ctypes.create_string_buffer(64)
    buf2 = ctypes.create_string_buffer(64)
    p, q = ctypes.addressof(buf), ctypes.addressof(buf2)      # never dereferenced: every call below is answered on its arguments
    ok = dict(rowptr=p, colidx=p, vals=p, n_rows=3, H=p, W=q, n_cols=9, rank=8, gram=q, omega=0.05, l1=0.0, l2=0.0, max_iter=5,
              tol=0.0, n_iter=None, order=None, block=0, long_rows=0, stream=None)

    def call(**kw):
        return lib.nmfmu_fold_in_cd(*{**ok, **kw}.values())
    for kw in (dict(rowptr=None), dict(colidx=None), dict(vals=None), dict(H=None), dict(W=None), dict(W=p), dict(rank=0),
               dict(rank=-3), dict(n_rows=-1), dict(n_cols=0), dict(max_iter=-1), dict(tol=-1e-3), dict(tol=float('nan')),
               dict(block=-1), dict(long_rows=-1), dict(omega=-0.1), dict(omega=1.5), dict(omega=float('nan')),
               dict(gram=None), dict(gram=None, omega=1.0)):
        assert call(**kw) == _capi.ERR_ARG, kw
    assert call(rank=257) == _capi.ERR_UNSUPPORTED
    assert call(rank=257, H=None) == _capi.ERR_ARG
    before = bytes(buf)
    for kw in (dict(n_rows=0), dict(max_iter=0), dict(n_rows=0, omega=0.0, gram=None), dict(max_iter=0, omega=1.0),
               dict(max_iter=0, omega=0.0, gram=None)):               # nothing to do: no launch, H untouched
        assert call(**kw) == _capi.OK, kw
    assert bytes(buf) == before
    assert call(n_rows=0, rank=257) == _capi.ERR_UNSUPPORTED             # the refusals come first
