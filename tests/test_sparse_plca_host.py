"""PLCA on sparse targets without a GPU: the argument errors of the two C entries (every call returns before a launch), the
workspace rule, the unchanged ABI number, the validation order of ``PLCA.fit`` on CPU sparse tensors, the refusal of the
shift-invariant models and the M-step helper the dense and the sparse EM state share."""
import inspect

import pytest
import torch

from torchnmf_amd import _capi, plca
from torchnmf_amd import sparse_autograd as SA
from torchnmf_amd.plca import PLCA, SIPLCA, SIPLCA2, SIPLCA3

P = 0x1000          # a non-null pointer no call below may dereference


def _estep(lib, **kw):
    a = dict(seg=P, n_seg=4, multi=None, n_multi=0, colidx=P, vals_n=P, owner=P, z=P, panel=P, rank=5, g_out=P, ws=None, num=P,
             r_pad=32)
    a.update(kw)
    return lib.nmfmu_sp_plca_estep(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['colidx'], a['vals_n'], a['owner'], a['z'],
                                   a['panel'], a['rank'], a['g_out'], a['ws'], a['num'], a['r_pad'], None)


def _gather(lib, **kw):
    a = dict(seg=P, n_seg=4, multi=None, n_multi=0, rowidx=P, perm=P, g=P, panel=P, rank=5, ws=None, num=P, r_pad=32)
    a.update(kw)
    return lib.nmfmu_sp_plca_gather(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['rowidx'], a['perm'], a['g'], a['panel'],
                                    a['rank'], a['ws'], a['num'], a['r_pad'], None)


@pytest.mark.parametrize('call,pointers', [(_estep, ('seg', 'colidx', 'vals_n', 'owner', 'z', 'panel', 'g_out', 'num')),
                                           (_gather, ('seg', 'rowidx', 'perm', 'g', 'panel', 'num'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    assert call(lib, rank=0) == _capi.ERR_ARG and call(lib, rank=-3) == _capi.ERR_ARG
    assert call(lib, n_seg=0) == _capi.ERR_ARG and call(lib, n_seg=-1) == _capi.ERR_ARG
    assert call(lib, rank=257, r_pad=256) == _capi.ERR_UNSUPPORTED
    assert call(lib, rank=300, r_pad=512) == _capi.ERR_UNSUPPORTED
    for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
        assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
    assert call(lib, n_multi=-1) == _capi.ERR_ARG
    assert call(lib, n_multi=2, multi=None, ws=P) == _capi.ERR_ARG      # split rows need their list
    assert call(lib, n_multi=2, multi=P, ws=None) == _capi.ERR_ARG      # ... and the workspace


def test_workspace_rule_is_the_autograd_one():
    lib = _capi.load()
    for n_ws in (1, 3, 17):
        for r_pad in (32, 64, 128, 256):
            assert lib.nmfmu_sp_div_backward_ws(n_ws, r_pad) == SA.workspace_floats(n_ws, r_pad) == n_ws * r_pad   # one plane
    assert SA.workspace_floats(0, 64) == 0 and SA.workspace_floats(4, 0) == 0


def test_abi_is_additive():
    assert _capi.ABI_VERSION == 10 and _capi.load().nmfmu_abi_version() == 10
    for name in ('nmfmu_sp_plca_estep', 'nmfmu_sp_plca_gather'):
        assert hasattr(_capi.load(), name) and name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES['nmfmu_sp_plca_estep'][1]) == 15 and len(_capi.SIGNATURES['nmfmu_sp_plca_gather'][1]) == 13


def _sparse(vals=(1.0, 2.0, 0.5, 3.0), N=6, Cc=5, dtype=torch.float32):
    i = torch.tensor([[0, 1, 1, 4], [0, 2, 3, 4]])
    return torch.sparse_coo_tensor(i, torch.tensor(vals, dtype=dtype), (N, Cc)).coalesce()


def test_fit_validation_order(monkeypatch):
    """1. device, 2. sign of the stored values, 3. their total, 4. the rank -- and nothing is prepared before all four."""
    m = PLCA((6, 5), rank=2)
    bad_everywhere = _sparse((-1.0, 0.0, 0.0, 0.0))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):       # the device check comes before the sign
        m.fit(bad_everywhere)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(_sparse())
    # past the device check (switched off): the remaining three, in order, before SparseTarget -- whose constructor insists on
    # the device -- is reached
    monkeypatch.setattr(plca, '_require_device', lambda t, what: None)
    wide = PLCA((6, 5), rank=300)
    with pytest.raises(AssertionError, match='Target should be non-negative'):
        wide.fit(_sparse((-1.0, 0.0, 0.0, 0.0)))
    with pytest.raises(ValueError, match='sum to 0'):
        wide.fit(_sparse((0.0, 0.0, 0.0, 0.0)))
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        wide.fit(_sparse())
    with pytest.raises(NotImplementedError, match='rank 257 > 256'):
        PLCA((6, 5), rank=257).fit(_sparse(dtype=torch.float64))
    with pytest.raises(_capi.NmfmuError, match='SparseTarget'):          # all four passed: now the target is prepared
        m.fit(_sparse())
    with pytest.raises(AssertionError, match='does not match'):
        PLCA((7, 5), rank=2).fit(_sparse())


def test_shift_invariant_models_refuse_sparse_targets():
    for m, shape in ((SIPLCA((1, 5, 8), 2, 3), (1, 5, 8)), (SIPLCA2((1, 2, 6, 7), 2, 2), (1, 2, 6, 7)),
                     (SIPLCA3((1, 2, 4, 5, 6), 2, 2), (1, 2, 4, 5, 6))):
        with pytest.raises(NotImplementedError, match='sparse targets are supported by PLCA only'):
            m.fit(torch.rand(*shape).to_sparse())


def test_dense_targets_do_not_take_the_sparse_branch():
    assert not plca._is_sparse_target(torch.rand(3, 4)) and plca._is_sparse_target(torch.rand(3, 4).to_sparse())
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        PLCA((6, 5), rank=2).fit(_sparse().to_dense())


def test_both_em_states_share_the_m_step():
    assert issubclass(plca._PlcaEM, plca._PlcaMStep) and issubclass(plca._SparsePlcaEM, plca._PlcaMStep)
    for cls in (plca._PlcaEM, plca._SparsePlcaEM):
        assert '_m_step' not in vars(cls) and 'self._m_step(' in inspect.getsource(cls.em_step)
    # the sparse state packs no images
    src = inspect.getsource(plca._SparsePlcaEM)
    assert 'FactorBuf' not in src and 'def repack' not in src and 'pack_x' not in src and 'nmfmu_pack' not in src
