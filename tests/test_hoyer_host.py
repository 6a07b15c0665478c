"""Host side of the Hoyer entry points (no GPU): constructor checks and group state of trainer.SparsityProj, the missing CPU
path of hoyer_project / SparsityProj.step / sparse_fit, argument checking of the C entries (every call returns before a launch)."""
import pytest
import torch

from torchnmf_amd import _capi, hoyer
from torchnmf_amd.nmf import NMF
from torchnmf_amd.trainer import SparsityProj


@pytest.mark.parametrize('sparsity', [0, 1, -0.5, 1.5])
def test_sparsity_outside_open_unit_interval(sparsity):
    with pytest.raises(ValueError):
        SparsityProj([torch.nn.Parameter(torch.rand(4, 3))], sparsity)


def test_constructor_group_state():
    p = torch.nn.Parameter(torch.rand(4, 3))
    opt = SparsityProj([p], 0.3)
    g, = opt.param_groups
    assert g['lr'] == 1 and g['dim'] == 1 and g['max_iter'] == 10 and g['sparsity'] == 0.3
    g, = SparsityProj([p], 0.6, dim=0, max_iter=4).param_groups
    assert g['lr'] == 1 and g['dim'] == 0 and g['max_iter'] == 4 and g['sparsity'] == 0.6


def test_no_cpu_path():
    x = torch.rand(6, 3)
    with pytest.raises(_capi.NmfmuError):
        hoyer.hoyer_project(x, 1.0, 1.0)
    with pytest.raises(_capi.NmfmuError):
        hoyer.project_(x, 1.0, 1.0)
    p = torch.nn.Parameter(x.clone())
    opt = SparsityProj([p], 0.3)
    calls = []

    def closure():
        calls.append(1)
        return (p * p).sum()
    with pytest.raises(_capi.NmfmuError):
        opt.step(closure)
    assert not calls and torch.equal(p.data, x)          # refused before anything was evaluated or changed
    # sparse_fit keeps answering NotImplementedError off the device (the pin of test_host_logic.py::test_no_cpu_fallback)
    m = NMF((20, 30), 4)
    with pytest.raises(NotImplementedError, match='sparse_fit has no CPU path'):
        m.sparse_fit(torch.rand(20, 30))
    with pytest.raises(NotImplementedError, match='sparse_fit has no CPU path'):
        m.sparse_fit(torch.rand(20, 30), sW=0.4)
    assert not isinstance(NotImplementedError('x'), _capi.NmfmuError)


def test_public_names():
    assert hoyer.__all__ == ['hoyer_project']
    from torchnmf_amd import nmf, trainer
    assert nmf.__all__ == ['BaseComponent', 'NMF', 'NMFD', 'NMF2D', 'NMF3D'] and 'SparsityProj' in trainer.__all__


def test_slice_norms():
    x = torch.rand(5, 3, 4, dtype=torch.float64)
    for dim in (0, 1, 2, -1):
        want = torch.stack([x.select(dim, j).norm() for j in range(x.shape[dim])])
        assert torch.allclose(hoyer.slice_norms(x, dim), want, rtol=1e-14)


def test_c_entry_argument_checks():
    """nmfmu_hoyer_project_ws is host code; nmfmu_hoyer_project rejects these before touching a device."""
    lib = _capi.load()
    ws = lib.nmfmu_hoyer_project_ws
    assert ws(4096, 128, 1, hoyer.LDS_MAX_ELEMS) == 0                       # slice in LDS
    assert ws(65536, 128, 1, hoyer.LDS_MAX_ELEMS) == 65536 * 128 * 4        # streamed from a slice-major copy
    assert ws(300, 5, 1, 256) == 300 * 5 * 4 and ws(100, 5, 3, 256) == 300 * 5 * 4
    assert ws(1, 128, 65536, 0) == 0 and ws(65536, 1, 1, 0) == 0            # slice-major already: streamed in place
    assert ws(hoyer.LDS_MAX_ELEMS, 2, 1, 0) == 0 and ws(hoyer.LDS_MAX_ELEMS + 1, 2, 1, 0) > 0
    assert ws(hoyer.LDS_MAX_ELEMS + 1, 2, 1, 1 << 30) > 0                   # a request above the built maximum is clamped
    assert ws(1 << 31, 1, 1, 0) == _capi.ERR_UNSUPPORTED and ws(1 << 16, 2, 1 << 15, 0) == _capi.ERR_UNSUPPORTED
    assert ws(4, 0, 1, 0) == _capi.ERR_UNSUPPORTED and ws(0, 3, 1, 0) == _capi.ERR_ARG and ws(3, 3, 0, 0) == _capi.ERR_ARG
    f = lib.nmfmu_hoyer_project
    assert f(None, 1 << 31, 1, 1, None, None, 0, None, None, None) == _capi.ERR_UNSUPPORTED
    assert f(None, 4, 0, 1, None, None, 0, None, None, None) == _capi.ERR_UNSUPPORTED
    assert f(None, 4, 2, 1, None, None, 0, None, None, None) == _capi.ERR_ARG
