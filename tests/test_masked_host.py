"""Missing-data NMF without a GPU: the argument errors of the three C entries and of the workspace rule (every call returns
before a launch), the validation order of ``unstored``, and the work lists the W side reads."""
import ctypes as C

import pytest
import torch

from torchnmf_amd import _capi
from torchnmf_amd import sparse_autograd as SA
from torchnmf_amd.nmf import NMF, NMFD

P = 0x1000          # a non-null pointer no call below may dereference


def test_workspace_rule():
    lib = _capi.load()
    for n_ws in (1, 3, 17):
        for r_pad in (32, 64, 128, 256):
            assert lib.nmfmu_sp_masked_ws(n_ws, r_pad) == SA.masked_workspace_floats(n_ws, r_pad) == n_ws * 2 * r_pad
    assert lib.nmfmu_sp_masked_ws(0, 64) == 0 and lib.nmfmu_sp_masked_ws(-1, 64) == 0 and lib.nmfmu_sp_masked_ws(4, 0) == 0
    assert SA.masked_workspace_floats(0, 64) == 0 and SA.masked_workspace_floats(4, 0) == 0
    # twice the rule of the autograd kernels: a [num | den] pair per segment
    assert lib.nmfmu_sp_masked_ws(5, 128) == 2 * lib.nmfmu_sp_div_backward_ws(5, 128)


def _terms(lib, **kw):
    a = dict(seg=P, n_seg=4, multi=None, n_multi=0, idx=P, vals=P, owner=P, panel=P, rank=5, beta=1.0, ws=None, num=P, den=P,
             r_pad=32)
    a.update(kw)
    return lib.nmfmu_sp_masked_terms(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['idx'], a['vals'], a['owner'],
                                     a['panel'], a['rank'], a['beta'], a['ws'], a['num'], a['den'], a['r_pad'], None)


def _step(lib, **kw):
    a = dict(seg=P, n_seg=4, multi=None, n_multi=0, idx=P, vals=P, owner=P, panel=P + 64, rank=5, beta=1.0, ws=None, r_pad=32)
    a.update(kw)
    return lib.nmfmu_sp_masked_step(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['idx'], a['vals'], a['owner'],
                                    a['panel'], a['rank'], a['beta'], 0.0, 0.0, 1.0, a['ws'], a['r_pad'], None)


def _loss(lib, **kw):
    a = dict(seg=P, n_seg=4, colidx=P, vals=P, owner=P, panel=P, rank=5, beta=1.0, part=P, out=P)
    a.update(kw)
    return lib.nmfmu_sp_masked_loss(a['seg'], a['n_seg'], a['colidx'], a['vals'], a['owner'], a['panel'], a['rank'],
                                    a['beta'], 0.0, a['part'], a['out'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('seg', 'idx', 'vals', 'owner', 'panel', 'num', 'den')),
                                           (_step, ('seg', 'idx', 'vals', 'owner', 'panel')),
                                           (_loss, ('seg', 'colidx', 'vals', 'owner', 'panel', 'part', 'out'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    assert call(lib, rank=0) == _capi.ERR_ARG and call(lib, rank=-3) == _capi.ERR_ARG
    assert call(lib, n_seg=0) == _capi.ERR_ARG
    assert call(lib, rank=257, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    for beta in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0):                      # no beta is refused -- only the rank
        assert call(lib, rank=300, beta=beta, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    if call is not _loss:
        for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
            assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
        assert call(lib, n_multi=-1) == _capi.ERR_ARG
        assert call(lib, n_multi=2, multi=None, ws=P) == _capi.ERR_ARG      # split rows need their list
        assert call(lib, n_multi=2, multi=P, ws=None) == _capi.ERR_ARG      # ... and the workspace


def test_step_refuses_aliased_factors():
    assert _step(_capi.load(), owner=P, panel=P) == _capi.ERR_ARG


def test_abi_is_additive():
    # (the masked entries were added at ABI 9 without a version change; 10 is the alpha argument of the PLCA entries)
    assert _capi.ABI_VERSION == 10 and _capi.load().nmfmu_abi_version() == 10
    for name in ('nmfmu_sp_masked_ws', 'nmfmu_sp_masked_terms', 'nmfmu_sp_masked_step', 'nmfmu_sp_masked_loss'):
        assert hasattr(_capi.load(), name)
    assert _capi.load().nmfmu_sp_masked_ws.restype is C.c_int64


def _sparse(N=6, Cc=5):
    i = torch.tensor([[0, 1, 1, 4], [0, 2, 3, 4]])
    return torch.sparse_coo_tensor(i, torch.tensor([1.0, 2.0, 0.5, 3.0]), (N, Cc)).coalesce()


def test_unstored_validation_comes_first():
    """On CPU tensors: the ValueErrors are raised before the device check (which raises NmfmuError)."""
    m = NMF((6, 5), rank=2)
    Vs, Vd = _sparse(), _sparse().to_dense()
    for V in (Vs, Vd):
        with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
            m.fit(V, unstored='ignore')
    with pytest.raises(ValueError, match=r'V\.sparse_mask\(mask\)'):
        m.fit(Vd, unstored='missing')
    with pytest.raises(NotImplementedError, match='not sharded'):
        m.fit(Vs, unstored='missing', process_group=object())
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):     # past the validation: the device check
        m.fit(Vs, unstored='missing')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):     # the default is untouched
        m.fit(Vs)
    with pytest.raises(TypeError):                                     # keyword-only
        m.fit(Vs, 1, 1e-4, 200, False, 0, 0, 'missing')


def test_convolutive_models_keep_refusing_sparse_targets():
    m = NMFD((1, 5, 6), rank=2, T=2)
    V = torch.rand(1, 5, 6).to_sparse()
    with pytest.raises(NotImplementedError, match='NMF only'):
        m.fit(V, unstored='missing')


def test_sparse_beta_div_validation():
    H, W = torch.rand(6, 2), torch.rand(5, 2)
    with pytest.raises(ValueError, match="unstored must be 'zero' or 'missing'"):
        SA.sparse_beta_div(H, W, _sparse(), 1, unstored='unknown')
    with pytest.raises(ValueError, match='When beta <= 0'):            # the default path's pinned error
        SA.sparse_beta_div(H, W, _sparse(), 0)
    with pytest.raises(NotImplementedError, match=r'beta in \{1, 2\}'):
        SA.sparse_beta_div(H, W, _sparse(), 0.5)
    with pytest.raises(_capi.NmfmuError, match='ROCm device'):         # 'missing' admits the beta, then needs the device
        SA.sparse_beta_div(H, W, _sparse(), 0.5, unstored='missing')
    with pytest.raises(_capi.NmfmuError, match='ROCm device'):
        SA.sparse_beta_div(H, W, _sparse(), -1, unstored='missing')


class _T(SA.SparseTarget):
    """A SparseTarget planned on the CPU (the constructor insists on the device; the planning functions do not)."""

    def __init__(self, V, chunk):
        V = V.coalesce()
        idx, vals = V.indices(), V.values().float()
        self.shape, self.nnz, self.vals, self.chunk = tuple(V.shape), int(vals.numel()), vals, chunk
        self.csr, self.csc, self.perm = SA.csr_csc(idx[0], idx[1], vals, *V.shape)
        self.seg_h, self.multi_h, self.n_ws_h = SA.plan_worklist(self.csr[0], chunk)
        self.seg_w, self.multi_w, self.n_ws_w = SA.plan_worklist(self.csc[0], chunk)
        self._v_norm, self._has_zero = {}, None


def test_w_side_reads_the_csc_list():
    g = torch.Generator().manual_seed(3)
    dense = torch.rand(9, 40, generator=g) * (torch.rand(9, 40, generator=g) < 0.6)
    dense[:, 4] = 0
    T = _T(dense.to_sparse(), chunk=4)
    (ptr, idx, vals), seg, multi, n_ws = T.side('w')
    assert ptr is T.csc[0] and idx is T.csc[1] and vals is T.csc[2] and seg is T.seg_w and multi is T.multi_w
    assert ptr.numel() == 40 + 1 and int(idx.max()) < 9                # owner rows = columns of V, indices = rows of V
    assert torch.equal(vals, T.vals[T.perm.long()])                    # values in CSC order
    col = 7
    p0, p1 = int(ptr[col]), int(ptr[col + 1])
    assert torch.equal(vals[p0:p1], dense[:, col][dense[:, col] != 0])
    seg_w, multi_w, n = SA.plan_worklist(T.csc[0], 4)                  # the same plan_worklist, fed the column pointer
    assert torch.equal(seg, seg_w) and torch.equal(multi, multi_w) and n == n_ws
    own = seg[:, 0].long()
    assert int(own.max()) == 39 and bool(((seg[:, 2] - seg[:, 1]) <= 4).all())
    assert bool((seg[own == 4][:, 1:3] == int(ptr[4])).all()) and int((own == 4).sum()) == 1   # the empty column: one empty segment
    (ptr_h, _, vals_h), seg_h, _, _ = T.side('h')
    assert ptr_h is T.csr[0] and vals_h is T.vals and seg_h is T.seg_h
    assert T.has_zero is False
    z = torch.sparse_coo_tensor(torch.tensor([[0, 1], [0, 1]]), torch.tensor([0.0, 1.0]), (2, 2))
    assert _T(z, 4).has_zero is True                                   # a STORED zero counts; the unstored entries do not


def test_masked_v_term_matches_the_metrics():
    v = torch.tensor([0.25, 1.0, 1.5, 3.0])
    eps = 1.1920928955078125e-07
    vd = v.double()
    assert SA.masked_v_term(v, 2.0) == 0.0
    assert SA.masked_v_term(v, 1.0) == pytest.approx(float(vd @ (vd + eps).log() - vd.sum()), rel=1e-15)
    assert SA.masked_v_term(v, 0.0) == pytest.approx(float(-(vd + eps).log().sum() - 4), rel=1e-15)
    assert SA.masked_v_term(v, 0.5) == pytest.approx(float(vd.sqrt().sum()), rel=1e-15)
    assert SA.masked_v_term(v, -1.0) == pytest.approx(float((1 / (vd + eps)).sum()), rel=1e-15)
