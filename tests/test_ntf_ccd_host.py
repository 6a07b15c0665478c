"""``NTF.fit(solver='ccd')``, ``ntf_ccd_sweep`` and ``nmfmu_sp_ntf_ccd_sweep`` without a GPU: the refusals in their order before
the device is asked, the new names, and the status codes the C entry answers on pointers that are never dereferenced."""
import os
import re

import pytest
import torch

from torchnmf_amd import _capi, ntf

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_in_their_order_then_the_device():
    V = torch.rand(4, 5, 6) + 0.1
    S = V.to_sparse()
    m, W = ntf.NTF(V.shape, rank=2), torch.ones(4, 5, 6)
    with pytest.raises(ValueError, match="solver must be 'mu' or 'hals', or 'ccd' on a sparse target"):
        m.fit(V, beta=1, weights=W, unstored='zero', solver='cd')
    with pytest.raises(NotImplementedError, match="solver='ccd'.*beta = 2"):
        m.fit(V, beta=1, weights=W, unstored='zero', solver='ccd')
    with pytest.raises(NotImplementedError, match="solver='ccd' takes no weights"):
        m.fit(V, beta=2, weights=W, unstored='zero', solver='ccd')
    for kw in ({'unstored': 'zero'}, {}, {'unstored': 'nothing'}):            # 'zero' and a dense target have solver='hals'
        for target in (S, V):
            with pytest.raises(NotImplementedError, match="unstored='missing'.*solver='hals'"):
                m.fit(target, beta=2, solver='ccd', precision='bf16', tile='tall', **kw)
    with pytest.raises(NotImplementedError, match="missing.*solver='mu' or solver='ccd'"):      # HALS points here now
        m.fit(S, beta=2, unstored='missing', solver='hals')
    with pytest.raises(ValueError, match='precision must be'):                # the existing checks follow
        m.fit(S, beta=2, unstored='missing', solver='ccd', precision='bf16', tile='tall')
    with pytest.raises(ValueError, match='tile must be'):
        m.fit(S, beta=2, unstored='missing', solver='ccd', tile='tall')
    with pytest.raises(NotImplementedError, match='one kernel'):
        m.fit(S, beta=2, unstored='missing', solver='ccd', tile='short')
    with pytest.raises(ValueError, match='sparse COO target'):                # a dense V with 'missing'
        m.fit(V, beta=2, unstored='missing', solver='ccd')
    keep = [f.detach().clone() for f in m.factors]
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(S, beta=2, unstored='missing', solver='ccd', alpha=0.1, l1_ratio=0.5)
    fs = [f.detach() for f in m.factors]
    with pytest.raises(ValueError, match='mode must be'):
        ntf.ntf_ccd_sweep(S, fs, 3)
    with pytest.raises(ValueError, match='3-D sparse-COO'):
        ntf.ntf_ccd_sweep(V, fs, 0)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ntf.ntf_ccd_sweep(S, fs, 0, _limit=999, _vec=7)
    assert all(torch.equal(f.detach(), k) for f, k in zip(m.factors, keep))


def test_the_name_is_declared_bound_and_exported():
    lib, name = _capi.load(), 'nmfmu_sp_ntf_ccd_sweep'
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)
    assert 'ntf_ccd_sweep' in ntf.__all__ and callable(ntf.ntf_ccd_sweep)
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    mk = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'nmfmu_sparse_ntf_ccd.hip' in mk.split('SRCS', 1)[1].split('\n', 1)[0]


KEYS = ('rowptr', 'idx_a', 'idx_b', 'vals', 'order', 'n_rows', 'owner', 'pa', 'rows_a', 'pb', 'rows_b', 'rank', 'l1', 'l2',
        'scratch', 'limit', 'wg_rows', 'vec')
ARG, UNS = _capi.ERR_ARG, _capi.ERR_UNSUPPORTED


@pytest.mark.parametrize('kw, want', [
    ({'rowptr': None}, ARG), ({'idx_a': None}, ARG), ({'idx_b': None}, ARG), ({'vals': None}, ARG), ({'owner': None}, ARG),
    ({'pa': None}, ARG), ({'pb': None}, ARG), ({'scratch': None}, ARG), ({'pa': P + 448}, ARG), ({'pb': P + 448}, ARG),
    ({'n_rows': 0}, ARG), ({'n_rows': -1}, ARG), ({'rows_a': 0}, ARG), ({'rows_b': -2}, ARG), ({'rank': 0}, ARG),
    ({'rank': -2}, ARG), ({'limit': -1}, ARG), ({'limit': 513}, ARG), ({'wg_rows': -1}, ARG), ({'vec': -1}, ARG), ({'vec': 3}, ARG),
    ({'rank': 257}, UNS), ({'rank': 1 << 20, 'order': None}, UNS),
    ({'rank': 300, 'owner': None}, ARG), ({'rank': 257, 'limit': 600}, ARG)], ids=str)      # the order of the checks
def test_c_entry_refuses_before_device_work(kw, want):
    ok = dict(rowptr=P, idx_a=P + 64, idx_b=P + 128, vals=P + 192, order=P + 256, n_rows=3, owner=P + 448, pa=P + 512, rows_a=5,
              pb=P + 576, rows_b=7, rank=4, l1=0.0, l2=0.0, scratch=P + 640, limit=0, wg_rows=0, vec=0)
    a = dict(ok, **kw)
    assert _capi.load().nmfmu_sp_ntf_ccd_sweep(*(a[k] for k in KEYS), None) == want
