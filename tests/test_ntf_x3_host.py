"""``precision='bf16x3'`` and ``nmfmu_ntf_mttkrp_x3`` without a GPU: the refusals in their order before the device is asked, the
new name, and the status codes of the C entry side by side with ``nmfmu_ntf_mttkrp``'s on pointers that are never dereferenced."""
import os
import re

import pytest
import torch

from torchnmf_amd import _capi, ntf

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_in_their_order_then_the_device():
    V = torch.rand(4, 5, 6) + 0.1
    m, W = ntf.NTF(V.shape, rank=2), torch.ones(4, 5, 6)
    with pytest.raises(ValueError, match="solver must be 'mu' or 'hals'"):       # the solver checks come first
        m.fit(V, beta=2, solver='cd', precision='bf16')
    with pytest.raises(NotImplementedError, match="no weights.*solver='mu'"):
        m.fit(V, beta=2, weights=W, solver='hals', precision='bf16')
    with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16x3'"):
        m.fit(V, beta=2, solver='hals', precision='bf16', tile='tall')
    with pytest.raises(NotImplementedError, match="solver='mu' is exact fp32 only"):
        m.fit(V, beta=2, precision='bf16x3', tile='tall')
    with pytest.raises(NotImplementedError, match="solver='mu' is exact fp32 only"):
        m.fit(V, beta=2, weights=W, precision='bf16x3')
    with pytest.raises(NotImplementedError, match='sparse targets are exact fp32 only'):
        m.fit(V.to_sparse(), beta=2, unstored='zero', solver='hals', precision='bf16x3', tile='short')
    with pytest.raises(ValueError, match='tile must be'):                        # the existing checks follow
        m.fit(V, beta=2, solver='hals', precision='bf16x3', tile='tall')
    for kw in ({}, {'tile': 'short'}):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, beta=2, solver='hals', precision='bf16x3', **kw)
    with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16x3'"):
        ntf.ntf_mttkrp(V, list(m.factors), 0, precision='bf16')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ntf.ntf_mttkrp(V, list(m.factors), 0, precision='bf16x3')


def test_the_name_is_declared_bound_and_exported():
    lib, name = _capi.load(), 'nmfmu_ntf_mttkrp_x3'
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    assert hasattr(lib, name) and re.search(r'\b' + name + r'\(', hdr)
    assert _capi.SIGNATURES[name] == _capi.SIGNATURES['nmfmu_ntf_mttkrp']


@pytest.mark.parametrize('kw', [
    {'rank': 257, 'r_pad': 256}, {'I': 1, 'J': 1 << 16, 'K': 1 << 15}, {'J': 1 << 12, 'K': 1 << 10, 'nsplit': 70000},
    {'mode': 3}, {'mode': -1}, {'V': None}, {'pa': None}, {'pb': None}, {'ws': None}, {'num': None}, {'I': 0}, {'rank': 0},
    {'r_pad': 64}, {'nsplit': -1}, {'tile': 2},
    {'ws': None, 'rank': 257}, {'tile': 2, 'I': 1, 'J': 1 << 16, 'K': 1 << 15}, {'rank': 257, 'r_pad': 64, 'mode': 3}], ids=str)
def test_status_codes_are_those_of_the_fp32_entry(kw):
    """Every bad argument test_ntf_hals_host tries, and three pairs of them that show the order of the checks."""
    lib = _capi.load()
    a = dict(dict(V=P, I=131, J=6, K=11, mode=0, pa=P + 64, pb=P + 128, rank=5, r_pad=32, nsplit=0, tile=0, ws=P, num=P), **kw)
    args = [a[k] for k in ('V', 'I', 'J', 'K', 'mode', 'pa', 'pb', 'rank', 'r_pad', 'nsplit', 'tile', 'ws', 'num')] + [None]
    rc = lib.nmfmu_ntf_mttkrp_x3(*args)
    assert rc == lib.nmfmu_ntf_mttkrp(*args) and rc in (_capi.ERR_ARG, _capi.ERR_UNSUPPORTED)
