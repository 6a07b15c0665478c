"""``NTF.fit(solver='hals')`` and ``nmfmu_ntf_mttkrp`` without a GPU: the refusals in their order before the device is asked, the
new names, and the status codes the C entry answers before any launch on pointers that are never dereferenced."""
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
    with pytest.raises(ValueError, match="solver must be 'mu' or 'hals'"):
        m.fit(V, beta=1, weights=W, unstored='missing', solver='cd')
    with pytest.raises(NotImplementedError, match='beta = 2'):
        m.fit(V, beta=1, weights=W, unstored='missing', solver='hals')
    with pytest.raises(NotImplementedError, match="no weights.*solver='mu'"):
        m.fit(V, beta=2, weights=W, unstored='missing', solver='hals')
    with pytest.raises(NotImplementedError, match="missing.*solver='mu'"):
        m.fit(V.to_sparse(), beta=2, unstored='missing', solver='hals')
    with pytest.raises(ValueError, match='tile must be'):                      # the existing checks follow
        m.fit(V, beta=2, solver='hals', tile='tall')
    with pytest.raises(NotImplementedError, match='one kernel'):
        m.fit(V.to_sparse(), beta=2, unstored='zero', solver='hals', tile='short')
    for kw in ({}, {'tile': 'short'}):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, beta=2, solver='hals', **kw)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(V.to_sparse(), beta=2, unstored='zero', solver='hals')
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ntf.ntf_mttkrp(V, list(m.factors), 0)
    with pytest.raises(ValueError, match='dense 3-D tensor'):
        ntf.ntf_mttkrp(V.to_sparse(), list(m.factors), 0)


def _mttkrp(lib, **kw):
    a = dict(dict(V=P, I=131, J=6, K=11, mode=0, pa=P + 64, pb=P + 128, rank=5, r_pad=32, nsplit=0, tile=0, ws=P, num=P), **kw)
    return lib.nmfmu_ntf_mttkrp(a['V'], a['I'], a['J'], a['K'], a['mode'], a['pa'], a['pb'], a['rank'], a['r_pad'], a['nsplit'],
                                a['tile'], a['ws'], a['num'], None)


def test_names_and_status_codes():
    lib = _capi.load()
    assert 'ntf_mttkrp' in ntf.__all__ and callable(ntf.ntf_mttkrp)
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in ('nmfmu_ntf_mttkrp', 'nmfmu_ntf_mttkrp_ws'):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)
    assert _mttkrp(lib, rank=257, r_pad=256) == _capi.ERR_UNSUPPORTED
    assert _mttkrp(lib, I=1, J=1 << 16, K=1 << 15) == _capi.ERR_UNSUPPORTED          # a contraction past 2^30 steps
    assert _mttkrp(lib, J=1 << 12, K=1 << 10, nsplit=70000) == _capi.ERR_UNSUPPORTED      # 65536 parts: past grid.z
    for bad in ({'mode': 3}, {'mode': -1}, {'V': None}, {'pa': None}, {'pb': None}, {'ws': None}, {'num': None}, {'I': 0},
                {'rank': 0}, {'r_pad': 64}, {'nsplit': -1}, {'tile': 2}):
        assert _mttkrp(lib, **bad) == _capi.ERR_ARG, bad
    # the workspace: parts of whole stages (32 steps wide, 128 short), no empty part; one plane per part
    for rows, contraction in ((131, 66), (6, 1441), (8, 1025 * 8192), (512, 262144), (1, 1)):
        for r_pad in (32, 256):
            for tile, stage in ((0, 32), (1, 128)):
                for nsplit in (0, 1, 3, 1000):
                    parts, rest = divmod(lib.nmfmu_ntf_mttkrp_ws(rows, contraction, r_pad, nsplit, tile), rows * r_pad)
                    stages = -(-contraction // stage)
                    assert rest == 0 and 1 <= parts <= stages and (parts - 1) * -(-stages // parts) < stages
                    assert nsplit == 0 or parts <= nsplit
    assert lib.nmfmu_ntf_mttkrp_ws(0, 70, 32, 0, 0) == 0 and lib.nmfmu_ntf_mttkrp_ws(131, 70, 32, 0, 2) == 0
