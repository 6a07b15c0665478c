"""NTF without a GPU: the refusals of ``NTF`` / ``NTF.fit`` come before any device work, every C entry answers bad arguments
with its error code on pointers that are never dereferenced, and the split / workspace rules are pure and consistent."""
import os
import re

import pytest
import torch

from torchnmf_amd import _capi, ntf

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('nmfmu_ntf_nsplit', 'nmfmu_ntf_ws', 'nmfmu_ntf_terms', 'nmfmu_ntf_step', 'nmfmu_ntf_loss_parts', 'nmfmu_ntf_loss')


def _terms(lib, **kw):
    a = dict(dict(V=P, M=None, I=131, J=6, K=11, mode=0, owner=P, pa=P + 64, pb=P + 128, rank=5, r_pad=32, nsplit=0, ws=P, num=P, den=P), **kw)
    return lib.nmfmu_ntf_terms(a['V'], a['M'], a['I'], a['J'], a['K'], a['mode'], a['owner'], a['pa'], a['pb'], a['rank'],
                               a['r_pad'], 1.0, a['nsplit'], a['ws'], a['num'], a['den'], None)


def _step(lib, **kw):
    a = dict(dict(V=P, M=None, I=131, J=6, K=11, mode=0, owner=P, pa=P + 64, pb=P + 128, rank=5, r_pad=32, nsplit=0, ws=P), **kw)
    return lib.nmfmu_ntf_step(a['V'], a['M'], a['I'], a['J'], a['K'], a['mode'], a['owner'], a['pa'], a['pb'], a['rank'],
                              a['r_pad'], 1.0, 0.0, 0.0, 1.0, a['nsplit'], a['ws'], None)


def _loss(lib, **kw):
    a = dict(dict(V=P, M=None, I=131, J=6, K=11, owner=P, pa=P + 64, pb=P + 128, rank=5, part=P, out=P), **kw)
    return lib.nmfmu_ntf_loss(a['V'], a['M'], a['I'], a['J'], a['K'], a['owner'], a['pa'], a['pb'], a['rank'], 1.0, 0.0,
                              a['part'], a['out'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('V', 'owner', 'pa', 'pb', 'ws', 'num', 'den')),
                                           (_step, ('V', 'owner', 'pa', 'pb', 'ws')),
                                           (_loss, ('V', 'owner', 'pa', 'pb', 'part', 'out'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    for dim in 'IJK':
        assert call(lib, **{dim: 0}) == _capi.ERR_ARG and call(lib, **{dim: -2}) == _capi.ERR_ARG
    assert call(lib, rank=0) == _capi.ERR_ARG
    r256 = {} if call is _loss else {'r_pad': 256}
    assert call(lib, rank=257, **r256) == call(lib, rank=300, **r256) == _capi.ERR_UNSUPPORTED
    assert call(lib, I=1, J=1 << 16, K=1 << 15) == _capi.ERR_UNSUPPORTED          # a contraction past 2^30 steps
    if call is not _loss:
        for mode in (-1, 3):
            assert call(lib, mode=mode) == _capi.ERR_ARG
        for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
            assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
        assert call(lib, nsplit=-1) == _capi.ERR_ARG
        assert call(lib, J=1 << 12, K=1 << 10, nsplit=70000) == _capi.ERR_UNSUPPORTED      # 65536 parts: past grid.z
    if call is _step:
        assert call(lib, pa=P) == _capi.ERR_ARG and call(lib, pb=P) == _capi.ERR_ARG      # the owner aliases a panel factor


def test_split_and_workspace_rules():
    lib = _capi.load()
    for rows, contraction in [(131, 66), (6, 1441), (2, 490), (8, 1025 * 8192), (1025, 8 * 8192), (8192, 8200), (512, 262144),
                              (1, 1), (128, 32), (129, 33), (100000, 100)]:
        stages = -(-contraction // 32)
        for r_pad in (32, 64, 128, 256):
            auto = lib.nmfmu_ntf_nsplit(rows, contraction, r_pad)
            tiles = -(-rows // 128) * -(-r_pad // 128)
            assert 1 <= auto <= max(1, -(-512 // tiles)) and lib.nmfmu_ntf_nsplit(rows, contraction, r_pad) == auto
            for nsplit in (0, 1, 2, 3, 7, 1000):
                ws = lib.nmfmu_ntf_ws(rows, contraction, r_pad, nsplit)
                parts, rest = divmod(ws, 2 * rows * r_pad)
                assert rest == 0 and 1 <= parts <= stages and (nsplit == 0) <= (parts == auto)
                part_len = -(-stages // parts) * 32
                assert (parts - 1) * part_len < contraction <= parts * part_len          # no empty part
                assert nsplit or parts == 1 or part_len >= 4 * 32                       # the library's own parts: >= 4 stages
    # one small owner mode: the device is filled where wmu's rule stops at 64 parts
    assert lib.nmfmu_ntf_nsplit(8, 1025 * 8192, 32) == 512 > lib.nmfmu_wmu_nsplit(8, 1025 * 8192, 32) == 64
    for bad in ((0, 70, 32, 0), (131, 0, 32, 0), (131, 70, 0, 0), (131, 70, 32, -1)):
        assert lib.nmfmu_ntf_ws(*bad) == 0
    assert lib.nmfmu_ntf_nsplit(0, 70, 32) == _capi.ERR_ARG and lib.nmfmu_ntf_loss_parts(131, 0, 5) == _capi.ERR_ARG
    assert lib.nmfmu_ntf_loss_parts(131, 6, 11) == 2 and lib.nmfmu_ntf_loss_parts(8, 1025, 8192) == 512


def test_abi_is_additive():
    lib = _capi.load()
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)


def test_refusals_come_before_the_device():
    V = torch.rand(4, 5, 6) + 0.1
    m = ntf.NTF(V.shape, rank=2)
    assert m.rank == 2 and [tuple(f.shape) for f in m.factors] == [(4, 2), (5, 2), (6, 2)] and tuple(m().shape) == (4, 5, 6)
    with pytest.raises(ValueError, match='dense 3-D tensor'):
        m.fit(V.numpy())
    with pytest.raises(NotImplementedError, match="unstored='missing'"):
        m.fit(V.to_sparse())
    for bad in (torch.rand(4, 5), torch.rand(4, 5, 6, 2)):
        with pytest.raises(NotImplementedError, match='order 3'):
            m.fit(bad)
    with pytest.raises(NotImplementedError, match='order 3'):
        ntf.NTF((4, 5), rank=2)
    with pytest.raises(ValueError, match='does not match'):
        m.fit(torch.rand(4, 6, 5))
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        ntf.NTF(V.shape, rank=300).fit(V)
    with pytest.raises(ValueError, match='shape of V'):
        m.fit(V, weights=torch.ones(4, 5))
    with pytest.raises(ValueError, match='finite and non-negative'):
        m.fit(V, weights=-torch.ones(4, 5, 6))
    for w in (None, torch.ones(4, 5, 6), torch.ones(4, 5, 6) > 0):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, weights=w)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):      # before the target is scanned: -1 is never seen
        ntf.ntf_loss(-V, None, list(m.factors), 1)
    with pytest.raises(NotImplementedError, match='2\\^30'):
        ntf.NTF(factors=[torch.ones(d, 1) for d in (1, 1 << 16, 1 << 15)]).fit(torch.ones(1).expand(1, 1 << 16, 1 << 15))
    assert __import__('torchnmf_amd').ntf is ntf


def test_target_flags_and_v_term():
    """The flags look at weighted entries only; the terms of v alone against their float64 statement."""
    g = torch.Generator().manual_seed(1)
    V = torch.rand(3, 4, 5, generator=g) + 0.1
    M = torch.rand(3, 4, 5, generator=g) * (torch.rand(3, 4, 5, generator=g) > 0.3)
    V[M == 0] = float('nan')
    T = ntf.NtfTarget(V, M)
    assert (T.bad, T.has_zero) == (False, False)
    vd, md, e = torch.where(M > 0, V, torch.ones(())).double(), M.double(), ntf.eps
    want = {2.0: 0.0, 1.0: (md * (vd * (vd + e).log() - vd)).sum(), 0.0: (md * (-(vd + e).log() - 1)).sum(),
            0.5: (md * vd.sqrt()).sum(), -1.0: (md / (vd + e)).sum()}
    for beta, t in want.items():
        assert T.v_term(beta) == pytest.approx(float(t), rel=1e-13)
    U = ntf.NtfTarget(torch.where(M > 0, V, torch.zeros(())))           # unweighted: every entry counts
    assert (U.bad, U.has_zero) == (False, True) and ntf.NtfTarget(-V, M).bad
