"""Sparse NTF without a GPU: the refusals of ``NTF.fit(..., unstored=)`` in their order, the planner against a brute-force
sort, the pure rules of the C entries and every argument error on pointers that are never dereferenced."""
import os
import re

import pytest
import torch

from torchnmf_amd import _capi, ntf

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('nmfmu_sp_ntf_lds_rows', 'nmfmu_sp_ntf_ws', 'nmfmu_sp_ntf_terms', 'nmfmu_sp_ntf_step', 'nmfmu_sp_ntf_loss')
BASE = dict(seg=P, n_seg=4, multi=None, n_multi=0, idx_a=P, idx_b=P, vals=P, nnz=9, owner=P, pa=P + 64, rows_a=5, pb=P + 128,
            rows_b=6, rank=5, beta=1.0, zero=0, pos=None, plane=0, ws=None, num=P, den=P, r_pad=32, stage=0, part=P, out=P)


def _terms(lib, **kw):
    a = dict(BASE, **kw)
    return lib.nmfmu_sp_ntf_terms(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['idx_a'], a['idx_b'], a['vals'], a['nnz'],
                                  a['owner'], a['pa'], a['rows_a'], a['pb'], a['rows_b'], a['rank'], a['beta'], a['zero'],
                                  a['pos'], a['plane'], a['ws'], a['num'], a['den'], a['r_pad'], a['stage'], None)


def _step(lib, **kw):
    a = dict(BASE, **kw)
    return lib.nmfmu_sp_ntf_step(a['seg'], a['n_seg'], a['multi'], a['n_multi'], a['idx_a'], a['idx_b'], a['vals'], a['nnz'],
                                 a['owner'], a['pa'], a['rows_a'], a['pb'], a['rows_b'], a['rank'], a['beta'], a['zero'],
                                 a['pos'], a['plane'], 0.0, 0.0, 1.0, a['ws'], a['r_pad'], a['stage'], None)


def _loss(lib, **kw):
    a = dict(BASE, **kw)
    return lib.nmfmu_sp_ntf_loss(a['seg'], a['n_seg'], a['idx_a'], a['idx_b'], a['vals'], a['nnz'], a['owner'], a['pa'],
                                 a['rows_a'], a['pb'], a['rows_b'], a['rank'], a['beta'], a['zero'], 0.0, a['part'], a['out'],
                                 a['stage'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('seg', 'idx_a', 'idx_b', 'vals', 'owner', 'pa', 'pb', 'num', 'den')),
                                           (_step, ('seg', 'idx_a', 'idx_b', 'vals', 'owner', 'pa', 'pb')),
                                           (_loss, ('seg', 'idx_a', 'idx_b', 'vals', 'owner', 'pa', 'pb', 'part', 'out'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for bad in [{name: None} for name in pointers] + [dict(n_seg=0), dict(nnz=-1), dict(rows_a=0), dict(rows_b=-3), dict(rank=0),
                                                      dict(zero=2), dict(stage=-1), dict(stage=3)]:
        assert call(lib, **bad) == _capi.ERR_ARG, bad
    assert call(lib, rank=257, r_pad=256) == call(lib, rank=300, r_pad=256) == _capi.ERR_UNSUPPORTED
    for beta in (0.0, 0.5, 3.0):
        assert call(lib, zero=1, pos=P, beta=beta) == _capi.ERR_UNSUPPORTED
    if call is not _loss:
        assert call(lib, zero=1, pos=None) == _capi.ERR_ARG
        for bad in (dict(n_multi=-1), dict(n_multi=2, multi=None, ws=P), dict(n_multi=2, multi=P, ws=None), dict(r_pad=64),
                    dict(rank=100, r_pad=256), dict(r_pad=0)):
            assert call(lib, **bad) == _capi.ERR_ARG, bad
    if call is _step:
        assert call(lib, pa=P) == _capi.ERR_ARG and call(lib, pb=P) == _capi.ERR_ARG      # the owner aliases a panel factor


def test_pure_rules_and_names():
    lib = _capi.load()
    for rank in (1, 3, 64, 100, 200, 256):
        rows = lib.nmfmu_sp_ntf_lds_rows(rank)
        # both panels staged and the loss kernel's 32 bytes: below 64 KiB, and two workgroups inside a CU's 160 KiB
        assert rows >= 31 and (rows + 1) * rank > 7936 >= rows * rank and 2 * (2 * rows * rank * 4 + 32) <= 160 * 1024
    assert lib.nmfmu_sp_ntf_lds_rows(0) == lib.nmfmu_sp_ntf_lds_rows(257) == lib.nmfmu_sp_ntf_lds_rows(-1) == 0
    assert lib.nmfmu_sp_ntf_ws(7, 128) == 7 * 2 * 128 and lib.nmfmu_sp_ntf_ws((1 << 31) - 1, 256) == ((1 << 31) - 1) * 512
    assert lib.nmfmu_sp_ntf_ws(0, 128) == lib.nmfmu_sp_ntf_ws(-1, 128) == lib.nmfmu_sp_ntf_ws(7, 0) == 0
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)


@pytest.mark.parametrize('chunk', (3, 512))
def test_planner_against_a_brute_force_sort(chunk):
    g = torch.Generator().manual_seed(3)
    shape = (4, 7, 5)
    D = torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) < 0.6)
    D[2], D[:, 3], D[:, :, 1] = 0, 0, 0
    V = D.to_sparse().coalesce()
    modes = ntf.plan_sparse_ntf(V.indices(), V.values(), shape, chunk)
    ent = [(tuple(int(x) for x in ix), float(v)) for ix, v in zip(V.indices().t(), V.values())]
    for n, m in enumerate(modes):
        a, b = (x for x in range(3) if x != n)
        want = sorted(ent, key=lambda e: (e[0][n], e[0][a], e[0][b]))
        assert m['idx_a'].tolist() == [e[0][a] for e in want] and m['idx_b'].tolist() == [e[0][b] for e in want]
        assert m['vals'].tolist() == [e[1] for e in want] and m['idx_a'].dtype == m['rowptr'].dtype == torch.int32
        counts = [sum(e[0][n] == r for e in want) for r in range(shape[n])]
        assert torch.diff(m['rowptr']).tolist() == counts and int(m['rowptr'][0]) == 0
        seg = m['seg'].tolist()          # every row is covered once, in order, by runs of at most chunk entries
        assert [s[0] for s in seg] == sorted(s[0] for s in seg) and {s[0] for s in seg} == set(range(shape[n]))
        assert all(0 <= s[2] - s[1] <= chunk for s in seg)
        for r in range(shape[n]):
            runs = [s for s in seg if s[0] == r]
            assert runs[0][1] == int(m['rowptr'][r]) and runs[-1][2] == int(m['rowptr'][r + 1])
            assert all(x[2] == y[1] for x, y in zip(runs, runs[1:])) and (len(runs) > 1) == (runs[0][3] >= 0)
        assert m['n_ws'] == sum(len([s for s in seg if s[0] == mu[0]]) for mu in m['multi'].tolist())


def test_refusals_in_their_order():
    V = (torch.rand(4, 5, 6) + 0.1).to_sparse()
    m, big = ntf.NTF(V.shape, rank=2), ntf.NTF((4, 5, 6), rank=300)
    w = torch.ones(4, 5, 6)
    with pytest.raises(NotImplementedError, match="unstored='missing'"):          # the keyword is still required
        m.fit(V)
    for bad_unstored in ('ZERO', 0.5, True):                                      # 1: before everything else
        with pytest.raises(ValueError, match="'zero' or 'missing'"):
            big.fit(torch.rand(4, 5).to_sparse(), beta=0, weights=w, unstored=bad_unstored)
    with pytest.raises(ValueError, match='dense tensor stores every entry'):
        m.fit(V.to_dense(), unstored='missing')
    with pytest.raises(NotImplementedError, match='order 3'):                     # 2
        big.fit(torch.rand(4, 5).to_sparse(), beta=0, weights=w, unstored='zero')
    with pytest.raises(ValueError, match='does not match'):                       # 3
        big.fit(torch.rand(4, 6, 5).to_sparse(), beta=0, weights=w, unstored='zero')
    with pytest.raises(NotImplementedError, match='stored set is the mask'):      # 4
        big.fit(V, beta=0, weights=w, unstored='zero')
    for beta in (0, 0.5, 3):
        with pytest.raises(NotImplementedError, match="use unstored='missing'"):  # 5
            big.fit(V, beta=beta, unstored='zero')
    for unstored, beta in (('zero', 1), ('zero', 2), ('missing', 0)):
        with pytest.raises(NotImplementedError, match='rank 300 > 256'):          # 6
            big.fit(V, beta=beta, unstored=unstored)
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):            # 7: -V is never scanned
            m.fit(-V, beta=beta, unstored=unstored)
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            ntf.sparse_ntf_loss(-V, list(m.factors), beta, unstored)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ntf.SparseNtfTarget(V)
