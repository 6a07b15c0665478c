"""``gram_rows=`` of ``NTF.fit(solver='ccd')`` / ``ntf_ccd_sweep`` and the ``nmfmu_sp_ntf_ccd_gram*`` entries without a GPU: the
refusals before the device is asked, the new names, the status codes on pointers that are never dereferenced, and the part
rule with its workspace cap."""
import os
import re

import pytest
import torch

from torchnmf_amd import _capi, ntf

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('nmfmu_sp_ntf_ccd_gram', 'nmfmu_sp_ntf_ccd_gram_ws', 'nmfmu_sp_ntf_ccd_gram_part')


def test_refusals_before_the_device():
    S = (torch.rand(4, 5, 6) + 0.1).to_sparse()
    m = ntf.NTF(S.shape, rank=2)
    keep = [f.detach().clone() for f in m.factors]
    fs = [f.detach() for f in m.factors]
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='gram_rows must be None or an integer >= 0'):
            m.fit(S, beta=2, unstored='missing', solver='ccd', gram_rows=bad)
        with pytest.raises(ValueError, match='gram_rows must be None or an integer >= 0'):
            ntf.ntf_ccd_sweep(S, fs, 0, gram_rows=bad)
    for solver, unstored in (('mu', 'missing'), ('hals', 'zero')):
        with pytest.raises(NotImplementedError, match="gram_rows= is the normal-equations route of solver='ccd'"):
            m.fit(S, beta=2, unstored=unstored, solver=solver, gram_rows=0)
    with pytest.raises(NotImplementedError, match="missing.*solver='mu' or solver='ccd'"):      # today's refusals come first
        m.fit(S, beta=2, unstored='missing', solver='hals', gram_rows=0)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.fit(S, beta=2, unstored='missing', solver='ccd', gram_rows=0)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        ntf.ntf_ccd_sweep(S, fs, 0, gram_rows=0, _part=33)
    assert all(torch.equal(f.detach(), k) for f, k in zip(m.factors, keep))


def test_the_names_are_declared_bound_and_exported():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr), name
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    mk = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'nmfmu_sparse_ntf_ccd_gram.hip' in mk.split('SRCS', 1)[1].split('\n', 1)[0]


KEYS = ('rowptr', 'idx_a', 'idx_b', 'vals', 'rows', 'row_part', 'part_row', 'n_long', 'n_parts', 'part', 'owner', 'pa', 'rows_a',
        'pb', 'rows_b', 'rank', 'l1', 'l2', 'ws', 'vec')
ARG, UNS = _capi.ERR_ARG, _capi.ERR_UNSUPPORTED


@pytest.mark.parametrize('kw, want', [
    *(({k: None}, ARG) for k in ('rowptr', 'idx_a', 'idx_b', 'vals', 'rows', 'row_part', 'part_row', 'owner', 'pa', 'pb', 'ws')),
    ({'pa': P + 448}, ARG), ({'pb': P + 448}, ARG), ({'n_long': 0}, ARG), ({'n_parts': 2}, ARG), ({'rows_a': 0}, ARG),
    ({'rows_b': -2}, ARG), ({'rank': 0}, ARG), ({'part': -32}, ARG), ({'part': 0}, ARG), ({'part': 48}, ARG), ({'vec': 3}, ARG),
    ({'rank': 257}, UNS), ({'rank': 300, 'owner': None}, ARG), ({'rank': 257, 'part': 33}, ARG)], ids=str)      # the order of the checks
def test_c_entry_refuses_before_device_work(kw, want):
    ok = dict(rowptr=P, idx_a=P + 64, idx_b=P + 128, vals=P + 192, rows=P + 256, row_part=P + 320, part_row=P + 384, n_long=3,
              n_parts=4, part=64, owner=P + 448, pa=P + 512, rows_a=5, pb=P + 576, rows_b=7, rank=4, l1=0.0, l2=0.0, ws=P + 640,
              vec=0)
    a = dict(ok, **kw)
    assert _capi.load().nmfmu_sp_ntf_ccd_gram(*(a[k] for k in KEYS), None) == want


@pytest.mark.parametrize('rank', [8, 64, 100, 256])
@pytest.mark.parametrize('n_long, count', [(24, 417_000), (1, 2_000_000_000), (512, 2700), (3, 40)])
def test_part_rule_and_workspace_cap(rank, n_long, count):
    """Equal rows: a multiple of 32, about four parts per compute unit where the rows are few, the workspace of
    ``ceil(count / part)`` parts per row under the 256 MiB cap -- which at r_pad 256 (653 parts) asks for longer parts."""
    lib = _capi.load()
    part = lib.nmfmu_sp_ntf_ccd_gram_part(n_long * count, n_long, count, rank, 256)
    n_parts = n_long * -(-count // part)
    assert part >= 256 and part % 32 == 0
    assert n_parts <= 1024 and (count < 100_000 or n_parts > (512 if rank <= 128 else 326))
    assert 0 < lib.nmfmu_sp_ntf_ccd_gram_ws(n_parts, n_long, rank) <= ntf.GRAM_CAP == 1 << 26
    assert part >= lib.nmfmu_sp_ntf_ccd_gram_part(n_long * count, n_long, count, 64, 256)
    if rank == 256 and count >= 100_000:
        assert n_parts <= 653 and part > lib.nmfmu_sp_ntf_ccd_gram_part(n_long * count, n_long, count, 128, 256)
    assert lib.nmfmu_sp_ntf_ccd_gram_part(n_long * count, n_long, count, 257, 256) == 0 == lib.nmfmu_sp_ntf_ccd_gram_ws(1, 2, rank)
