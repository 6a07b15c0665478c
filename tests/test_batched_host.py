"""Batched NMF without a GPU: the argument errors of the new C entries (every call returns before a launch), the workspace and
split-count rules against their Python statement in tests/batched_emulation.py (the split ignores the batch), the validation
order of ``BatchedNMF.fit`` on CPU tensors, and the signatures -- ``NMF.fit``'s is what it was."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import batched_emulation as BE
from torchnmf_amd import _capi, batched, metrics
from torchnmf_amd.batched import BatchedNMF, batched_beta_div
from torchnmf_amd.nmf import NMF, BaseComponent

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _terms(lib, **kw):
    a = dict(V=P, vstride=131 * 70, ld=70, batch=3, n=131, c=70, side=0, owner=P, panel=P + 64, rank=5, r_pad=32, beta=1.0,
             nsplit=0, active=None, ws=P, num=P, den=P)
    a.update(kw)
    return lib.nmfmu_bmu_terms(a['V'], a['vstride'], a['ld'], a['batch'], a['n'], a['c'], a['side'], a['owner'], a['panel'],
                               a['rank'], a['r_pad'], a['beta'], a['nsplit'], a['active'], a['ws'], a['num'], a['den'], None)


def _step(lib, **kw):
    a = dict(V=P, vstride=131 * 70, ld=70, batch=3, n=131, c=70, side=0, owner=P, panel=P + 64, rank=5, r_pad=32, beta=1.0,
             nsplit=0, active=None, ws=P)
    a.update(kw)
    return lib.nmfmu_bmu_step(a['V'], a['vstride'], a['ld'], a['batch'], a['n'], a['c'], a['side'], a['owner'], a['panel'],
                              a['rank'], a['r_pad'], a['beta'], 0.0, 0.0, 1.0, a['nsplit'], a['active'], a['ws'], None)


def _loss(lib, **kw):
    a = dict(V=P, vstride=131 * 70, ld=70, batch=3, n=131, c=70, owner=P, panel=P + 64, rank=5, beta=1.0, v_term=P,
             active=None, part=P, out=P)
    a.update(kw)
    return lib.nmfmu_bmu_loss(a['V'], a['vstride'], a['ld'], a['batch'], a['n'], a['c'], a['owner'], a['panel'], a['rank'],
                              a['beta'], a['v_term'], a['active'], a['part'], a['out'], None)


def _judge(lib, **kw):
    a = dict(batch=3, div=P, loss_init=P, previous=P, tol=1e-4, iteration=9, active=P, n_iter=P, n_active=P)
    a.update(kw)
    return lib.nmfmu_bmu_judge(a['batch'], a['div'], a['loss_init'], a['previous'], a['tol'], a['iteration'], a['active'],
                               a['n_iter'], a['n_active'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('V', 'owner', 'panel', 'ws', 'num', 'den')),
                                           (_step, ('V', 'owner', 'panel', 'ws')),
                                           (_loss, ('V', 'owner', 'panel', 'v_term', 'part', 'out'))])
def test_argument_errors(call, pointers):
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    assert call(lib, rank=0) == _capi.ERR_ARG and call(lib, rank=-3) == _capi.ERR_ARG
    assert call(lib, n=0) == _capi.ERR_ARG and call(lib, c=-1) == _capi.ERR_ARG and call(lib, ld=69) == _capi.ERR_ARG
    assert call(lib, batch=0) == _capi.ERR_ARG and call(lib, batch=-2) == _capi.ERR_ARG
    assert call(lib, vstride=-1) == _capi.ERR_ARG
    assert call(lib, rank=257, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    for beta in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0):                      # no beta is refused -- only the rank
        assert call(lib, rank=300, beta=beta, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    if call is not _loss:
        for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
            assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
        assert call(lib, nsplit=-1) == _capi.ERR_ARG
        assert call(lib, side=2) == _capi.ERR_ARG and call(lib, side=-1) == _capi.ERR_ARG
        assert call(lib, nsplit=-1, rank=300, r_pad=256) == _capi.ERR_ARG      # the arguments are judged before the rank


def test_step_refuses_aliased_factors():
    assert _step(_capi.load(), owner=P, panel=P) == _capi.ERR_ARG


def test_a_batch_past_the_grid_is_refused_before_a_launch():
    """The problem index is the slow part of grid.x: batch * row tiles (and the other kernels' workgroups per problem) must fit
    2^31 - 1.  131 rows are two tiles: 2^30 problems pass the limit."""
    lib = _capi.load()
    for call in (_terms, _step, _loss):
        assert call(lib, batch=2 ** 30) == _capi.ERR_UNSUPPORTED


def test_judge_argument_errors():
    lib = _capi.load()
    for name in ('div', 'loss_init', 'previous', 'active', 'n_iter', 'n_active'):
        assert _judge(lib, **{name: None}) == _capi.ERR_ARG, name
    assert _judge(lib, batch=0) == _capi.ERR_ARG and _judge(lib, iteration=-1) == _capi.ERR_ARG


def test_v_term_argument_errors():
    lib = _capi.load()

    def call(**kw):
        a = dict(V=P, vstride=131 * 70, ld=70, batch=3, n=131, c=70, beta=1.0, out=P)
        a.update(kw)
        return lib.nmfmu_bmu_v_term(a['V'], a['vstride'], a['ld'], a['batch'], a['n'], a['c'], a['beta'], a['out'], None)
    for kw in (dict(V=None), dict(out=None), dict(batch=0), dict(n=0), dict(c=-1), dict(ld=69), dict(vstride=-1)):
        assert call(**kw) == _capi.ERR_ARG, kw


def test_workspace_and_split_rules():
    lib = _capi.load()
    shapes = [(131, 70), (70, 131), (132, 72), (513, 128), (128, 513), (64, 64), (5168, 1025), (1025, 5168), (1, 1), (128, 32),
              (129, 33)]
    for rows, contraction in shapes:
        for r_pad in (32, 64, 128, 256):
            auto = lib.nmfmu_bmu_nsplit(rows, contraction, r_pad)
            assert auto == BE.split(rows, contraction, r_pad) == lib.nmfmu_wmu_nsplit(rows, contraction, r_pad) >= 1
            for nsplit in (0, 1, 2, 3, 7, 1000):
                one = lib.nmfmu_bmu_ws(1, rows, contraction, r_pad, nsplit)
                assert one == BE.workspace_floats(1, rows, contraction, r_pad, nsplit) == lib.nmfmu_wmu_ws(rows, contraction,
                                                                                                          r_pad, nsplit)
                parts = one // (2 * rows * r_pad)
                assert 1 <= parts <= BE.stages(contraction)
                for batch in (2, 5, 4096):      # the batch multiplies the slab and nothing else: the split ignores it
                    want = BE.workspace_floats(batch, rows, contraction, r_pad, nsplit)
                    assert lib.nmfmu_bmu_ws(batch, rows, contraction, r_pad, nsplit) == want == batch * one
                    assert batched.workspace_floats(batch, rows, contraction, r_pad, nsplit) == want
        assert lib.nmfmu_bmu_loss_parts(rows, contraction) == BE.loss_parts(rows, contraction) >= -(-rows // 128)
    # the three benchmark shapes: what the rule gives (H side, W side)
    assert (lib.nmfmu_bmu_nsplit(513, 128, 32), lib.nmfmu_bmu_nsplit(128, 513, 32)) == (1, 4)
    assert (lib.nmfmu_bmu_nsplit(64, 64, 32), lib.nmfmu_bmu_nsplit(5168, 1025, 128)) == (1, 7)     # 33 stages, 5 per part
    for bad in ((0, 131, 70, 32, 0), (3, 0, 70, 32, 0), (3, 131, 0, 32, 0), (3, 131, 70, 0, 0), (3, 131, 70, 32, -1)):
        assert lib.nmfmu_bmu_ws(*bad) == 0
    assert lib.nmfmu_bmu_nsplit(0, 70, 32) == _capi.ERR_ARG and lib.nmfmu_bmu_loss_parts(131, 0) == _capi.ERR_ARG


def test_abi_is_additive():
    lib = _capi.load()
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in ('nmfmu_bmu_nsplit', 'nmfmu_bmu_ws', 'nmfmu_bmu_terms', 'nmfmu_bmu_step', 'nmfmu_bmu_loss_parts',
                 'nmfmu_bmu_loss', 'nmfmu_bmu_v_term', 'nmfmu_bmu_judge'):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)
    assert lib.nmfmu_bmu_ws.restype is C.c_int64
    assert len(_capi.SIGNATURES['nmfmu_bmu_terms'][1]) == 18 and len(_capi.SIGNATURES['nmfmu_bmu_step'][1]) == 19
    assert len(_capi.SIGNATURES['nmfmu_bmu_loss'][1]) == 15 and len(_capi.SIGNATURES['nmfmu_bmu_judge'][1]) == 10
    assert _capi.SIGNATURES['nmfmu_bmu_judge'][1][4] is C.c_double


def test_signatures():
    par = inspect.signature(BaseComponent.fit).parameters          # NMF.fit is what it was
    assert list(par) == ['self', 'V', 'beta', 'tol', 'max_iter', 'verbose', 'alpha', 'l1_ratio', 'precision', 'process_group',
                         'allreduce', 'unstored', 'weights', 'solver']
    assert [par[k].default for k in ('beta', 'tol', 'max_iter', 'verbose', 'alpha', 'l1_ratio')] == [1, 1e-4, 200, False, 0, 0]
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(par)[8:])
    assert 'fit' not in NMF.__dict__                                # still BaseComponent's
    par = inspect.signature(NMF.fit_restarts).parameters
    assert list(par) == ['self', 'V', 'n_init', 'beta', 'tol', 'max_iter', 'alpha', 'l1_ratio', 'generator']
    assert [par[k].default for k in list(par)[3:]] == [1, 1e-4, 200, 0, 0, None]
    par = inspect.signature(BatchedNMF.fit).parameters
    assert list(par)[:7] == ['self', 'V', 'beta', 'tol', 'max_iter', 'alpha', 'l1_ratio']
    assert [par[k].default for k in list(par)[2:7]] == [1, 1e-4, 200, 0, 0]
    assert metrics.batched_beta_div is batched_beta_div and 'batched_beta_div' in metrics.__all__
    assert batched.MAX_RANK == 256


def test_construction():
    torch.manual_seed(3)
    m = BatchedNMF((4, 6, 5), rank=2)
    assert tuple(m.H.shape) == (4, 6, 2) and tuple(m.W.shape) == (4, 5, 2) and (m.batch, m.rank) == (4, 2)
    assert bool((m.H >= 0).all()) and bool((m.W >= 0).all()) and m.H.requires_grad and m.W.requires_grad
    assert tuple(m().shape) == (4, 6, 5) and torch.allclose(m()[2], m.H[2] @ m.W[2].T)
    W, H = torch.rand(3, 5, 2), torch.rand(3, 6, 2)
    m = BatchedNMF(W=W, H=H, trainable_W=False)
    assert torch.equal(m.W.data, W) and torch.equal(m.H.data, H) and not m.W.requires_grad and m.H.requires_grad
    p = m.problem(1)
    assert isinstance(p, NMF) and torch.equal(p.W.data, W[1]) and torch.equal(p.H.data, H[1]) and not p.W.requires_grad
    p.H.data.zero_()
    assert torch.equal(m.H.data, H)                                   # copies
    with pytest.raises(AssertionError, match='non-negative'):
        BatchedNMF(W=-W, H=H)
    with pytest.raises(AssertionError, match='share batch and rank'):
        BatchedNMF(W=W, H=torch.rand(4, 6, 2))
    with pytest.raises(AssertionError, match=r'\(batch, rows, rank\)'):
        BatchedNMF(W=W[0], H=H[0])


def test_validation_comes_before_the_device():
    """On CPU tensors: every refusal that needs no device is raised before the device check (which raises NmfmuError)."""
    m = BatchedNMF((3, 6, 5), rank=2)
    V = torch.rand(3, 6, 5) + 0.1
    for call in (lambda v: m.fit(v), lambda v: m.loss(v, 1), lambda v: batched_beta_div(m.H.data, m.W.data, v, 1),
                 lambda v: m.best(v)):
        with pytest.raises(ValueError, match='must be a tensor'):
            call(V.numpy())
        with pytest.raises(NotImplementedError, match='dense targets only'):
            call(V[0].to_sparse())
        for bad in (torch.rand(3, 5, 6), torch.rand(2, 6, 5), torch.rand(5, 6), torch.rand(90)):
            with pytest.raises(ValueError, match='does not match the model'):
                call(bad)
        with pytest.raises(NotImplementedError, match='fp32 targets only'):
            call(V.double())
        for ok in (V, V[0]):                                          # a batch of targets, or one shared target
            with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
                call(ok)
    big = BatchedNMF((2, 6, 5), rank=300)
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        big.fit(torch.rand(2, 6, 5))
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):   # ... before the dtype of the target
        big.fit(torch.rand(2, 6, 5).double())
    with pytest.raises(NotImplementedError, match='keeps fp32 factors'):
        BatchedNMF((3, 6, 5), rank=2).double().fit(V)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):     # fit_restarts ends at the same check
        NMF((6, 5), rank=2).fit_restarts(V[0], 3)
    with pytest.raises(ValueError, match='n_init must be >= 1'):
        NMF((6, 5), rank=2).fit_restarts(V[0], 0)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):     # the default fit is untouched
        NMF((6, 5), rank=2).fit(V[0])
