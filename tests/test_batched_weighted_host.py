"""Weighted batched NMF and model selection without a GPU: the argument errors of the four nmfmu_bwmu entries (every call
returns before a launch), the validation order and messages of ``weights`` / ``weight_index`` / per-problem ``alpha`` on CPU
tensors (each judged before any device use), the signatures, ``holdout_masks``, and the float64 model of
tests/batched_weighted_emulation.py against the reference's recorded runs (golden g25)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import batched_weighted_emulation as BWE
from conftest import load_golden, rel_err
from torchnmf_amd import _capi, batched, metrics, model_selection
from torchnmf_amd.batched import BatchedNMF, batched_beta_div
from torchnmf_amd.model_selection import cross_validate, holdout_masks
from torchnmf_amd.nmf import BaseComponent

P = 0x1000          # a non-null pointer no call below may dereference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(V=P, vstride=131 * 70, M=P + 128, mstride=131 * 70, m_index=None, ld=70, batch=3, n=131, c=70, side=0, owner=P,
            panel=P + 64, rank=5, r_pad=32, beta=1.0, nsplit=0, active=None, ws=P, num=P, den=P, reg=None, v_term=P, part=P,
            out=P)


def _args(kw):
    a = dict(BASE)
    a.update(kw)
    return a


def _terms(lib, **kw):
    a = _args(kw)
    return lib.nmfmu_bwmu_terms(a['V'], a['vstride'], a['M'], a['mstride'], a['m_index'], a['ld'], a['batch'], a['n'], a['c'],
                                a['side'], a['owner'], a['panel'], a['rank'], a['r_pad'], a['beta'], a['nsplit'], a['active'],
                                a['ws'], a['num'], a['den'], None)


def _step(lib, **kw):
    a = _args(kw)
    return lib.nmfmu_bwmu_step(a['V'], a['vstride'], a['M'], a['mstride'], a['m_index'], a['ld'], a['batch'], a['n'], a['c'],
                               a['side'], a['owner'], a['panel'], a['rank'], a['r_pad'], a['beta'], 0.0, 0.0, a['reg'], 1.0,
                               a['nsplit'], a['active'], a['ws'], None)


def _loss(lib, **kw):
    a = _args(kw)
    return lib.nmfmu_bwmu_loss(a['V'], a['vstride'], a['M'], a['mstride'], a['m_index'], a['ld'], a['batch'], a['n'], a['c'],
                               a['owner'], a['panel'], a['rank'], a['beta'], a['v_term'], a['active'], a['part'], a['out'], None)


def _v_term(lib, **kw):
    a = _args(kw)
    return lib.nmfmu_bwmu_v_term(a['V'], a['vstride'], a['M'], a['mstride'], a['m_index'], a['ld'], a['batch'], a['n'], a['c'],
                                 a['beta'], a['out'], None)


@pytest.mark.parametrize('call,pointers', [(_terms, ('V', 'owner', 'panel', 'ws', 'num', 'den')),
                                           (_step, ('V', 'owner', 'panel', 'ws')),
                                           (_loss, ('V', 'owner', 'panel', 'v_term', 'part', 'out')),
                                           (_v_term, ('V', 'out'))])
def test_argument_errors(call, pointers):
    """The nmfmu_bmu list, then the two of the weights.  A batch past the grid is how an ACCEPTED argument list is seen without
    a launch: it comes back NMFMU_ERR_UNSUPPORTED after every argument check has passed."""
    lib = _capi.load()
    for name in pointers:
        assert call(lib, **{name: None}) == _capi.ERR_ARG, name
    assert call(lib, n=0) == _capi.ERR_ARG and call(lib, c=-1) == _capi.ERR_ARG and call(lib, ld=69) == _capi.ERR_ARG
    assert call(lib, batch=0) == _capi.ERR_ARG and call(lib, batch=-2) == _capi.ERR_ARG
    assert call(lib, vstride=-1) == _capi.ERR_ARG
    # the weights' own: a negative stride; an index with nothing to index (before anything else is looked at)
    assert call(lib, mstride=-1) == _capi.ERR_ARG
    assert call(lib, M=None, m_index=P) == _capi.ERR_ARG
    assert call(lib, M=None, m_index=P, batch=2 ** 30) == _capi.ERR_ARG
    if call is _v_term:
        return
    assert call(lib, rank=0) == _capi.ERR_ARG and call(lib, rank=-3) == _capi.ERR_ARG
    assert call(lib, rank=257, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    for beta in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0):                      # no beta is refused -- only the rank
        assert call(lib, rank=300, beta=beta, **({} if call is _loss else {'r_pad': 256})) == _capi.ERR_UNSUPPORTED
    if call is not _loss:
        for rank, r_pad in ((5, 64), (33, 32), (100, 256), (200, 128), (5, 0)):
            assert call(lib, rank=rank, r_pad=r_pad) == _capi.ERR_ARG, (rank, r_pad)
        assert call(lib, nsplit=-1) == _capi.ERR_ARG
        assert call(lib, side=2) == _capi.ERR_ARG and call(lib, side=-1) == _capi.ERR_ARG
        assert call(lib, nsplit=-1, rank=300, r_pad=256) == _capi.ERR_ARG      # the arguments are judged before the rank
    # accepted: M == NULL (the unweighted instantiation), a shared M, an index -- each gets as far as the grid check
    for ok in (dict(M=None), dict(M=None, mstride=0), dict(mstride=0), dict(m_index=P), dict(mstride=0, m_index=P),
               dict(vstride=0)):
        assert call(lib, batch=2 ** 30, **ok) == _capi.ERR_UNSUPPORTED, ok
    if call is _step:
        assert call(lib, batch=2 ** 30, reg=P) == _capi.ERR_UNSUPPORTED
        assert call(lib, batch=2 ** 30, reg=P, M=None) == _capi.ERR_UNSUPPORTED
        assert call(lib, owner=P, panel=P) == _capi.ERR_ARG


def test_abi_is_additive():
    lib = _capi.load()
    assert _capi.ABI_VERSION == 10 and lib.nmfmu_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    for name in ('nmfmu_bwmu_terms', 'nmfmu_bwmu_step', 'nmfmu_bwmu_loss', 'nmfmu_bwmu_v_term'):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r'\b' + name + r'\(', hdr)
        assert hdr.index(name) < hdr.index('10: nmfmu_plca_normalize')          # listed in the header comment's ABI history
    n = {k: len(_capi.SIGNATURES[k][1]) for k in _capi.SIGNATURES}
    assert n['nmfmu_bwmu_terms'] == n['nmfmu_bmu_terms'] + 3 and n['nmfmu_bwmu_step'] == n['nmfmu_bmu_step'] + 4
    assert n['nmfmu_bwmu_loss'] == n['nmfmu_bmu_loss'] + 3 and n['nmfmu_bwmu_v_term'] == n['nmfmu_bmu_v_term'] + 3
    assert _capi.SIGNATURES['nmfmu_bwmu_step'][1][17] is C.c_void_p          # reg sits between l2 and gamma


def test_signatures():
    par = inspect.signature(BaseComponent.fit).parameters          # NMF.fit is what it was
    assert list(par) == ['self', 'V', 'beta', 'tol', 'max_iter', 'verbose', 'alpha', 'l1_ratio', 'precision', 'process_group',
                         'allreduce', 'unstored', 'weights', 'solver']
    par = inspect.signature(BatchedNMF.fit).parameters
    assert list(par) == ['self', 'V', 'beta', 'tol', 'max_iter', 'alpha', 'l1_ratio', 'nsplit', 'weights', 'weight_index']
    assert [par[k].default for k in list(par)[2:]] == [1, 1e-4, 200, 0, 0, 0, None, None]
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('nsplit', 'weights', 'weight_index'))
    for fn in (batched_beta_div, BatchedNMF.loss, BatchedNMF.best):
        par = inspect.signature(fn).parameters
        assert list(par)[-2:] == ['weights', 'weight_index'] and par['weights'].default is None \
            and par['weight_index'].default is None
    assert metrics.batched_beta_div is batched_beta_div
    par = inspect.signature(cross_validate).parameters
    assert list(par) == ['V', 'ranks', 'beta', 'folds', 'n_init', 'alpha', 'l1_ratio', 'tol', 'max_iter', 'generator', 'weights']
    assert [par[k].default for k in list(par)[2:]] == [1, 5, 1, 0, 0, 1e-4, 200, None, None]
    par = inspect.signature(holdout_masks).parameters
    assert list(par) == ['shape', 'folds', 'generator', 'device', 'weights']


def test_validation_comes_before_the_device():
    """On CPU tensors every refusal of the new arguments is raised before the device check (NmfmuError), in order: the target,
    the weights, the index, the regulariser, the device."""
    m = BatchedNMF((3, 6, 5), rank=2)
    V = torch.rand(3, 6, 5) + 0.1
    M = torch.rand(3, 6, 5)
    calls = (lambda **k: m.fit(V, **k), lambda **k: m.loss(V, 1, **k), lambda **k: m.best(V, 1, **k),
             lambda **k: batched_beta_div(m.H.data, m.W.data, V, 1, **k))
    for call in calls:
        with pytest.raises(ValueError, match='weights must be a tensor'):
            call(weights=M.numpy())
        for bad in (torch.rand(6, 6), torch.rand(2, 6, 5), torch.rand(3, 5, 6), torch.rand(90)):
            with pytest.raises(ValueError, match='weights must be a dense tensor'):
                call(weights=bad)
        with pytest.raises(ValueError, match='weights must be a dense tensor'):
            call(weights=M[0].to_sparse())
        with pytest.raises(ValueError, match='weights must be bool, integer or floating'):
            call(weights=torch.complex(M, M))
        for bad in (-M, M.clone().index_put_((torch.tensor(1), torch.tensor(2), torch.tensor(3)), torch.tensor(float('nan'))),
                    M.clone().index_put_((torch.tensor(0), torch.tensor(0), torch.tensor(0)), torch.tensor(float('inf')))):
            with pytest.raises(ValueError, match='weights must be finite and non-negative'):
                call(weights=bad)
        with pytest.raises(ValueError, match='weight_index needs weights'):
            call(weight_index=torch.zeros(3, dtype=torch.int64))
        G = torch.rand(2, 6, 5)
        with pytest.raises(ValueError, match=r'must be a dense tensor \(G, 6, 5\)'):
            call(weights=M[0], weight_index=torch.zeros(3, dtype=torch.int64))
        with pytest.raises(ValueError, match='must be an integer tensor'):
            call(weights=G, weight_index=torch.zeros(3))
        with pytest.raises(ValueError, match='must be an integer tensor'):
            call(weights=G, weight_index=[0, 1, 0])
        with pytest.raises(ValueError, match='one entry per problem'):
            call(weights=G, weight_index=torch.zeros(2, dtype=torch.int64))
        for bad in ([0, 2, 1], [0, -1, 1]):
            with pytest.raises(ValueError, match=r'must lie in \[0, 2\)'):
                call(weights=G, weight_index=torch.tensor(bad))
        # accepted forms end at the device check: bool, integer and floating; shared, per problem, indexed
        for ok in (dict(weights=M), dict(weights=M[0]), dict(weights=M > 0.5), dict(weights=(M * 3).to(torch.int32)),
                   dict(weights=M.double()), dict(weights=G, weight_index=torch.tensor([1, 0, 1])),
                   dict(weights=G, weight_index=torch.tensor([1, 0, 1], dtype=torch.int32))):
            with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
                call(**ok)
        with pytest.raises(ValueError, match='does not match the model'):       # the target is judged before the weights
            (m.fit if call is calls[0] else lambda v, **k: m.loss(v, 1, **k))(torch.rand(3, 5, 6), weights='nonsense')
    # per-problem regulariser: a float, or one value per problem
    for bad in ([0.1, 0.2], torch.rand(4), (0.1,)):
        with pytest.raises(ValueError, match=r'alpha must be a float or hold one value per problem \[3\]'):
            m.fit(V, alpha=bad)
        with pytest.raises(ValueError, match=r'l1_ratio must be a float or hold one value per problem \[3\]'):
            m.fit(V, alpha=0.1, l1_ratio=bad)
    with pytest.raises(ValueError, match='weights must be a tensor'):          # the weights before the regulariser
        m.fit(V, alpha=[0.1, 0.2], weights=3)
    for ok in (dict(alpha=[0.1, 0.2, 0.3]), dict(alpha=torch.rand(3), l1_ratio=(0.1, 0.5, 0.9)), dict(alpha=0.1, l1_ratio=0.5),
               dict(alpha=torch.tensor(0.1))):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.fit(V, **ok)


def test_reg_pairs():
    """nmf.py:348-349 per problem, in double; scalars stay scalars (the unweighted entries are then called as always)."""
    assert batched._check_reg(0.07, 0.3, 4) == (0.07 * 0.3, 0.07 * (1 - 0.3), None)
    l1, l2, reg = batched._check_reg([0.0, 0.07, 0.5], 0.3, 3)
    assert (l1, l2) == (0.0, 0.0) and reg.dtype == torch.float64 and tuple(reg.shape) == (3, 2)
    assert reg.tolist() == [[0.0, 0.0], [0.07 * 0.3, 0.07 * (1 - 0.3)], [0.5 * 0.3, 0.5 * (1 - 0.3)]]
    _, _, reg = batched._check_reg(torch.tensor([1.0, 2.0]), torch.tensor([0.25, 0.5]), 2)
    assert reg.tolist() == [[0.25, 0.75], [1.0, 1.0]]
    assert BWE.l1_l2([0.0, 0.07, 0.5], 0.3).tolist() == batched._check_reg([0.0, 0.07, 0.5], 0.3, 3)[2].tolist()


def test_cross_validate_validation():
    V = torch.rand(12, 9) + 0.1
    with pytest.raises(ValueError, match='must be a tensor'):
        cross_validate(V.numpy(), (2, 3))
    with pytest.raises(NotImplementedError, match='dense target'):
        cross_validate(V.to_sparse(), (2, 3))
    with pytest.raises(ValueError, match=r'must be \(N, C\)'):
        cross_validate(V[None], (2, 3))
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        cross_validate(V, (2, 300))
    with pytest.raises(NotImplementedError, match='fp32 target'):
        cross_validate(V.double(), (2, 3))
    with pytest.raises(ValueError, match='ranks >= 1'):
        cross_validate(V, ())
    with pytest.raises(ValueError, match='ranks >= 1'):
        cross_validate(V, (2, 0))
    with pytest.raises(ValueError, match='folds must lie in'):
        cross_validate(V, (2, 3), folds=1)
    with pytest.raises(ValueError, match='weights must be a dense tensor'):
        cross_validate(V, (2, 3), weights=torch.rand(9, 12))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        cross_validate(V, (2, 3), alpha=(0.0, 0.1))
    assert [x.tolist() for x in model_selection.problem_layout(2, 3, 2)] == \
        [list(x) for x in BWE.problem_layout(2, 3, 2)] == \
        [[0] * 6 + [1] * 6, [0, 0, 1, 1, 2, 2] * 2, [0, 1] * 6]


@pytest.mark.parametrize('folds', [2, 4, 5])
def test_holdout_masks(folds):
    N, C = 13, 7                                   # 91 entries: no fold count above divides them
    train, test = holdout_masks((N, C), folds, torch.Generator().manual_seed(3))
    assert train.shape == test.shape == (folds, N, C) and train.dtype == test.dtype == torch.float32
    assert train.device.type == 'cpu'
    assert torch.equal(train + test, torch.ones(folds, N, C)) and torch.equal(test.sum(0), torch.ones(N, C))
    assert bool(((test == 0) | (test == 1)).all())
    sizes = test.sum(dim=(1, 2))
    assert float(sizes.max() - sizes.min()) <= 1 and float(sizes.sum()) == N * C
    again = holdout_masks((N, C), folds, torch.Generator().manual_seed(3))
    assert torch.equal(again[0], train) and torch.equal(again[1], test)
    other = holdout_masks((N, C), folds, torch.Generator().manual_seed(4))
    assert not torch.equal(other[1], test)
    # a base of real weights with zeros: respected, dealt evenly, the identities exact
    g = torch.Generator().manual_seed(9)
    base = (torch.rand(N, C, generator=g) * 3.75 + 0.25) * (torch.rand(N, C, generator=g) < 0.6)
    base[4] = 0
    train, test = holdout_masks((N, C), folds, torch.Generator().manual_seed(3), weights=base)
    assert torch.equal(train + test, base.expand(folds, N, C)) and torch.equal(test.sum(0), base)
    assert bool((test[:, base == 0] == 0).all()) and bool((train[:, base == 0] == 0).all())
    assert bool(((test == 0) | (test == base)).all()) and bool(((test > 0).sum(0) == (base > 0)).all())
    counts = (test > 0).sum(dim=(1, 2))
    assert int(counts.max() - counts.min()) <= 1 and int(counts.sum()) == int((base > 0).sum())
    # bool and integer bases go through check_weights' conversion
    tb, sb = holdout_masks((N, C), folds, torch.Generator().manual_seed(3), weights=base > 0)
    assert torch.equal(tb + sb, (base > 0).float().expand(folds, N, C)) and torch.equal(sb > 0, test > 0)
    with pytest.raises(ValueError, match='folds must lie in'):
        holdout_masks((N, C), 1)
    with pytest.raises(ValueError, match='folds must lie in'):
        holdout_masks((2, 2), 5)
    with pytest.raises(ValueError, match='finite and non-negative'):
        holdout_masks((N, C), folds, weights=-base)


def test_summarise_is_nan_safe():
    loss = torch.tensor([[[[1.0, 3.0], [2.0, 2.0]]], [[[float('nan'), 0.1], [0.1, 0.1]]], [[[1.0, 1.0], [4.0, 2.0]]]],
                        dtype=torch.float64)                                    # [3 ranks, 1 alpha, 2 folds, 2 starts]
    n_test = torch.tensor([2.0, 4.0], dtype=torch.float64)
    mean, best = model_selection.summarise(loss, n_test, (2, 4, 8), (0.5,))
    assert mean[:, 0].tolist()[0] == (0.5 + 1.5 + 0.5 + 0.5) / 4 and bool(torch.isnan(mean[1, 0]))
    assert mean[2, 0] == (0.5 + 0.5 + 1.0 + 0.5) / 4 and best == (8, 0.5)           # the NaN mean of rank 4 never wins
    m2, b2 = BWE.summarise(loss.numpy(), n_test.numpy(), (2, 4, 8), (0.5,))
    assert np.array_equal(m2, mean.numpy(), equal_nan=True) and b2 == best


G25 = load_golden('g25_batched_weighted')


@pytest.mark.parametrize('case', [str(c) for c in G25['cases']])
def test_model_reproduces_golden_g25(case):
    """The float64 model (weights read through the index, the regulariser per problem) against the reference's float64 runs:
    two float64 routes to the same factors -- 1e-9 relative is the room for 20 iterations of different summation orders."""
    g = G25
    beta = float(g[case + '_beta'])
    reg = BWE.l1_l2(g['alpha'], g['l1_ratio'])
    assert len({tuple(r) for r in reg.tolist()}) == 2 and g['weight_index'].tolist() == [0, 1, 0, 1]
    M = g['M']
    assert M.shape == (2, 37, 29) and set(np.unique(M).tolist()) == {0, 1, 2, 3}
    assert not M[:, 11].any() and not M[:, :, 7].any() and not np.array_equal(M[0], M[1])
    W, H, n, _ = BWE.fit(g['V'], M, g['W0'], g['H0'], beta, -1e9, int(g['iterations']), reg, g['weight_index'])
    assert n.tolist() == [int(g['iterations'])] * 4
    losses = [x[0] for x in BWE.loss(g['V'], M, H, W, beta, g['weight_index'])]
    for b in range(4):
        assert rel_err(torch.from_numpy(W[b]), g[case + '_W'][b]) < 1e-9 and rel_err(torch.from_numpy(H[b]), g[case + '_H'][b]) < 1e-9
        assert abs(losses[b] - float(g[case + '_loss'][b])) < 1e-9 * abs(float(g[case + '_loss'][b]))
