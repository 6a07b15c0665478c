"""Fold-in on the device (csrc/nmfmu_fold_in.hip, torchnmf_amd/fold_in.py, ``NMF.transform``): one iteration per element
against the float64 reference under the bounds derived in tests/fold_in_emulation.py (no element left out), the reference's
recorded runs (golden g22, g20's frozen-W case), the bitwise properties the kernel promises, the per-row stop rule against
the states of one-iteration calls, the frozen-W ``fit`` route, and the checks that need the data.

Targets: (a) 37 x 29, row counts cycling 0, 1, 4, 5, 8, 9, 20 -- with the thresholds forced small (block 8, long rows above
16) a row of exactly one block, rows of two and three blocks and a workgroup row; (b) 9 x 700 with rows of 0, 1, 63, 64, 65,
130, 300, 513 and 700 stored entries -- the block edges at the largest block (64), rows that restage, and at every rank rows
above the default long-row threshold (the rank's largest block: 64 at ranks 3 and 33, 12 at rank 256).

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 22.
"""
import functools

import numpy as np
import pytest
import torch

import fold_in_emulation as F
import masked_emulation as M
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

RANKS = [3, 33, 100, 200, 256]        # r_pad 32 / 64 / 128 / 256 / 256
MODES = [('missing', b) for b in (-1, 0, 0.5, 1, 2, 3)] + [('zero', 1), ('zero', 2)]
ALPHA, L1_RATIO = 0.07, 0.3
REG = (ALPHA * L1_RATIO, ALPHA * (1 - L1_RATIO))
SMALL = dict(_block=8, _long_rows=16)
TOL = 1e-4                            # the project's bar for factors after a recorded run
GARBAGE = -7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(which, R):
    if which == 'a':
        return M.make_problem(37, 29, R, 0) + ((37, 29),)
    return F.make_wide(R) + ((9, 700),)


def _sparse(idx, vals, shape, dev):
    return torch.sparse_coo_tensor(torch.from_numpy(np.asarray(idx)), torch.from_numpy(np.asarray(vals)), shape).to(dev)


def _fold(dev, prob, beta, mode, reg=False, max_iter=1, tol=0.0, H0=None, target=None, **kw):
    from torchnmf_amd.fold_in import fold_in
    idx, vals, W0, H00, shape = prob
    Wd = torch.from_numpy(W0).to(dev)
    Hd = torch.from_numpy(H00).to(dev) if H0 is None else H0
    V = _sparse(idx, vals, shape, dev) if target is None else target
    keepW, keepH = Wd.clone(), Hd.clone()
    H, cnt = fold_in(Wd, V, beta, max_iter, tol, ALPHA if reg else 0, L1_RATIO if reg else 0, unstored=mode, H0=Hd,
                     return_n_iter=True, _fill=GARBAGE, **kw)
    assert torch.equal(Wd, keepW) and torch.equal(Hd, keepH)           # W and the caller's H0 are bitwise unchanged
    assert H.dtype == torch.float32 and cnt.dtype == torch.int32 and H.shape == Hd.shape and cnt.shape == (shape[0],)
    return H, cnt


# ---- 1. one iteration, per element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('mode,beta', MODES)
def test_one_iteration_per_element(dev, mode, beta, R):
    for which in ('a', 'b'):
        prob = _problem(which, R)
        idx, vals, W0, H0, shape = prob
        for reg in (False, True):
            l1, l2 = REG if reg else (0.0, 0.0)
            for kw in ({}, SMALL):
                ref, bound, t = F.iteration(idx, vals, shape, H0, W0, beta, mode, l1, l2,
                                            long_rows=kw.get('_long_rows'))
                H, cnt = _fold(dev, prob, beta, mode, reg, **kw)
                worst, ok = F.check(H.double().cpu().numpy(), ref, bound, cnt.cpu().numpy(), np.ones(shape[0]))
                info = dict(mode=mode, beta=beta, R=R, target=which, reg=reg, small=bool(kw))
                record('fold_in_iteration', worst_fraction_of_bound=worst, **info)
                print(f'fold_in_iteration {info}: worst |got - ref| / bound = {worst:.3f}')
                assert ok, (info, worst)
                if mode == 'missing' and not reg:                         # nothing measured there: H0 exactly
                    empty = torch.from_numpy(t['count'] == 0)
                    assert bool(empty.any()) and torch.equal(H.cpu()[empty], torch.from_numpy(H0)[empty])


# ---- 2. the reference's recorded runs -------------------------------------------------------------------------------------------
G22 = load_golden('g22_fold_in')
G20 = load_golden('g20_masked_fit')


def _golden_problem(g):
    return g['indices'], g['values'], g['W0'], g['H0'], tuple(int(x) for x in g['shape'])


@pytest.mark.parametrize('case', [str(c) for c in G22['cases']])
def test_golden_g22(dev, case):
    from torchnmf_amd.nmf import NMF
    beta, alpha, l1_ratio, missing = (float(x) for x in G22[case + '_par'])
    idx, vals, W0, H0, shape = _golden_problem(G22)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0[:3])).to(dev)       # (its own H plays no part)
    keep = {k: v.detach().clone() for k, v in m.named_parameters()}
    H, cnt = m.transform(_sparse(idx, vals, shape, dev), beta, int(G22['iterations']), 0.0, alpha, l1_ratio,
                         unstored='missing' if missing else 'zero', H0=torch.from_numpy(H0).to(dev), return_n_iter=True)
    assert bool((cnt == int(G22['iterations'])).all())
    assert all(torch.equal(v, keep[k]) for k, v in m.named_parameters())
    err = rel_err(H.cpu(), G22[case + '_H'])
    record('fold_in_g22', case=case, rel_H=err, tol=TOL)
    print(f'fold_in_g22 {case}: H {err:.2e}')
    assert err <= TOL, (case, err)


def test_golden_g20_frozen_w(dev):
    case = 'b1.5_frozenW'
    prob = _golden_problem(G20)
    H, _ = _fold(dev, prob, 1.5, 'missing', max_iter=int(G20['iterations']))
    err = rel_err(H.cpu(), G20[case + '_H'])
    record('fold_in_g20', case=case, rel_H=err, tol=TOL)
    print(f'fold_in_g20 {case}: H {err:.2e}')
    assert err <= TOL, err


# ---- 3. bitwise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [33, 200])
@pytest.mark.parametrize('mode,beta', [('missing', 0.5), ('missing', 1), ('zero', 1), ('zero', 2)])
def test_bitwise_properties(dev, mode, beta, R):
    from torchnmf_amd.metrics import SparseTarget
    K = 6
    for which in ('a', 'b'):
        prob = _problem(which, R)
        idx, vals, W0, H0, shape = prob
        V = _sparse(idx, vals, shape, dev)
        for reg in (False, True):
            H, cnt = _fold(dev, prob, beta, mode, reg, K)
            assert bool((cnt == K).all()) and bool(torch.isfinite(H).all())
            H2, cnt2 = _fold(dev, prob, beta, mode, reg, K)
            assert torch.equal(H, H2) and torch.equal(cnt, cnt2)                                   # a repeated call
            assert torch.equal(H, _fold(dev, prob, beta, mode, reg, K, _block=8)[0])               # the block size ...
            Hs = _fold(dev, prob, beta, mode, reg, K, **SMALL)[0]
            assert torch.equal(Hs, _fold(dev, prob, beta, mode, reg, K, _long_rows=16)[0])         # ... at either threshold
            assert torch.equal(H, _fold(dev, prob, beta, mode, reg, K, target=SparseTarget(V))[0])  # tensor / SparseTarget
            # a shuffled subset of the rows: the same bits per row
            g = np.random.default_rng(R + shape[0])
            pick = g.permutation(shape[0])[: max(3, 2 * shape[0] // 3)]
            sub_rows = np.concatenate([np.full(int((idx[0] == r).sum()), i) for i, r in enumerate(pick)]).astype(np.int64)
            sel = np.concatenate([np.flatnonzero(idx[0] == r) for r in pick]).astype(np.int64)
            sub = (np.stack([sub_rows, idx[1][sel]]), vals[sel], W0, H0[pick], (len(pick), shape[1]))
            for kw in ({}, SMALL):
                full = H if not kw else Hs
                assert torch.equal(_fold(dev, sub, beta, mode, reg, K, **kw)[0], full[torch.from_numpy(pick).to(dev)])
        # max_iter = 0: H0, no iteration counted
        H, cnt = _fold(dev, prob, beta, mode, False, 0)
        assert torch.equal(H.cpu(), torch.from_numpy(H0)) and bool((cnt == 0).all())


def test_target_without_entries(dev):
    _, _, W0, H0, shape = _problem('a', 33)
    prob = (np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.float32), W0, H0, shape)
    H, cnt = _fold(dev, prob, 0.5, 'missing', max_iter=3)
    assert torch.equal(H.cpu(), torch.from_numpy(H0)) and bool((cnt == 3).all())
    H, cnt = _fold(dev, prob, 1, 'zero', max_iter=1)
    ref, bound, _ = F.iteration(prob[0], prob[1], shape, H0, W0, 1, 'zero')
    assert F.check(H.double().cpu().numpy(), ref, bound)[1]


# ---- 4. the stop rule ------------------------------------------------------------------------------------------------------------
STOP_MAX = 30
# tol = 1e-3 where that leaves the inputs mixed -- at least a quarter of the rows stop before STOP_MAX and at least one does
# not -- and 1e-2 where 1e-3 stops too few within 30 iterations (beta = 2 with unstored zeros; the 9-row target).  Chosen
# from the float64 model (fold_in_emulation.run), which gives for the seven cases 13 / 12 / 12 / 14 / 28 of 37 and 4 / 7 of 9
# early rows; the condition is asserted below on the states the device returns.
STOP_CASES = [('a', 3, 'missing', 1, 1e-3), ('a', 33, 'missing', 0.5, 1e-3), ('a', 200, 'missing', 1, 1e-3),
              ('a', 3, 'zero', 1, 1e-3), ('a', 3, 'zero', 2, 1e-2), ('b', 33, 'missing', 0.5, 1e-2), ('b', 3, 'zero', 2, 1e-2)]


@pytest.mark.parametrize('kw', [{}, SMALL], ids=['default', 'small'])
@pytest.mark.parametrize('which,R,mode,beta,STOP_TOL', STOP_CASES)
def test_stop_rule(dev, which, R, mode, beta, STOP_TOL, kw):
    prob = _problem(which, R)
    n = prob[4][0]
    sts = [torch.from_numpy(prob[3]).to(dev)]
    for _ in range(STOP_MAX):                                              # the states of tol = 0, one iteration per call
        sts.append(_fold(dev, prob, beta, mode, max_iter=1, H0=sts[-1], **kw)[0])
    assert torch.equal(sts[-1], _fold(dev, prob, beta, mode, max_iter=STOP_MAX, **kw)[0])
    H, cnt = _fold(dev, prob, beta, mode, max_iter=STOP_MAX, tol=STOP_TOL, **kw)
    # the criterion, recomputed in fp32 from the states k - 1 and k
    want = torch.full((n,), STOP_MAX, dtype=torch.int32)
    tol32 = torch.tensor(STOP_TOL, dtype=torch.float32)
    for k in range(STOP_MAX, 0, -1):
        a, b = sts[k - 1].cpu(), sts[k].cpu()
        hit = (b - a).abs().amax(1) <= tol32 * b.amax(1)
        want[hit] = k
    assert np.array_equal(want.numpy(), F.stop_counts([s.cpu().numpy() for s in sts], STOP_TOL))
    early = int((want < STOP_MAX).sum())
    print(f'fold_in_stop {which} R={R} {mode} beta={beta}: counts {sorted(want.tolist())}')
    record('fold_in_stop', target=which, R=R, mode=mode, beta=beta, tol=STOP_TOL, small=bool(kw), early=early, rows=n)
    assert 4 * early >= n and early < n                                    # a condition on the inputs
    assert torch.equal(cnt.cpu(), want)
    for i in range(n):
        assert torch.equal(H[i], sts[int(want[i])][i]), i                  # bitwise the state its count names


# ---- 5. against the frozen-W fit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,beta', [('missing', 0.5), ('missing', 1), ('missing', 2), ('zero', 1), ('zero', 2)])
def test_against_frozen_w_fit(dev, mode, beta):
    from torchnmf_amd.nmf import NMF
    for which, R in (('a', 33), ('b', 100)):
        idx, vals, W0, H0, shape = _problem(which, R)
        V = _sparse(idx, vals, shape, dev)
        for reg in (False, True):
            a, r = (ALPHA, L1_RATIO) if reg else (0, 0)
            m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0), trainable_W=False).to(dev)
            assert m.fit(V, beta=beta, max_iter=5, alpha=a, l1_ratio=r, unstored=mode) == 5
            got = m.transform(V, beta, 5, 0.0, a, r, unstored=mode, H0=torch.from_numpy(H0).to(dev))
            err = rel_err(got.cpu(), m.H.data.cpu())
            record('fold_in_vs_fit', mode=mode, beta=beta, target=which, R=R, reg=reg, rel_H=err, tol=TOL)
            print(f'fold_in_vs_fit {mode} beta={beta} {which} R={R} reg={reg}: {err:.2e}')
            assert err <= TOL, err


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def test_double_module_and_topk(dev):
    from torchnmf_amd.metrics import topk_scores
    from torchnmf_amd.nmf import NMF
    idx, vals, W0, H0, shape = _problem('a', 33)
    V = _sparse(idx, vals, shape, dev)
    m = NMF(W=torch.from_numpy(W0), rank=33).double().to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    H = m.transform(V, unstored='missing', generator=g)
    assert H.dtype == torch.float64 and H.shape == (37, 33) and not H.requires_grad and bool((H >= 0).all())
    assert torch.equal(H, m.transform(V, unstored='missing', generator=torch.Generator(device=dev).manual_seed(3)))
    H32 = NMF(W=torch.from_numpy(W0), rank=33).to(dev).transform(V, unstored='missing',
                                                                generator=torch.Generator(device=dev).manual_seed(3))
    assert H32.dtype == torch.float32 and torch.equal(H32.double(), H)
    top = topk_scores(H32, m.W.float(), 5, exclude=V)
    stored = set(zip(idx[0].tolist(), idx[1].tolist()))
    ind = top.indices.cpu().numpy()
    assert ind.shape == (37, 5) and ind.min() >= 0
    assert not any((i, int(j)) in stored for i in range(37) for j in ind[i])


# ---- the checks of fold_in that read the data (behind the device check: they cannot run on CPU tensors) --------------------------
def test_data_checks_in_order(dev):
    from torchnmf_amd.fold_in import fold_in
    W = torch.rand(9, 4, device=dev)
    ij = torch.tensor([[0, 1, 2], [2, 3, 5]])

    def sp(*v):
        return torch.sparse_coo_tensor(ij, torch.tensor(v), (3, 9)).to(dev)
    bad_h0 = -torch.ones(3, 4, device=dev)
    with pytest.raises(AssertionError, match='Target should be non-negative'):
        fold_in(W, sp(1.0, -1.0, 0.0), beta=0, unstored='zero', H0=bad_h0)       # every later check would answer as well
    for kw in (dict(beta=0, unstored='zero'), dict(beta=-1, unstored='zero'), dict(beta=0, unstored='missing'),
               dict(beta=-1, unstored='missing')):
        with pytest.raises(ValueError, match='beta <= 0 and V contains zeros'):
            fold_in(W, sp(1.0, 2.0, 0.0), H0=bad_h0, **kw)
    fold_in(W, sp(1.0, 2.0, 0.5), beta=-1, unstored='missing', max_iter=2)       # strictly positive: admitted
    fold_in(W, sp(1.0, 2.0, 0.0), beta=0.5, unstored='missing', max_iter=2)      # a stored zero with beta > 0: admitted
    for beta in (0.5, 1.5, 3):
        with pytest.raises(NotImplementedError, match='trainable_W=False'):
            fold_in(W, sp(1.0, 2.0, 0.5), beta=beta, unstored='zero', H0=bad_h0)
    with pytest.raises(AssertionError, match='should be non-negative'):
        fold_in(W, sp(1.0, 2.0, 0.5), H0=bad_h0)
    with pytest.raises(AssertionError, match='should be non-negative'):
        fold_in(W, sp(1.0, 2.0, 0.5), H0=bad_h0, max_iter=0)
