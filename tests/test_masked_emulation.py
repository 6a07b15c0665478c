"""The float64 reference of missing-data NMF (tests/masked_emulation.py) against the reference's own runs (g20_masked_fit:
its update rule driven on the gathered graph, tools/make_golden_masked.py), on the CPU."""
import numpy as np
import pytest

import masked_emulation as M
from conftest import load_golden

G = load_golden('g20_masked_fit')
CASES = [str(c) for c in G['cases']]


def test_fixture_shape():
    N, C = (int(x) for x in G['shape'])
    idx = G['indices']
    assert (N, C) == (37, 29) and G['W0'].shape == (29, 5) and G['H0'].shape == (37, 5)
    assert 0.25 < idx.shape[1] / (N * C) < 0.35
    assert 11 not in idx[0] and 7 not in idx[1]                       # one row and one column without entries
    assert float(G['values'].min()) >= 0.1                            # strictly positive: beta <= 0 is admissible
    betas = sorted({float(G[c + '_par'][0]) for c in CASES})
    assert betas == [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0] and len(CASES) == 15
    assert sum(float(G[c + '_par'][3]) == 0.0 for c in CASES) == 1    # the frozen-W case


@pytest.mark.parametrize('case', CASES)
def test_emulation_matches_reference(case):
    beta, alpha, l1_ratio, update_W = (float(x) for x in G[case + '_par'])
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    idx, vals, shape = G['indices'], G['values'], tuple(int(x) for x in G['shape'])
    W, H = G['W0'].astype(np.float64), G['H0'].astype(np.float64)
    for _ in range(int(G['iterations'])):
        if update_W:
            W = M.step(idx, vals, shape, H, W, beta, 'w', l1, l2)[0]
        H = M.step(idx, vals, shape, H, W, beta, 'h', l1, l2)[0]
    # two float64 implementations of the same 20 iterations
    assert np.abs(W - G[case + '_W']).max() <= 1e-9 * np.abs(G[case + '_W']).max()
    assert np.abs(H - G[case + '_H']).max() <= 1e-9 * np.abs(G[case + '_H']).max()
    if alpha == 0:                                                    # rows / columns without entries stay as they were
        assert np.array_equal(H[11], G['H0'][11].astype(np.float64))
        if update_W:
            assert np.array_equal(W[7], G['W0'][7].astype(np.float64))
    got, bound = M.loss(idx, vals, H, W, beta)
    assert abs(got - float(G[case + '_loss'])) <= 1e-9 * abs(float(G[case + '_loss']))
    assert 0 < bound < 1e-4 * abs(got)


@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 1.5, 2, 3])
def test_loss_regrouping(beta):
    """``loss`` splits metrics.beta_div into the terms of v alone and the terms that hold s, as the kernel does."""
    idx, vals, W0, H0 = M.make_problem(37, 29, 33)
    a, _ = M.loss(idx, vals, H0, W0, beta)
    b = M.dense_loss(idx, vals, H0, W0, beta)
    assert abs(a - b) <= 1e-11 * abs(b)


@pytest.mark.parametrize('axis', [0, 1])
def test_problem_structure(axis):
    idx, vals, W0, H0 = M.make_problem(37, 29, 3, axis)
    own = np.bincount(idx[axis], minlength=(37, 29)[axis])
    assert set(M.COUNTS) == set(own.tolist())
    assert 3 not in idx[1 - axis]
    assert np.all(np.diff(idx[0] * 29 + idx[1]) > 0)                   # coalesced order, no duplicates
    assert vals.min() >= 0.1 and vals.max() < 2 and W0.min() >= 0.1 and H0.max() < 1
    segs = M.segments(own, 8)
    assert segs[own == 8].max() == 1 and segs[own == 9].min() == 2 and segs[own == 20].min() == 3 and segs[own == 0].min() == 1


def test_terms_are_the_gradient():
    """den - num is the gradient of the masked loss (checked by central differences in float64)."""
    idx, vals, W0, H0 = M.make_problem(14, 24, 3)
    H, W = H0.astype(np.float64), W0.astype(np.float64)
    for beta in (-1, 0, 0.5, 1, 2, 3):
        t = M.terms(idx, vals, (14, 24), H, W, beta, 'h')
        g = t['den'] - t['num']
        for (i, r) in ((0, 1), (5, 2), (8, 0)):
            d = np.zeros_like(H)
            d[i, r] = 1e-6
            fd = (M.dense_loss(idx, vals, H + d, W, beta) - M.dense_loss(idx, vals, H - d, W, beta)) / 2e-6
            assert abs(fd - g[i, r]) <= 1e-6 * max(1.0, abs(g[i, r])), (beta, i, r)
        assert np.all(t['num_bound'] >= 0) and np.all(t['den_bound'][t['count'] > 0] > 0)
        assert np.all(t['num'][t['count'] == 0] == 0) and np.all(t['den'][t['count'] == 0] == 0)
