"""The float64 reference of weighted NMF (tests/weighted_emulation.py) on the CPU: against the reference's own runs
(g23_weighted_fit: its update rule driven on the gathered graph with every pair repeated as often as its integer weight says,
tools/make_golden_weighted.py), against central differences of the loss, against the unweighted dense formulas of
oracle/mu_oracle.py at M = 1, and against masked_emulation on the stored set for a binary M."""
import numpy as np
import pytest
import torch

import masked_emulation as ME
import weighted_emulation as WE
from conftest import load_golden
from oracle import mu_oracle as O

G = load_golden('g23_weighted_fit')
CASES = [str(c) for c in G['cases']]
BETAS = [-1, 0, 0.5, 1, 1.5, 2, 3]


def test_fixture_shape():
    V, M = G['V'], G['M']
    assert V.shape == M.shape == (37, 29) and G['W0'].shape == (29, 5) and G['H0'].shape == (37, 5)
    assert M.dtype.kind == 'i' and set(np.unique(M).tolist()) == {0, 1, 2, 3}
    assert not M[11].any() and not M[:, 7].any()                      # one row and one column without weight
    assert float(V.min()) >= 0.1                                      # strictly positive: beta <= 0 is admissible
    betas = sorted({float(G[c + '_par'][0]) for c in CASES})
    assert betas == [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0] and len(CASES) == 15
    assert sum(float(G[c + '_par'][3]) == 0.0 for c in CASES) == 1    # the frozen-W case


@pytest.mark.parametrize('case', CASES)
def test_emulation_matches_reference(case):
    beta, alpha, l1_ratio, update_W = (float(x) for x in G[case + '_par'])
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    V, M = G['V'], G['M']
    W, H = WE.iterate(V, M, G['W0'], G['H0'], beta, int(G['iterations']), l1, l2, update_W=bool(update_W))
    # two float64 implementations of the same 20 iterations
    assert np.abs(W - G[case + '_W']).max() <= 1e-9 * np.abs(G[case + '_W']).max()
    assert np.abs(H - G[case + '_H']).max() <= 1e-9 * np.abs(G[case + '_H']).max()
    if alpha == 0:                                                    # the weightless row / column stays as it was
        assert np.array_equal(H[11], G['H0'][11].astype(np.float64))
        if update_W:
            assert np.array_equal(W[7], G['W0'][7].astype(np.float64))
    got, bound = WE.loss(V, M, H, W, beta)
    assert abs(got - float(G[case + '_loss'])) <= 1e-9 * abs(float(G[case + '_loss']))
    assert 0 < bound < 1e-4 * abs(got)


@pytest.mark.parametrize('beta', BETAS)
def test_loss_regrouping(beta):
    """``loss`` splits the weighted divergence into the terms of v alone and the terms that hold y, as the kernel does."""
    V, M, W0, H0 = WE.make_problem(37, 29, 33)
    a, _ = WE.loss(V, M, H0, W0, beta)
    b = WE.dense_loss(V, M, H0, W0, beta)
    assert np.isfinite(b) and abs(a - b) <= 1e-11 * abs(b)


def test_problem_structure():
    V, M, W0, H0 = WE.make_problem(131, 70, 3)
    assert not M[5].any() and not M[:, 3].any()
    z = float((M == 0).mean())
    assert 0.25 < z < 0.4 and M[M > 0].min() >= 0.25 and M.max() < 4
    junk = V[M == 0]
    assert np.isnan(junk).any() and np.isinf(junk).any() and (junk == -1).any() and (junk == 1000).any()
    assert V[M > 0].min() >= 0.1 and V[M > 0].max() < 2 and W0.min() >= 0.1 and H0.max() < 1


def test_terms_are_the_gradient():
    """den - num is the gradient of the weighted loss (central differences in float64), whatever V holds where M == 0."""
    V, M, W0, H0 = WE.make_problem(14, 24, 3)
    H, W = H0.astype(np.float64), W0.astype(np.float64)
    for beta in (-1, 0, 0.5, 1, 2, 3):
        for side, F in (('h', H), ('w', W)):
            t = WE.terms(V, M, H, W, beta, side)
            g = t['den'] - t['num']
            assert np.all(np.isfinite(g))
            for (i, r) in ((0, 1), (6, 2), (8, 0)):
                d = np.zeros_like(F)
                d[i, r] = 1e-6
                Hp, Hm, Wp, Wm = (H + d, H - d, W, W) if side == 'h' else (H, H, W + d, W - d)
                fd = (WE.dense_loss(V, M, Hp, Wp, beta) - WE.dense_loss(V, M, Hm, Wm, beta)) / 2e-6
                assert abs(fd - g[i, r]) <= 1e-6 * max(1.0, abs(g[i, r])), (beta, side, i, r)
            assert np.all(t['num_bound'] >= 0) and np.all(t['den_bound'] >= 0)
            dead = 5 if side == 'h' else 3                            # the weightless row / column: exact zeros
            assert np.all(t['num'][dead] == 0) and np.all(t['den'][dead] == 0) and np.all(t['num_bound'][dead] == 0)


@pytest.mark.parametrize('beta', BETAS)
def test_unit_weights_are_the_dense_update(beta):
    """M = 1: the step is the dense multiplicative update of oracle/mu_oracle.py.  (beta == 1: the oracle takes the closed-form
    denominator, the panel's column sums, WITHOUT relu + eps (nmf.py:122-131) where the weighted rule adds eps: a relative
    eps / den of the multiplier.)"""
    V, _, W0, H0 = WE.make_problem(23, 31, 4)
    V = np.where(np.isfinite(V) & (V > 0), V, 0.5).astype(np.float64)
    M = np.ones_like(V)
    W, H = W0.astype(np.float64), H0.astype(np.float64)
    gam = O.gamma_of(beta)
    Vt, Wt, Ht = (torch.from_numpy(x) for x in (V, W, H))
    for l1, l2 in ((0.0, 0.0), (0.021, 0.049)):
        Wr = O.nmf_w_step(Vt, Wt, Ht, beta, gam, l1, l2).numpy()
        Hr = O.nmf_h_step(Vt, torch.from_numpy(Wr), Ht, beta, gam, l1, l2).numpy()
        Wn = WE.step(V, M, H, W, beta, 'w', l1, l2)[0]
        Hn = WE.step(V, M, H, Wr, beta, 'h', l1, l2)[0]
        tol = 1e-12 if beta != 1 else 2 * WE.EPS / min(H.sum(0).min(), Wr.sum(0).min())
        assert np.abs(Wn - Wr).max() <= tol * np.abs(Wr).max() and np.abs(Hn - Hr).max() <= tol * np.abs(Hr).max()
    x = torch.from_numpy(H @ W.T)
    assert abs(WE.loss(V, M, H, W, beta)[0] - float(O.beta_div(x, Vt, beta))) <= 1e-11 * abs(float(O.beta_div(x, Vt, beta)))


@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 2, 3])
def test_binary_weights_are_the_masked_update(beta):
    """A 0 / 1 mask: terms, step and loss are masked_emulation's on the stored set."""
    V, M, W0, H0 = WE.make_problem(37, 29, 5)
    M = (M > 0).astype(np.float64)
    idx = np.stack(np.nonzero(M))
    vals = V[M > 0]
    H, W = H0.astype(np.float64), W0.astype(np.float64)
    for side in ('h', 'w'):
        a = WE.step(V, M, H, W, beta, side, 0.02, 0.05)
        b = ME.step(idx, vals, V.shape, H, W, beta, side, 0.02, 0.05)
        assert np.abs(a[0] - b[0]).max() <= 1e-13 * np.abs(b[0]).max()
        for k in ('num', 'den'):
            assert np.abs(a[2][k] - b[2][k]).max() <= 1e-13 * max(np.abs(b[2][k]).max(), 1e-300)
    assert abs(WE.loss(V, M, H, W, beta)[0] - ME.loss(idx, vals, H, W, beta)[0]) <= 1e-12 * abs(ME.loss(idx, vals, H, W, beta)[0])


def test_split_rule_and_bound_growth():
    """The chain a term rides is as long as its part: forcing more parts shortens it, and the bound with it."""
    assert [WE.parts_for(70, n) for n in (1, 2, 3, 9)] == [1, 2, 3, 3]       # 3 stages: (64 | 6), (32 | 32 | 6)
    assert [WE.parts_for(131, n) for n in (1, 2, 3)] == [1, 2, 3]            # 5 stages: (96 | 35), (64 | 64 | 3)
    assert WE.part_len(70, 2) == 64 and WE.part_len(131, 2) == 96 and WE.part_len(131, 3) == 64
    assert WE.split(4096, 65536, 128) == 16 and WE.split(65536, 4096, 128) == 1 and WE.split(131, 70, 32) == 1
    V, M, W0, H0 = WE.make_problem(131, 70, 3)
    b1 = WE.terms(V, M, H0, W0, 2, 'h', 1)['num_bound']
    b3 = WE.terms(V, M, H0, W0, 2, 'h', 3)['num_bound']
    live = b1 > 0
    assert np.all(b3[live] < b1[live])
