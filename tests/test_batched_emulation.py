"""The float64 model of batched NMF (tests/batched_emulation.py) on the CPU: its half-steps against the dense multiplicative
update of oracle/mu_oracle.py (the port of the reference's _double_backward_update this repository keeps) on tiny problems, its
stop rule on hand-made numbers, and its whole ``fit`` loop -- counts, frozen problems, the NaN loss -- against the reference's
own ``NMF.fit`` runs (golden g24, tools/make_golden_batched.py)."""
import numpy as np
import pytest
import torch

import batched_emulation as BE
from conftest import load_golden
from oracle import mu_oracle as O

G = load_golden('g24_batched_fit')
CASES = [str(c) for c in G['cases']]
TOL, MAX_ITER = float(G['tol']), int(G['max_iter'])


def test_fixture_shape():
    assert G['V'].shape == (6, 37, 29) and G['W0'].shape == (6, 29, 5) and G['H0'].shape == (6, 37, 5)
    assert G['V'].dtype == G['W0'].dtype == G['H0'].dtype == np.float32
    assert float(G['V'].min()) > 0 and float(G['W0'].min()) >= 0.1 and float(G['H0'].max()) < 1
    assert CASES == ['b0.5', 'b1', 'b2', 'b1_reg', 'b2_frozenW'] and (TOL, MAX_ITER) == (1e-3, 80)
    for beta in ('b0.5', 'b1', 'b2'):            # per beta: one problem stops early, one runs to the end
        n = G[beta + '_n_iter']
        assert n.min() < MAX_ITER and n.max() == MAX_ITER and np.all(n % 10 == 0)
    assert tuple(G['b1_reg_par']) == (1.0, 0.07, 0.3, 1.0) and tuple(G['b2_frozenW_par']) == (2.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 1.5, 2, 3])
def test_half_steps_are_the_dense_update(beta):
    """Every problem of a tiny batch: the step is the reference's dense update.  (beta == 1: the oracle takes the closed-form
    denominator, the panel's column sums, WITHOUT relu + eps (nmf.py:122-131) where the kernel's rule adds eps: a relative
    eps / den of the multiplier.)"""
    V, W0, H0 = BE.make_problems(3, 23, 31, 4)
    gam = O.gamma_of(beta)
    for b in range(3):
        Vb, W, H = V[b].astype(np.float64), W0[b].astype(np.float64), H0[b].astype(np.float64)
        Vt, Wt, Ht = (torch.from_numpy(x) for x in (Vb, W, H))
        for l1, l2 in ((0.0, 0.0), (0.021, 0.049)):
            Wr = O.nmf_w_step(Vt, Wt, Ht, beta, gam, l1, l2).numpy()
            Hr = O.nmf_h_step(Vt, torch.from_numpy(Wr), Ht, beta, gam, l1, l2).numpy()
            Wn = BE.step(Vb, H, W, beta, 'w', l1, l2)[0]
            Hn = BE.step(Vb, H, Wr, beta, 'h', l1, l2)[0]
            tol = 1e-12 if beta != 1 else 2 * BE.EPS / min(H.sum(0).min(), Wr.sum(0).min())
            assert np.abs(Wn - Wr).max() <= tol * np.abs(Wr).max() and np.abs(Hn - Hr).max() <= tol * np.abs(Hr).max()
        x = torch.from_numpy(H @ W.T)
        ref = float(O.beta_div(x, Vt, beta))
        got, bound = BE.loss(Vb, H, W, beta)
        assert abs(got - ref) <= 1e-11 * abs(ref) and 0 < bound < 1e-4 * abs(ref)
        assert abs(BE.dense_loss(Vb, H, W, beta) - ref) <= 1e-11 * abs(ref)


def test_a_shared_target_is_every_problems_target():
    V, W0, H0 = BE.make_problems(2, 14, 9, 3)
    a = BE.fit(V[0], W0, H0, 1.0, -1e9, 3)
    b = BE.fit(np.stack([V[0], V[0]]), W0, H0, 1.0, -1e9, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tolist() == [3, 3]


def test_judge():
    div = np.array([2.0, 0.5, -1e-9, 8.0, 0.5])
    loss_init = np.array([4.0, 2.0, 3.0, 4.0, 2.0])
    previous = np.array([2.002, 1.5, 3.0, 4.0, 1.0])
    active = np.array([1, 1, 1, 1, 0], dtype=np.int32)
    n_iter = np.full(5, 80, dtype=np.int64)
    # problem 0: loss 2, (2.002 - 2) / 4 = 5e-4 < 1e-3 stops; 1: loss 1, 0.25 goes on; 2: NaN goes on; 3: loss 4, 0 < tol
    # stops; 4: already stopped, untouched
    alive = BE.judge(div, loss_init, previous, 1e-3, 19, active, n_iter)
    assert alive == 2 and active.tolist() == [0, 1, 1, 0, 0] and n_iter.tolist() == [20, 80, 80, 20, 80]
    assert previous[0] == 2.002 and previous[1] == 1.0 and np.isnan(previous[2]) and previous[3] == 4.0 and previous[4] == 1.0
    # a NaN `previous` cannot stop the problem at the next checkpoint either: the comparison is False again
    div[2] = 4.5
    assert BE.judge(div, loss_init, previous, 1e-3, 29, active, n_iter) == 1      # (1 stops: loss unchanged; 2 goes on)
    assert active.tolist() == [0, 0, 1, 0, 0] and n_iter.tolist() == [20, 30, 80, 20, 80] and previous[2] == 3.0
    assert np.isnan(BE.sqrt2(-1e-300)) and BE.sqrt2(0.0) == 0.0 and BE.sqrt2(8.0) == 4.0


@pytest.mark.parametrize('case', CASES)
def test_fit_matches_the_reference(case):
    """Counts equal the reference's for every problem; the factors of a problem -- frozen at its own stop iteration while the
    others went on -- are the reference's.  Two float64 implementations of the same iterations: 1e-9.  beta == 1: the
    reference's closed-form denominator has no eps (above), a relative eps / den of the multiplier per half-step, den a column
    sum of the panel: at least 29 entries that start at 0.1 or more, so >= 2.9 (asserted at the end as well), eps / den <=
    4.1e-8; at most 160 half-steps, 6.6e-6 if every one of them pushed the same way: the bar is 1e-5.  The counts cannot move
    with it: the fixture keeps every decision 0.05 tol = 5e-5 of loss_init away from its threshold."""
    beta, alpha, l1_ratio, update_W = (float(x) for x in G[case + '_par'])
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    W, H, n_iter, trace = BE.fit(G['V'], G['W0'], G['H0'], beta, TOL, MAX_ITER, l1, l2, update_W=bool(update_W))
    assert n_iter.tolist() == G[case + '_n_iter'].tolist()
    bar = 1e-5 if beta == 1 else 1e-9
    for b in range(6):
        assert np.abs(W[b] - G[case + '_W'][b]).max() <= bar * np.abs(G[case + '_W'][b]).max(), b
        assert np.abs(H[b] - G[case + '_H'][b]).max() <= bar * np.abs(G[case + '_H'][b]).max(), b
        got = BE.loss(G['V'][b], H[b], W[b], beta)[0]
        assert abs(got - G[case + '_div'][b]) <= 10 * bar * abs(G[case + '_div'][b])
        assert len(trace[b]) == 1 + n_iter[b] // 10            # judged at every 10th iteration until it stopped
        t = trace[b]
        if alpha == 0:
            assert all(y <= x for x, y in zip(t, t[1:]))        # MU without a penalty: the loss never grows
    if beta == 1:
        assert min(W.sum(1).min(), H.sum(1).min()) >= 2.9
    if not update_W:
        assert np.array_equal(W, G['W0'].astype(np.float64))


def test_a_stopped_problem_is_frozen():
    """A problem that stopped at k holds exactly what a run of k iterations gives it, in whatever company."""
    n_ref = G['b2_n_iter']
    W, H, n_iter, _ = BE.fit(G['V'], G['W0'], G['H0'], 2.0, TOL, MAX_ITER)
    for b in (4, 5):
        assert n_ref[b] < MAX_ITER
        Wk, Hk, nk, _ = BE.fit(G['V'][b:b + 1], G['W0'][b:b + 1], G['H0'][b:b + 1], 2.0, -1e9, int(n_ref[b]))
        assert nk.tolist() == [n_ref[b]] and np.array_equal(Wk[0], W[b]) and np.array_equal(Hk[0], H[b])


def test_a_negative_divergence_never_stops():
    """Problem 5 would stop at 40; handed a negative divergence at every checkpoint its loss is NaN and it runs to max_iter,
    while the others stop where they did."""
    V, W0, H0 = G['V'], G['W0'], G['H0']

    def loss_fn(b, H, W):
        return -1e-7 if b == 5 else BE.loss(V[b], H, W, 2.0)[0]
    _, _, n_iter, trace = BE.fit(V, W0, H0, 2.0, TOL, MAX_ITER, loss_fn=loss_fn)
    want = G['b2_n_iter'].tolist()
    assert want[5] < MAX_ITER and n_iter.tolist() == want[:5] + [MAX_ITER]
    assert all(np.isnan(x) for x in trace[5]) and len(trace[5]) == 1 + MAX_ITER // 10
