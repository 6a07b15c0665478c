"""The float64 model of solver='hals' (tests/hals_emulation.py) on its own, no GPU: descent, the convergence claim the feature
stands on, the update against sklearn's coordinate descent, the initial scale, and the per-element check applied to an fp32
numpy rendering of the kernel's accumulation scheme."""
import numpy as np
import pytest

import hals_emulation as E


@pytest.mark.parametrize('name', ['dense', 'sparse'])
@pytest.mark.parametrize('reg', [(0.0, 0.0), (0.021, 0.049)])
def test_objective_never_increases(name, reg):
    """Every coordinate step minimises the regularised objective along its coordinate from factors >= eps (the floor and the
    eps in the denominator only shorten the step): non-increasing over every half-step of 10 iterations."""
    V, W0, H0 = E.fit_case(name)
    trace = []
    E.fit(V, W0, H0, 10, l1=reg[0], l2=reg[1], trace=trace)
    trace = np.array(trace)
    assert len(trace) == 21
    assert (np.diff(trace) <= 1e-12 * trace[:-1]).all(), np.diff(trace).max()
    if reg == (0.0, 0.0):
        # the margin the GPU test's 1e-5 tolerance leans on: every iteration gains more than 1e-3 of the objective
        per_iter = (trace[:-2:2] - trace[2::2]) / trace[2::2]
        assert per_iter.min() > 1e-3, per_iter.min()


@pytest.mark.parametrize('name,hals20,mu40', [('dense', 608.2186, 745.5664), ('sparse', 310.3098, 318.4808)])
def test_hals_20_beats_mu_40(name, hals20, mu40):
    """1/2 |V - H W^T|^2 in float64 from the same |randn| factors (HALS scales them first, that is part of it):

        target                         HALS, 20 iterations    MU, 40 iterations    margin
        dense 200 x 130, rank 33       608.2186               745.5664             18.4 %
        5 %-dense 300 x 257, rank 64   310.3098               318.4808              2.57 %

    (1/2 |V|^2 = 4339.26 and 625.48.)  The seeds are chosen so that this emulation alone shows at least 2 %."""
    V, W0, H0 = E.fit_case(name)
    W, H, n = E.fit(V, W0, H0, 20)
    Wm, Hm = E.mu_fit(V, W0, H0, 40)
    h, m = E.divergence(V, W, H), E.divergence(V, Wm, Hm)
    assert n == 20
    assert h == pytest.approx(hals20, rel=1e-6) and m == pytest.approx(mu40, rel=1e-6)
    assert h < 0.98 * m


def test_half_step_is_sklearn_coordinate_descent():
    """With floor = den_eps = 0 one half-step is sklearn's _update_cdnmf_fast with the identity permutation."""
    cd = pytest.importorskip('sklearn.decomposition._cdnmf_fast')
    rng = np.random.default_rng(11)
    X = rng.random((60, 45))
    Wsk = np.abs(rng.standard_normal((60, 9)))            # sklearn: X (n, m) ~ W (n, k) @ H (k, m)
    Hsk = np.abs(rng.standard_normal((9, 45)))
    for shrink in (1.0, 0.3):                             # (0.3: a target the factors overshoot -- many coordinates clamp at 0)
        got = E.half_step(X * shrink, Wsk, Hsk.T, floor=0.0, den_eps=0.0)
        want = np.ascontiguousarray(Wsk.copy())
        HHt = np.ascontiguousarray(Hsk @ Hsk.T)
        XHt = np.ascontiguousarray((X * shrink) @ Hsk.T)
        cd._update_cdnmf_fast(want, HHt, XHt, np.arange(9, dtype=np.intp))
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        if shrink < 1:
            assert (want == 0).any() and (want > 0).any()


def test_optimal_scale_is_the_scalar_minimiser():
    V, W0, H0 = E.fit_case('dense')
    a = E.optimal_scale(V, W0, H0)
    loss = lambda t: ((V - t * (H0 @ W0.T)) ** 2).sum()
    lo, hi = 0.0, 10 * a                                   # golden-section search on the (convex) scalar problem
    g = (5 ** 0.5 - 1) / 2
    for _ in range(200):
        x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
        if loss(x1) < loss(x2):
            hi = x2
        else:
            lo = x1
    assert abs(0.5 * (lo + hi) - a) <= 1e-6 * a
    # both trainable: sqrt(a) each; one trainable: a on that one; the product is scaled by a either way
    for tw, th in ((True, True), (True, False), (False, True)):
        W, H = E.init_scale(V, W0, H0, tw, th)
        assert np.allclose(H @ W.T, a * (H0 @ W0.T), rtol=1e-12, atol=1e-6)
        assert tw or (W == W0).all()
        assert th or (H == H0).all()
    # a target orthogonal to the model gives a = 0: skipped, only the floor is applied
    W, H = E.init_scale(np.zeros_like(V), W0, H0)
    assert (W == np.maximum(W0, E.EPS)).all() and (H == np.maximum(H0, E.EPS)).all()


def _kernel_scheme_fp32(F, A, G, l1, l2):
    """The kernel's arithmetic in numpy fp32: four interleaved accumulators (products rounded, where the kernel fuses: the
    bound has room for that), (acc0 + acc1) + (acc2 + acc3), the own term an exact +0."""
    f32 = np.float32
    F = F.copy()
    rows, R = F.shape
    for r in range(R):
        F[:, r] = 0
        acc = np.zeros((4, rows), dtype=f32)
        for j in range(R):
            acc[j & 3] = acc[j & 3] + F[:, j] * G[j, r]
        s = (acc[0] + acc[1]) + (acc[2] + acc[3])
        num = (A[:, r] - f32(l1)) - s
        den = (G[r, r] + f32(l2)) + f32(E.EPS)
        F[:, r] = np.maximum(f32(E.EPS), num / den)
    return F


@pytest.mark.parametrize('rows,rank', [(65, 3), (63, 33), (30, 100)])
@pytest.mark.parametrize('reg', [(0.0, 0.0), (0.021, 0.049)])
def test_sweep_check_accepts_fp32_and_rejects_an_ulp_scale_error(rows, rank, reg):
    F, A, G = E.sweep_case(rows, rank)
    assert (G == G.T).all() and G[rank // 2, rank // 2] < 1e-9 and (A[rows // 2] == 0).all()
    got = _kernel_scheme_fp32(F, A, G, *reg)
    clamped = got == np.float32(E.EPS)
    assert clamped.any() and (~clamped).any()
    err, bound = E.sweep_check(got, F, A, G, *reg)
    assert (err <= bound).all(), (err / bound).max()
    # the check has teeth: one element off by a relative 1e-3 is caught at that element (it also moves the references of the
    # coordinates after it, which is why only the first failure is pinned)
    i, r = np.argwhere(~clamped)[0]
    bad = got.copy()
    bad[i, r] *= np.float32(1.001)
    err, bound = E.sweep_check(bad, F, A, G, *reg)
    assert err[i, r] > bound[i, r]
    # ... and so is a sweep that used stale values (Jacobi instead of Gauss-Seidel)
    if rank > 1:
        jac = np.maximum(E.EPS, (A.astype(np.float64) - np.float32(reg[0])
                                 - (F.astype(np.float64) @ G.astype(np.float64) - F * np.diag(G).astype(np.float64)))
                         / (np.diag(G).astype(np.float64) + np.float32(reg[1]) + E.EPS)).astype(np.float32)
        err, bound = E.sweep_check(jac, F, A, G, *reg)
        assert (err > bound).any()


def test_bound_constant():
    assert [E.bound_c(r) for r in (1, 3, 4, 5, 33, 128, 256)] == [8, 8, 8, 9, 16, 39, 71]
