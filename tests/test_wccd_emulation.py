"""CPU checks of tests/wccd_emulation.py, the float64 model the GPU tests of ``fit(solver='ccd', unstored=omega)`` compare the
device against: every coordinate update against a dense brute force on an explicit weight matrix, the loss identity, the two
end points (omega = 0: ``ccd_emulation.sweep``; omega = 1: the HALS sweep on the densified target), rows without entries, and
the per-element check applied to an fp32 model of the kernel's own arithmetic (so that the bound's constants are tried before
any device run, and shown to be able to fail)."""
import numpy as np
import pytest

import ccd_emulation as CE
import hals_emulation as HE
import wccd_emulation as E

REG = (0.021, 0.049)
OMEGAS = (0.0625, 0.3)


@pytest.mark.parametrize('omega', OMEGAS)
@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_every_coordinate_update_is_the_dense_argmin_and_descends(reg, omega):
    n_panel = 90
    F, P, ptr, cols, vals = E.sweep_case([0, 1, 5, 64, 65, 0, 90], n_panel, 7, seed=3)
    F, P = F.astype(np.float64), P.astype(np.float64)
    X, Wt = E.dense(ptr, cols, vals, n_panel, omega)
    assert (Wt == 1.0).sum() == len(cols) and Wt[0].max() == omega and (Wt[6] == 1.0).all()
    G, c = P.T @ P, 1.0 - omega
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        Pi, v = P[cols[a:b]], vals[a:b].astype(np.float64)
        f = F[i].copy()
        t = v - c * (Pi @ f)
        before = E.row_objective(f, P, X[i], Wt[i], *reg)
        for k in range(F.shape[1]):
            p = Pi[:, k]
            fn = E.minimiser(f[k], p @ p, t @ p, f @ G[k], G[k, k], omega, *reg)
            brute = E.brute_minimiser(f, k, P, X[i], Wt[i], *reg)
            assert abs(fn - brute) <= 1e-11 * max(1.0, abs(brute)), (i, k, fn, brute)
            t -= c * (fn - f[k]) * p
            f[k] = fn
            after = E.row_objective(f, P, X[i], Wt[i], *reg)
            # (the eps in the denominator shortens the step by a factor 1 - eps / den: still a descent step)
            assert after <= before + 1e-12 * max(before, 1.0), (i, k, before, after)
            before = after
        assert np.allclose(t, v - c * (Pi @ f), rtol=0, atol=1e-10)     # the maintained residual is the residual
        assert np.abs(E.sweep(F[i:i + 1], P, [0, b - a], cols[a:b], vals[a:b], omega, *reg)[0] - f).max() <= 1e-12


@pytest.mark.parametrize('omega', OMEGAS)
def test_loss_identity(omega):
    for name in ('small', 'mid'):
        idx, vals, shape, W0, H0 = E.fit_case(name)
        a, b = E.divergence(idx, vals, W0, H0, omega), E.dense_divergence(idx, vals, shape, W0, H0, omega)
        assert abs(a - b) <= 1e-11 * b, (a, b)


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_omega_0_is_the_ccd_sweep(reg):
    F, P, ptr, cols, vals = E.sweep_case([3, 0, 40, 129, 1], 150, 9, seed=4)
    a, b = E.sweep(F, P, ptr, cols, vals, 0.0, *reg), CE.sweep(F, P, ptr, cols, vals, *reg)
    with_entries = np.diff(ptr) > 0
    assert np.abs(a - b)[with_entries].max() <= 1e-11
    assert (a[~with_entries] == E.EPS).all()                # (ccd leaves them as they are; here the minimiser of 0 is the floor)


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_omega_1_is_the_hals_sweep_on_the_densified_target(reg):
    idx, vals, shape, W0, H0 = E.fit_case('small')
    V = np.zeros(shape)
    V[idx[0], idx[1]] = vals
    lh, lw = E.side_list(idx, vals, shape, 'h'), E.side_list(idx, vals, shape, 'w')
    assert np.abs(E.sweep(H0, W0, *lh, 1.0, *reg) - HE.half_step(V, H0, W0, *reg)).max() <= 1e-11
    assert np.abs(E.sweep(W0, H0, *lw, 1.0, *reg) - HE.half_step(V.T, W0, H0, *reg)).max() <= 1e-11


@pytest.mark.parametrize('omega', OMEGAS)
def test_rows_without_entries_end_on_the_floor(omega):
    F, P, ptr, cols, vals = E.sweep_case([0, 4, 0, 0, 70], 100, 5)
    out = E.sweep(F, P, ptr, cols, vals, omega, *REG)
    for i in (0, 2, 3):
        assert (out[i] == E.EPS).all()
    assert E.zero_row([0, 4, 0, 0, 70]) == 1 and (out[1] == E.EPS).all()     # stored zeros only: the floor as well
    assert (out[4] != E.EPS).any()
    idx, vals, shape, W0, H0 = E.fit_case('mid')            # column 5 and row 7 store nothing
    W, H, _ = E.fit(idx, vals, shape, W0, H0, omega, 2)
    assert (W[5] == E.EPS).all() and (H[7] == E.EPS).all()


@pytest.mark.parametrize('omega', OMEGAS)
@pytest.mark.parametrize('name', ['small', 'mid'])
@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_fit_objective_never_increases(name, reg, omega):
    idx, vals, shape, W0, H0 = E.fit_case(name)
    trace, losses = [], []
    W, H, n = E.fit(idx, vals, shape, W0, H0, omega, 10, l1=reg[0], l2=reg[1], trace=trace, losses=losses)
    assert n == 10 and len(trace) == 21
    assert (np.diff(trace) <= 1e-12 * np.array(trace[:-1])).all()
    if reg == (0.0, 0.0):
        assert (np.diff(losses) <= 1e-12 * np.array(losses[:-1])).all()
    assert W.min() >= E.EPS and H.min() >= E.EPS
    assert abs(losses[-1] - E.dense_divergence(idx, vals, shape, W, H, omega)) <= 1e-10 * losses[-1]


def test_initial_scale_minimises_the_weighted_loss():
    idx, vals, shape, W0, H0 = E.fit_case('small')
    W, H = E.init_scale(idx, vals, W0, H0, 0.3)
    base = E.divergence(idx, vals, W, H, 0.3)
    for a in (0.98, 1.02):
        assert E.divergence(idx, vals, W * a, H, 0.3) >= base
    Wf, Hf = E.init_scale(idx, vals, W0, H0, 0.3, train_W=False)
    assert np.array_equal(Wf, W0)
    assert abs(E.divergence(idx, vals, Wf, Hf, 0.3) - base) <= 1e-9 * base      # the same product either way


# ---- the per-element check, on the fp32 model of the kernel --------------------------------------------------------------
@pytest.mark.parametrize('wg_rows', [E.LIMIT, 100])          # 100: the rows of 129 and 200 entries take the workgroup's order
@pytest.mark.parametrize('rank', [1, 3, 33, 65, 100])
@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_fp32_model_meets_its_bound(rank, reg, wg_rows):
    counts = [0, 1, 63, 64, 65, 129, 200]
    F, P, ptr, cols, vals = E.sweep_case(counts, 220, rank, seed=1)
    G = E.gram_f32(P)
    for omega in OMEGAS:
        got = E.sweep_f32(F, P, ptr, cols, vals, omega, *reg, G=G, wg_rows=wg_rows)
        assert np.isfinite(got).all() and (got >= np.float32(E.EPS)).all()
        err, bound = E.sweep_check(got, F, P, G, ptr, cols, vals, omega, *reg, wg_rows=wg_rows)
        assert (bound > 0).all()
        frac = E.fraction(err, bound)
        assert frac.max() <= 1.0, (omega, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
        ref = E.sweep(F, P, ptr, cols, vals, float(np.float32(omega)), *reg, G=G)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()       # (and the model is a model of this recurrence)
        clamped = got[1:] == np.float32(E.EPS)
        assert clamped.any() and ((~clamped).any() or rank == 1)


def test_check_detects_a_wrong_coordinate():
    """An output off by 64 ulp in one coordinate fails the check there (and, through the residual and q, may fail later
    ones); the untouched row still passes."""
    F, P, ptr, cols, vals = E.sweep_case([40, 90], 120, 8, seed=2)
    G = E.gram_f32(P)
    for wg in (E.LIMIT, 50):
        got = E.sweep_f32(F, P, ptr, cols, vals, 0.3, G=G, wg_rows=wg)
        assert E.fraction(*E.sweep_check(got, F, P, G, ptr, cols, vals, 0.3, wg_rows=wg)).max() <= 1.0
        k = int(np.argmax(got[1]))
        got[1, k] *= np.float32(1 + 64 * 2.0 ** -23)
        frac = E.fraction(*E.sweep_check(got, F, P, G, ptr, cols, vals, 0.3, wg_rows=wg))
        assert frac[1, k] > 1.0
        assert frac[0].max() <= 1.0
