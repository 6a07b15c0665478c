"""CPU checks of tests/ccd_emulation.py, the float64 model the GPU tests of solver='ccd' compare the device against: the
properties of the recurrence, the whole-fit procedure, and the per-element check applied to an fp32 model of the kernel's own
arithmetic (so that the bound's constants are tried before any device run)."""
import numpy as np
import pytest

import ccd_emulation as E
import hals_emulation as HE

REG = (0.021, 0.049)


def _row_objective(f, Pi, v, l1, l2):
    r = v - Pi @ f
    return 0.5 * float(r @ r) + l1 * f.sum() + 0.5 * l2 * float(f @ f)


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_every_coordinate_update_descends(reg):
    F, P, ptr, cols, vals = E.sweep_case([0, 1, 5, 64, 65, 130], 200, 7, seed=3)
    F, P = F.astype(np.float64), P.astype(np.float64)
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        if a == b:
            continue
        Pi, v = P[cols[a:b]], vals[a:b].astype(np.float64)
        f = F[i].copy()
        r = v - Pi @ f
        before = _row_objective(f, Pi, v, *reg)
        for k in range(F.shape[1]):
            p = Pi[:, k]
            fn = E.minimiser(f[k], p @ p, r @ p, *reg)
            r -= (fn - f[k]) * p
            f[k] = fn
            after = _row_objective(f, Pi, v, *reg)
            # (the eps in the denominator shortens the step by a factor 1 - eps / den: still a descent step)
            assert after <= before + 1e-12 * max(before, 1.0), (i, k, before, after)
            before = after
        assert np.allclose(r, v - Pi @ f, rtol=0, atol=1e-10)          # the maintained residual is the residual


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_sweep_is_gauss_seidel_on_the_rows_own_gram(reg):
    F, P, ptr, cols, vals = E.sweep_case([3, 0, 40, 129, 1], 150, 9, seed=4)
    a = E.sweep(F, P, ptr, cols, vals, *reg)
    b = E.gram_sweep(F, P, ptr, cols, vals, *reg)
    assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_fully_stored_target_is_the_hals_sweep(reg):
    idx, vals, shape, V, W0, H0 = E.full_case()
    lh, lw = E.side_list(idx, vals, shape, 'h'), E.side_list(idx, vals, shape, 'w')
    assert np.abs(E.sweep(H0, W0, *lh, *reg) - HE.half_step(V, H0, W0, *reg)).max() <= 1e-11
    assert np.abs(E.sweep(W0, H0, *lw, *reg) - HE.half_step(V.T, W0, H0, *reg)).max() <= 1e-11
    # and so is the whole procedure: the initial scale over all entries is HALS's
    Wc, Hc, nc = E.fit(idx, vals, shape, W0, H0, E.FULL_ITERS, l1=reg[0], l2=reg[1])
    Wh, Hh, nh = HE.fit(V, W0, H0, E.FULL_ITERS, l1=reg[0], l2=reg[1])
    assert nc == nh == E.FULL_ITERS
    assert np.abs(Wc - Wh).max() <= 1e-6 and np.abs(Hc - Hh).max() <= 1e-6


def test_rows_without_entries_are_unchanged():
    F, P, ptr, cols, vals = E.sweep_case([0, 4, 0, 0, 70], 100, 5)
    out = E.sweep(F, P, ptr, cols, vals, *REG)
    for i in (0, 2, 3):
        assert out[i].tobytes() == F[i].astype(np.float64).tobytes()
    assert (out[1] != F[1]).any() and (out[4] != F[4]).any()
    idx, vals, shape, W0, H0 = E.fit_case('mid')
    W, H, _ = E.fit(idx, vals, shape, W0, H0, 2)
    Ws, Hs = E.init_scale(idx, vals, W0, H0)
    assert np.array_equal(W[5], Ws[5]) and np.array_equal(H[7], Hs[7])     # only the initial scale reached them


@pytest.mark.parametrize('name', ['small', 'mid'])
@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_fit_objective_never_increases(name, reg):
    idx, vals, shape, W0, H0 = E.fit_case(name)
    trace, losses = [], []
    W, H, n = E.fit(idx, vals, shape, W0, H0, 10, l1=reg[0], l2=reg[1], trace=trace, losses=losses)
    assert n == 10 and len(trace) == 21
    assert (np.diff(trace) <= 1e-12 * np.array(trace[:-1])).all()
    if reg == (0.0, 0.0):
        assert (np.diff(losses) <= 1e-12 * np.array(losses[:-1])).all()
    assert W.min() >= E.EPS and H.min() >= E.EPS


def test_initial_scale_minimises_over_the_stored_entries():
    idx, vals, shape, W0, H0 = E.fit_case('small')
    W, H = E.init_scale(idx, vals, W0, H0)
    base = E.divergence(idx, vals, W, H)
    for a in (0.98, 1.02):
        assert E.divergence(idx, vals, W * a, H) >= base
    Wf, Hf = E.init_scale(idx, vals, W0, H0, train_W=False)
    assert np.array_equal(Wf, W0)
    assert abs(E.divergence(idx, vals, Wf, Hf) - base) <= 1e-9 * base      # the same product either way


def test_ccd_beats_masked_mu_after_ten_iterations():
    """The premise of the GPU comparison: from the same (scaled) start, ten iterations of each in float64."""
    idx, vals, shape, W0, H0 = E.fit_case('mid')
    Ws, Hs = E.init_scale(idx, vals, W0, H0)
    Wc, Hc, _ = E.fit(idx, vals, shape, W0, H0, 10)
    Wm, Hm = E.masked_mu_fit(idx, vals, shape, Ws, Hs, 10)
    ccd, mu = E.divergence(idx, vals, Wc, Hc), E.divergence(idx, vals, Wm, Hm)
    assert ccd < 0.8 * mu, (ccd, mu)


# ---- the per-element check, on the fp32 model of the kernel --------------------------------------------------------------
@pytest.mark.parametrize('wg_rows', [E.LIMIT, 100])          # 100: the rows of 129 and 200 entries take the workgroup's order
@pytest.mark.parametrize('rank', [1, 3, 33, 100])
@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_fp32_model_meets_its_bound(rank, reg, wg_rows):
    counts = [0, 1, 63, 64, 65, 129, 200]
    F, P, ptr, cols, vals = E.sweep_case(counts, 220, rank, seed=1)
    got = E.sweep_f32(F, P, ptr, cols, vals, *reg, wg_rows=wg_rows)
    assert np.isfinite(got).all() and (got >= np.float32(E.EPS)).all()
    err, bound = E.sweep_check(got, F, P, ptr, cols, vals, *reg, wg_rows=wg_rows)
    frac = E.fraction(err, bound)
    assert frac.max() <= 1.0, (frac.max(), np.unravel_index(frac.argmax(), frac.shape))
    z = E.zero_row(counts)
    assert (got[z] == np.float32(E.EPS)).all()               # the all-zero row ends on the floor
    assert got[0].tobytes() == F[0].tobytes()                # no entries: untouched
    clamped = got[1:] == np.float32(E.EPS)
    assert clamped.any() and (~clamped).any()


def test_check_detects_a_wrong_coordinate():
    """An output off by 64 ulp in one coordinate fails the check there (and, through the residual, may fail later ones)."""
    F, P, ptr, cols, vals = E.sweep_case([40, 90], 120, 8, seed=2)
    got = E.sweep_f32(F, P, ptr, cols, vals)
    k = int(np.argmax(got[1]))
    got[1, k] *= np.float32(1 + 64 * 2.0 ** -23)
    err, bound = E.sweep_check(got, F, P, ptr, cols, vals)
    assert E.fraction(err, bound)[1, k] > 1.0
    assert E.fraction(err, bound)[0].max() <= 1.0
