"""The float64 model of fold-in by coordinate descent (tests/fold_in_cd_emulation.py) on its own, CPU only: its end points
are the two sweeps the project already has, its fp32 model of the kernel stays inside the bound the GPU test holds the device
to, the check notices a planted error, and the objective it descends on does not rise.
"""
import numpy as np
import pytest

import ccd_emulation as CE
import fold_in_cd_emulation as E
import fold_in_emulation as FE
import hals_emulation as HE
import masked_emulation as M
import wccd_emulation as WE

REG = (0.07 * 0.3, 0.07 * 0.7)
OMEGAS = [0.0, 0.0625, 0.3, 1.0]
K = 6


def _problem(which, R):
    if which == 'a':
        idx, vals, W0, H0 = M.make_problem(37, 29, R, 0)
        shape = (37, 29)
    else:
        idx, vals, W0, H0 = FE.make_wide(R)
        shape = (9, 700)
    return E.work_list(idx, vals, shape), W0, H0, shape, idx


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_omega_0_is_the_iterated_ccd_sweep(reg):
    (ptr, cols, vals), W0, H0, _, _ = _problem('a', 5)
    sts = E.states(H0, W0, ptr, cols, vals, 0.0, K, *reg)
    ref = np.asarray(H0, np.float64)
    for k in range(1, K + 1):
        ref = CE.sweep(ref, W0, ptr, cols, vals, *reg)
        assert np.abs(sts[k] - ref).max() <= 1e-11
    empty = np.diff(ptr) == 0
    assert empty.any() and (sts[K][empty] == H0[empty]).all()           # returned as they came
    H, cnt = E.run(H0, W0, ptr, cols, vals, 0.0, K, 0.0, *reg)
    assert (cnt == K).all() and (H == sts[K]).all()
    H, cnt = E.run(H0, W0, ptr, cols, vals, 0.0, K, 1e-3, *reg)
    assert (cnt[empty] == 1).all() and (H[empty] == H0[empty]).all()    # the stop rule on the unchanged row


@pytest.mark.parametrize('reg', [(0.0, 0.0), REG])
def test_omega_1_is_the_iterated_hals_sweep_on_the_densified_target(reg):
    (ptr, cols, vals), W0, H0, shape, idx = _problem('a', 5)
    V = np.zeros(shape)
    V[idx[0], idx[1]] = vals
    sts = E.states(H0, W0, ptr, cols, vals, 1.0, K, *reg)
    ref = np.asarray(H0, np.float64)
    for k in range(1, K + 1):
        ref = HE.half_step(V, ref, W0, *reg)
        assert np.abs(sts[k] - ref).max() <= 1e-11


@pytest.mark.parametrize('omega', [0.0625, 0.3])
def test_between_the_end_points_it_is_the_iterated_wccd_sweep(omega):
    (ptr, cols, vals), W0, H0, _, _ = _problem('a', 5)
    ref = np.asarray(H0, np.float64)
    for _ in range(K):
        ref = WE.sweep(ref, W0, ptr, cols, vals, omega, *REG)
    assert (E.states(H0, W0, ptr, cols, vals, omega, K, *REG)[K] == ref).all()
    assert (ref[np.diff(ptr) == 0] == E.EPS).all()                      # rows without entries: swept to the floor


def test_run_takes_every_row_at_its_own_count():
    (ptr, cols, vals), W0, H0, _, _ = _problem('a', 3)
    sts = E.states(H0, W0, ptr, cols, vals, 0.05, 30)
    H, cnt = E.run(H0, W0, ptr, cols, vals, 0.05, 30, 1e-3)
    assert (cnt < 30).any() and (cnt >= 1).all()
    for i, c in enumerate(cnt):
        assert (H[i] == sts[int(c)][i]).all()
        a, b = sts[int(c) - 1][i].astype(np.float32), sts[int(c)][i].astype(np.float32)
        assert c == 30 or np.abs(b - a).max() <= np.float32(1e-3) * b.max()


# ---- the fp32 model of the kernel against the bound ---------------------------------------------------------------------------
@pytest.mark.parametrize('omega', OMEGAS)
@pytest.mark.parametrize('which,R,long_rows', [('a', 33, 16), ('b', 33, None), ('b', 100, None), ('b', 3, 16)])
def test_fp32_model_inside_the_bound(which, R, long_rows, omega):
    (ptr, cols, vals), W0, H0, _, _ = _problem(which, R)
    lr = E.default_long_rows(R) if long_rows is None else long_rows
    counts = np.diff(ptr)
    assert (counts > lr).any() and ((counts <= lr) & (counts > 0)).any()        # both paths
    G = None if omega == 0 else WE.gram_f32(W0)
    for reg in ((0.0, 0.0), REG):
        got = E.sweep_f32(H0, W0, ptr, cols, vals, omega, *reg, G=G, long_rows=lr)
        err, bound = E.sweep_check(got, H0, W0, G, ptr, cols, vals, omega, *reg, long_rows=lr)
        worst = E.fraction(err, bound).max()
        assert worst <= 1.0, (which, R, omega, reg, worst)
        # and the model is the float64 sweep up to rounding
        ref = E.sweep(H0, W0, ptr, cols, vals, omega, *reg, G=None if G is None else G.astype(np.float64))
        assert np.abs(got - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())


def test_the_thresholds_are_those_of_the_kernel():
    # csrc/nmfmu_fold_in_cd.hip: 2556 floats per wave (a workgroup has 40 KiB), three rank-padded vectors, (share + 3) + share * (R | 1) <= the rest
    assert E.PER_WAVE == 2556
    assert [E.avail(r) for r in (3, 64, 65, 256)] == [2364, 2364, 2172, 1788]
    assert [E.default_block(r) for r in (3, 33, 64, 100, 256)] == [590, 69, 35, 21, 6]
    assert [E.default_long_rows(r) for r in (3, 33, 64, 100, 256)] == [128, 69, 35, 21, 6]
    for r in (1, 3, 64, 255, 256):
        b = E.default_block(r)
        assert ((b + 3) & ~3) + b * (r | 1) <= E.avail(r)


@pytest.mark.parametrize('omega', [0.0, 0.3, 1.0])
def test_check_detects_a_wrong_coordinate(omega):
    """An output off by 64 ulp in one coordinate fails the check there (and, through the residual and q, may fail later ones
    of that row); the other rows still pass.  A row that must come back untouched and does not fails too.  (The problem of
    ``test_wccd_emulation``'s test of the same name: values a noisy product of the panel, so
    that the bound -- which grows with the residual -- is a few ulp of the result.)"""
    F, P, ptr, cols, vals = CE.sweep_case([40, 90], 120, 8, seed=2)                # (row 0 stores zeros only)
    G = None if omega == 0 else WE.gram_f32(P)
    for lr in (E.default_long_rows(8), 50):                             # 90 entries: one wave, four waves
        got = E.sweep_f32(F, P, ptr, cols, vals, omega, G=G, long_rows=lr)
        err, bound = E.sweep_check(got, F, P, G, ptr, cols, vals, omega, long_rows=lr)
        assert E.fraction(err, bound).max() <= 1.0
        for row in (1,):
            bad = got.copy()
            # the bound is a worst case that grows with the residual: the coordinate where it is tightest in ulps of the
            # result (the first: its residual carries the fewest roundings), where 64 ulp must lie outside it
            k = int(np.argmin(bound[row] / np.abs(got[row])))
            assert bound[row, k] < 60 * 2.0 ** -23 * abs(got[row, k])
            bad[row, k] *= np.float32(1 + 64 * 2.0 ** -23)
            frac = E.fraction(*E.sweep_check(bad, F, P, G, ptr, cols, vals, omega, long_rows=lr))
            assert frac[row, k] > 1.0, (omega, lr, row, frac[row, k])
            others = np.ones(len(got), dtype=bool)
            others[row] = False
            assert frac[others].max() <= 1.0
    if omega == 0:
        F, P, ptr, cols, vals = CE.sweep_case([40, 0, 90], 120, 8, seed=2)
        bad = E.sweep_f32(F, P, ptr, cols, vals, omega)
        assert (bad[1] == F[1]).all()
        bad[1, 0] = np.nextafter(bad[1, 0], np.float32(2))              # row 1 stores nothing
        frac = E.fraction(*E.sweep_check(bad, F, P, None, ptr, cols, vals, omega))
        assert np.isinf(frac[1, 0]) and frac[[0, 2]].max() <= 1.0


# ---- descent -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('omega', [0.0625, 0.3, 1.0])
@pytest.mark.parametrize('which,R', [('a', 5), ('a', 33), ('b', 8)])
def test_the_row_objective_does_not_rise(which, R, omega):
    (ptr, cols, vals), W0, H0, _, _ = _problem(which, R)
    for reg in ((0.0, 0.0), REG):
        sts = E.states(H0, W0, ptr, cols, vals, omega, 12, *reg)
        obj = np.stack([E.objectives(s, W0, ptr, cols, vals, omega, *reg) for s in sts])
        # (the eps in the denominator shortens a step by 1 - eps / den, the floor is a projection: still descent steps)
        assert (obj[1:] <= obj[:-1] + 1e-12 * np.maximum(obj[:-1], 1.0)).all(), (which, R, omega, reg)
        assert (obj[-1] < obj[0]).all()
