"""The float64 reference of the fold-in kernel (tests/fold_in_emulation.py) against the reference's own runs (g22_fold_in:
tools/make_golden_fold_in.py; g20's frozen-W case) and against masked_emulation, on the CPU; and the checker the GPU tests
use, shown to reject what it must."""
import numpy as np
import pytest

import fold_in_emulation as F
import masked_emulation as M
from conftest import load_golden

G = load_golden('g22_fold_in')
G20 = load_golden('g20_masked_fit')
CASES = [str(c) for c in G['cases']]


def _g22():
    return G['indices'], G['values'], tuple(int(x) for x in G['shape']), G['W0'], G['H0']


def test_fixture_shape():
    idx, vals, shape, W0, H0 = _g22()
    assert shape == (37, 29) and W0.shape == (29, 5) and H0.shape == (37, 5) and int(G['iterations']) == 20
    assert len(CASES) == 18
    got = sorted((float(G[c + '_par'][3]), float(G[c + '_par'][0]), float(G[c + '_par'][1])) for c in CASES)
    want = sorted([(0.0, b, a) for b in (1.0, 2.0) for a in (0.0, 0.07)]
                  + [(1.0, b, a) for b in (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0) for a in (0.0, 0.07)])
    assert got == want
    # the problem is g20's: one fixture can stand in for the other
    for k in ('indices', 'values', 'W0', 'H0'):
        assert np.array_equal(G[k], G20[k])
    assert 11 not in idx[0] and float(vals.min()) >= 0.1


@pytest.mark.parametrize('case', CASES)
def test_emulation_matches_reference(case):
    beta, alpha, l1_ratio, missing = (float(x) for x in G[case + '_par'])
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    idx, vals, shape, W0, H0 = _g22()
    mode = 'missing' if missing else 'zero'
    H = F.states(idx, vals, shape, H0, W0, beta, mode, int(G['iterations']), l1, l2)[-1]
    ref = G[case + '_H']
    assert np.abs(H - ref).max() <= 1e-9 * np.abs(ref).max()         # two float64 implementations of the same 20 iterations
    if missing and alpha == 0:
        assert np.array_equal(H[11], H0[11].astype(np.float64))       # a row without entries keeps H0


def test_emulation_matches_g20_frozen_w():
    idx, vals, shape, W0, H0 = _g22()
    case = 'b1.5_frozenW'
    assert float(G20[case + '_par'][3]) == 0.0 and np.array_equal(G20[case + '_W'], W0.astype(np.float64))
    H = F.states(idx, vals, shape, H0, W0, 1.5, 'missing', int(G20['iterations']))[-1]
    ref = G20[case + '_H']
    assert np.abs(H - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 2, 3])
@pytest.mark.parametrize('reg', [False, True])
def test_missing_is_k_masked_steps(beta, reg):
    l1, l2 = (0.021, 0.049) if reg else (0.0, 0.0)
    idx, vals, W0, H0 = M.make_problem(37, 29, 33)
    k = 4
    H = H0.astype(np.float64)
    for _ in range(k):
        H = M.step(idx, vals, (37, 29), H, W0, beta, 'h', l1, l2)[0]
    got = F.states(idx, vals, (37, 29), H0, W0, beta, 'missing', k, l1, l2)[-1]
    assert np.abs(got - H).max() <= 1e-12 * np.abs(H).max()


@pytest.mark.parametrize('mode,beta', [('missing', 0.5), ('missing', 2), ('zero', 1), ('zero', 2)])
def test_bounds_are_small_and_positive(mode, beta):
    idx, vals, W0, H0 = F.make_wide(33)
    new, bound, t = F.iteration(idx, vals, (9, 700), H0, W0, beta, mode, 0.021, 0.049)
    assert np.all(bound > 0) and np.all(bound < 1e-3 * np.abs(new) + 1e-30)
    assert list(t['count']) == list(F.WIDE_COUNTS)
    assert np.all(t['num'][0] == 0) and np.all(t['num_bound'][0] == 0)              # the row without entries
    # a long row's four partials: three more additions than the same row on one wave
    short = F.iteration(idx, vals, (9, 700), H0, W0, beta, mode, long_rows=10 ** 6)[2]['num_bound']
    long_ = F.iteration(idx, vals, (9, 700), H0, W0, beta, mode)[2]['num_bound']
    assert F.default_block(33) == 64
    assert np.all(long_[4:] > short[4:]) and np.array_equal(long_[:4], short[:4])     # counts 65 .. 700 are long rows


def test_operation_counts():
    assert F.colsum_ops(29) == 13 and F.colsum_ops(700) == 13 and F.colsum_ops(16384) == 16 and F.colsum_ops(16385) == 18
    assert F.gram_ops(29) == 68 and F.gram_ops(700) == 70


# ---- the stop rule -------------------------------------------------------------------------------------------------------------
def test_stop_counts():
    h0 = np.asarray([[1.0, 2.0], [1.0, 2.0], [0.0, 0.0]], np.float32)
    h1 = np.asarray([[1.0, 2.001], [1.5, 2.0], [0.0, 0.0]], np.float32)
    h2 = np.asarray([[1.0, 2.5], [1.5001, 2.0], [0.0, 0.0]], np.float32)
    sts = [h0, h1, h2]
    assert list(F.stop_counts(sts, 1e-3)) == [1, 2, 1]      # row 0 stops at 1 although it moves again later; 0 <= tol * 0
    assert list(F.stop_counts(sts, 0.0)) == [2, 2, 2]       # tol = 0 disables the rule, even for a row that does not move
    assert list(F.stop_counts(sts, 1e-6)) == [2, 2, 1]
    # the comparison is the fp32 one: d = 2^-23 (one ulp of 1 .. 2), m = 1 + 2^-23
    a = np.asarray([[1.0]], np.float32)
    b = np.asarray([[np.float32(1.0) + np.float32(2.0 ** -23)]], np.float32)
    t = np.float32(2.0 ** -23)
    assert list(F.stop_counts([a, b, b], float(t))) == [1]
    assert list(F.stop_counts([a, b, b], float(t * np.float32(0.999)))) == [2]      # the third state does not move: d = 0


def test_run_takes_each_row_at_its_count():
    idx, vals, W0, H0 = M.make_problem(37, 29, 3)
    sts = F.states(idx, vals, (37, 29), H0, W0, 1, 'missing', 12)
    H, cnt = F.run(idx, vals, (37, 29), H0, W0, 1, 'missing', 12, tol=3e-2)
    assert cnt.min() < 12 and len(set(cnt.tolist())) > 1
    for i, c in enumerate(cnt):
        assert np.array_equal(H[i], sts[int(c)][i])


# ---- the checker rejects what it must -------------------------------------------------------------------------------------------
def _checked_problem():
    idx, vals, W0, H0 = M.make_problem(37, 29, 33)
    ref, bound, _ = F.iteration(idx, vals, (37, 29), H0, W0, 1, 'missing')
    fp32 = ref.astype(np.float32)                     # what a correct kernel could return: within half an ulp
    return idx, vals, W0, H0, ref, bound, fp32


def test_checker_accepts_the_rounded_reference():
    *_, ref, bound, fp32 = _checked_problem()
    cnt = np.ones(37, np.int32)
    worst, ok = F.check(fp32, ref, bound, cnt, cnt.copy())
    assert ok and worst < 1


def test_checker_rejects_a_wrong_element():
    *_, ref, bound, fp32 = _checked_problem()
    bad = fp32.copy()
    bad[20, 17] *= np.float32(1 + 1e-4)
    worst, ok = F.check(bad, ref, bound)
    assert not ok and worst > 1
    bad = fp32.copy()
    bad[5, 0] = np.nan
    assert not F.check(bad, ref, bound)[1]


def test_checker_rejects_a_row_with_the_other_rows_entries():
    idx, vals, W0, H0, ref, bound, _ = _checked_problem()
    cnt = np.bincount(idx[0], minlength=37)
    a, b = [int(i) for i in np.flatnonzero(cnt == 9)[:2]]             # two rows of equal count
    swapped = idx.copy()
    swapped[0][idx[0] == a], swapped[0][idx[0] == b] = b, a
    order = np.lexsort((swapped[1], swapped[0]))
    got = F.iteration(swapped[:, order], vals[order], (37, 29), H0, W0, 1, 'missing')[0].astype(np.float32)
    e = M.bound_err(got, ref, bound)
    assert not F.check(got, ref, bound)[1]
    assert e[a].max() > 1 and e[b].max() > 1 and np.delete(e, [a, b], 0).max() <= 1


def test_checker_rejects_a_count_off_by_one():
    *_, ref, bound, fp32 = _checked_problem()
    want = np.full(37, 7, np.int32)
    got = want.copy()
    got[36] += 1
    assert F.check(fp32, ref, bound, want.copy(), want)[1]
    assert not F.check(fp32, ref, bound, got, want)[1]
    got[36] -= 2
    assert not F.check(fp32, ref, bound, got, want)[1]
    assert not F.check(fp32, ref, bound, None, want)[1]
