"""The numpy model of the top-k selection (tests/topk_emulation.py: tiles in column order, threshold test, sorted insertion
under the (score, column) order, exclusion cursor, nsplit partial lists and their merge) against a full stable sort --
exact agreement -- on the shape list of the GPU tests and on adversarial orders; and the checker of the GPU tests against
answers it must reject.  CPU only."""
import numpy as np
import pytest

import topk_emulation as E

TR, TC = 64, 128


def _scores(n, C, seed, ties=False):
    g = np.random.default_rng(seed)
    S = g.random((n, C), dtype=np.float32)
    if ties:
        S = np.round(S * 7).astype(np.float32)      # eight values: ties everywhere
    return S


def _pattern(n, C, seed):
    """Rows cycling through 0, 1, 4, 5, 8, 9, 20 stored columns; one row stores everything, one all but 2."""
    g = np.random.default_rng(seed)
    counts = [0, 1, 4, 5, 8, 9, 20]
    ex = [np.sort(g.choice(C, size=min(C, counts[r % 7]), replace=False)) for r in range(n)]
    if n > 2:
        ex[1] = np.arange(C)
        ex[2] = np.setdiff1d(np.arange(C), g.choice(C, size=min(2, C), replace=False))
    return ex


@pytest.mark.parametrize('C', [1, TC - 1, TC, TC + 1, 3 * TC + 17])
@pytest.mark.parametrize('k', [1, 5, 64, 65, 128])
def test_emulation_matches_sort(C, k):
    for ties in (False, True):
        S = _scores(5, C, 100 * C + k, ties)
        ref = E.sort_topk(S, k)
        for nsplit in (1, 2, 3, 5):
            got = E.emulate_topk(S, k, None, nsplit, TC)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (C, k, ties, nsplit)


@pytest.mark.parametrize('k', [1, 5, 65])
def test_emulation_with_exclusion(k):
    C = 3 * TC + 17
    S = _scores(9, C, k, ties=True)
    ex = _pattern(9, C, 3)
    ex[3] = np.arange(TC - 3, TC + 4)                       # a run across a tile edge (and a split edge for nsplit = 3)
    ex[4] = np.arange(2 * TC - 70, 2 * TC + 5)              # more than 64 stored columns inside one tile
    ref = E.sort_topk(S, k, ex)
    assert np.all(ref[1][1] == -1) and np.all(np.isneginf(ref[0][1]))
    assert np.sum(ref[1][2] >= 0) == min(k, 2)
    for nsplit in (1, 2, 3, 4):
        got = E.emulate_topk(S, k, ex, nsplit, TC)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (k, nsplit)
    empty = [np.zeros(0, dtype=np.int64)] * 9
    a, b = E.emulate_topk(S, k, empty, 2, TC), E.sort_topk(S, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('order', ['ascending', 'descending', 'equal', 'duplicated'])
def test_adversarial_orders(order):
    C, k = 3 * TC + 17, 5
    base = np.arange(C, dtype=np.float32)
    if order == 'ascending':         # every column is inserted
        S = base[None]
    elif order == 'descending':      # nothing enters after the first k
        S = -base[None]
    elif order == 'equal':
        S = np.full((1, C), 3.0, dtype=np.float32)
    else:                            # the same scores again in another tile and another split
        S = np.concatenate([base[:TC], base[:TC], base[:TC], base[:17]])[None]
    ref = E.sort_topk(S, k)
    if order == 'equal':
        assert list(ref[1][0]) == list(range(k))
    if order == 'duplicated':
        assert list(ref[1][0][:3]) == [TC - 1, 2 * TC - 1, 3 * TC - 1]
    for nsplit in (1, 2, 3, 4):
        got = E.emulate_topk(S, k, None, nsplit, TC)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (order, nsplit)


# ---- the checker ------------------------------------------------------------------------------------------------------------
def _checked_problem():
    g = np.random.default_rng(5)
    H, W = g.random((4, 7), dtype=np.float32), g.random((40, 7), dtype=np.float32)
    s64, bound = E.scores64(H, W), E.topk_bound(H, W)
    ex = [np.array([3, 9]), np.zeros(0, dtype=np.int64), np.arange(40), np.arange(38)]
    mask = E.excluded_mask(ex, 4, 40)
    vals, idx = E.sort_topk(s64.astype(np.float32), 5, ex)
    return s64, bound, mask, vals, idx


def test_checker_accepts_the_oracle():
    s64, bound, mask, vals, idx = _checked_problem()
    assert E.check_topk(vals, idx, s64, bound, 5, mask) <= 1.0
    assert np.all(idx[2] == -1) and list(idx[3][2:]) == [-1, -1, -1]


def test_checker_rejects_a_swapped_pair():
    s64, bound, mask, vals, idx = _checked_problem()
    vals[0, [1, 2]], idx[0, [1, 2]] = vals[0, [2, 1]], idx[0, [2, 1]]
    with pytest.raises(AssertionError, match='increase'):
        E.check_topk(vals, idx, s64, bound, 5, mask)


def test_checker_rejects_a_missing_best_column():
    s64, bound, mask, vals, idx = _checked_problem()
    full = E.sort_topk(s64.astype(np.float32), 6, [np.nonzero(m)[0] for m in mask])
    vals[0], idx[0] = full[0][0][1:], full[1][0][1:]          # ranks 2..6: the best column is gone
    with pytest.raises(AssertionError, match='left out'):
        E.check_topk(vals, idx, s64, bound, 5, mask)


def test_checker_rejects_an_excluded_column():
    s64, bound, mask, vals, idx = _checked_problem()
    free = E.sort_topk(s64.astype(np.float32), 5)
    mask[0, free[1][0][0]] = True                              # the best column of row 0 is now stored
    with pytest.raises(AssertionError, match='excluded'):
        E.check_topk(free[0], free[1], s64, bound, 5, mask)


def test_checker_rejects_a_short_row_and_a_wrong_value():
    s64, bound, mask, vals, idx = _checked_problem()
    v2, i2 = vals.copy(), idx.copy()
    v2[1, 4], i2[1, 4] = -np.inf, -1
    with pytest.raises(AssertionError):
        E.check_topk(v2, i2, s64, bound, 5, mask)
    v3 = vals.copy()
    v3[1, 0] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError, match='value off'):
        E.check_topk(v3, idx, s64, bound, 5, mask)
