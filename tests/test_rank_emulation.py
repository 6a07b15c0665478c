"""The model of full-ranking evaluation (tests/rank_emulation.py) against itself: the kernels' procedure equals the definition
exactly on the GPU tests' shapes, with ties and with the exclusion and held-out runs across tile and split edges; the metric
formulas equal a brute-force computation from the sorted lists; the GPU checkers reject what they must.  No GPU."""
import numpy as np
import pytest
import torch

import rank_emulation as E
import topk_emulation as T
from torchnmf_amd import scoring

TR, TC = E.TR, E.TC


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2], b[2])


def test_constants():
    assert (E.TR, E.TC, E.SCAN_ABOVE) == (scoring.TILE_ROWS, scoring.TILE_COLS, scoring.RANK_SCAN_ABOVE)
    assert E.SCAN_ABOVE in E.HELD and E.SCAN_ABOVE + 1 in E.HELD      # one value on each side of the threshold


@pytest.mark.parametrize('order', ['ascending', 'descending', 'equal', 'duplicated'])
def test_procedure_equals_definition_exact_scores(order):
    """Ties abound; every held-out count of HELD, every column count, every split and both forms."""
    for C in E.COLS:
        n = 2 * len(E.HELD) if C == E.C_ALL else len(E.HELD)
        _, _, S = E.exact_factors(order, C, n)
        ho = E.heldout_cycle(n, C, seed=1)
        ref = E.sort_ranks(S, ho)
        assert np.all(ref[0] >= 0) and np.all(ref[2] == C)
        for nsplit in (1, 2, 3):
            for form in (0, 1, 2):
                if form and nsplit == 2 and C != E.C_ALL:
                    continue
                assert _same(E.emulate_ranks(S, ho, None, nsplit, form), ref), (order, C, nsplit, form)
    if order == 'equal':      # all scores equal: the rank of column c is the number of columns below it
        assert np.array_equal(ref[0], np.concatenate(ho))


def test_procedure_equals_definition_with_exclusion():
    ex = E.exclusion_pattern()
    ho = E.heldout_for_pattern(ex)
    n = len(ex)
    g = np.random.default_rng(5)
    S_rand = g.random((n, E.C_ALL), dtype=np.float32)
    S_tie = np.floor(S_rand * 4).astype(np.float32)
    for S in (S_rand, S_tie, E.exact_factors('duplicated', E.C_ALL, n)[2]):
        ref = E.sort_ranks(S, ho, ex)
        mask = E.excluded_mask(ex, n, E.C_ALL)
        flat_r = np.concatenate([np.full(len(h), r) for r, h in enumerate(ho)])
        flat_c = np.concatenate(ho)
        assert np.array_equal(ref[0] == -1, mask[flat_r, flat_c])      # -1 exactly on the pairs that are excluded
        assert np.all(ref[0][flat_r == 5] == -1) and ref[2][5] == 0 and ref[2][6] == 2
        assert sorted(ref[0][flat_r == 6]) == [-1, 0, 1]
        for nsplit in (1, 2, 3, 4, 5):      # 5: a range without a tile
            for form in (0, 1, 2):
                assert _same(E.emulate_ranks(S, ho, ex, nsplit, form), ref), (nsplit, form)
    # the empty pattern excludes nothing
    empty = [np.zeros(0, dtype=np.int64)] * n
    assert _same(E.emulate_ranks(S_tie, ho, empty, 3), E.sort_ranks(S_tie, ho, None))


def test_rank_is_a_function_of_its_row_and_pair():
    """Other rows, other held-out pairs and the split do not enter a pair's rank."""
    g = np.random.default_rng(6)
    S = np.floor(g.random((5, 300)) * 8).astype(np.float32)
    ho = E.heldout_cycle(5, 300, seed=2, shift=3)
    ex = [np.sort(g.choice(300, size=9, replace=False)) for _ in range(5)]
    full = E.sort_ranks(S, ho, ex)
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in ho])])
    for r in range(5):
        alone = E.emulate_ranks(S[r:r + 1], ho[r:r + 1], ex[r:r + 1], 2)
        assert np.array_equal(alone[0], full[0][ptr[r]:ptr[r + 1]])
        if len(ho[r]) > 1:
            one = E.emulate_ranks(S[r:r + 1], [ho[r][:1]], ex[r:r + 1], 3)
            assert one[0][0] == full[0][ptr[r]]


def test_rank_agrees_with_topk():
    """rank < k exactly when the column is among the k best, and then it is the position."""
    g = np.random.default_rng(7)
    S = np.floor(g.random((6, 300)) * 16).astype(np.float32)
    ho = E.heldout_cycle(6, 300, seed=3, shift=5)
    ex = [np.sort(g.choice(300, size=11, replace=False)) for _ in range(6)]
    ranks, scores, _ = E.emulate_ranks(S, ho, ex, 2)
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(ho)])
    cols = np.concatenate(ho)
    for k in (1, 5, 64, 128):
        vals, idx = T.sort_topk(S, k, ex)
        for e in range(len(rows)):
            inside = cols[e] in idx[rows[e]]
            assert inside == (0 <= ranks[e] < k)
            if inside:
                assert idx[rows[e], ranks[e]] == cols[e] and vals[rows[e], ranks[e]] == scores[e]


# ---- the metrics ----------------------------------------------------------------------------------------------------------------
def test_metric_formulas_against_brute_force():
    ex = E.exclusion_pattern()
    ho = E.heldout_for_pattern(ex)
    n = len(ex)
    S = np.floor(np.random.default_rng(8).random((n, E.C_ALL)) * 50).astype(np.float32)
    ranks, _, adm = E.sort_ranks(S, ho, ex)
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(ho)])
    ks = (1, 10, 200, 1000)
    brute = E.metrics_brute(E.sorted_lists(S, ex), ho, ks)
    model = E.metrics_from_ranks(rows, ranks, adm, ks)
    r = scoring.Ranks(torch.from_numpy(rows), torch.from_numpy(np.concatenate(ho)), torch.from_numpy(ranks),
                      torch.zeros(len(rows)), torch.from_numpy(adm))
    got = scoring.metrics_from_ranks(r, ks)
    assert set(brute) == set(model) == set(got) and len(got) == 3 * len(ks) + 3
    with_valid = sum(1 for h, e in zip(ho, ex) if len(np.setdiff1d(h, e)))      # row 5 holds only excluded pairs
    assert brute['rows'] == with_valid < n - 1 and len(ho[5]) > 0
    for key in brute:
        assert got[key].dtype == torch.float64 and got[key].dim() == 0
        assert abs(model[key] - brute[key]) <= 1e-12, (key, model[key], brute[key])
        assert abs(float(got[key]) - brute[key]) <= 1e-12, (key, float(got[key]), brute[key])
    assert 0 < brute['auc'] < 1 and brute['recall@1000'] == 1.0


def test_metrics_without_rows():
    r = scoring.Ranks(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                      torch.zeros(0), torch.full((4,), 9))
    got = scoring.metrics_from_ranks(r, (3,))
    assert float(got['rows']) == 0 and all(torch.isnan(v) for k, v in got.items() if k != 'rows')


# ---- the checkers reject what they must -------------------------------------------------------------------------------------------
def _exact_case():
    ex = E.exclusion_pattern()
    ho = E.heldout_for_pattern(ex)
    S = E.exact_factors('duplicated', E.C_ALL, len(ex))[2]
    return S, ho, ex, E.sort_ranks(S, ho, ex)


def test_checker_accepts_the_definition():
    S, ho, ex, (ranks, scores, adm) = _exact_case()
    E.check_exact(ranks, scores, adm, S, ho, ex)


@pytest.mark.parametrize('what', ['off by one', 'counts an excluded column', 'counts the pair itself', 'missing -1',
                                  'one ulp', 'admissible'])
def test_exact_checker_rejects(what):
    S, ho, ex, (ranks, scores, adm) = _exact_case()
    ranks, scores, adm = ranks.copy(), scores.copy(), adm.copy()
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(ho)])
    cols = np.concatenate(ho)
    if what == 'off by one':
        ranks[np.nonzero(ranks > 0)[0][3]] -= 1
    elif what == 'counts an excluded column':
        # row 4 stores a run of 75 columns; recount one of its pairs with the run admissible
        e = int(np.nonzero((rows == 4) & (ranks >= 0))[0][0])
        wrong = E.sort_ranks(S[4:5], [cols[e:e + 1]], None)[0][0]
        assert wrong != ranks[e]
        ranks[e] = wrong
    elif what == 'counts the pair itself':
        ranks[np.nonzero(ranks >= 0)[0][0]] += 1
    elif what == 'missing -1':
        e = int(np.nonzero(ranks == -1)[0][0])
        ranks[e] = E.sort_ranks(S[rows[e]:rows[e] + 1], [cols[e:e + 1]], None)[0][0]
    elif what == 'one ulp':
        scores[5] = np.nextafter(scores[5], np.float32(np.inf))
    else:
        adm[4] += 1
    with pytest.raises(AssertionError):
        E.check_exact(ranks, scores, adm, S, ho, ex)


@pytest.mark.parametrize('what', [None, 'rank far off', 'counts an excluded column', 'missing -1', 'score off'])
def test_bounds_checker(what):
    g = np.random.default_rng(9)
    n, C, R = 7, 200, 33
    H = g.random((n, R), dtype=np.float32)
    W = g.random((C, R), dtype=np.float32)
    s64, bound = T.scores64(H, W), T.topk_bound(H, W)
    ex = [np.sort(g.choice(C, size=40, replace=False)) for _ in range(n)]
    ho = [np.sort(g.choice(C, size=12, replace=False)) for _ in range(n)]
    ho[2] = np.union1d(ho[2], ex[2][:2])
    S = s64.astype(np.float32)      # within the bound of s64: half an ulp
    ranks, scores, _ = E.sort_ranks(S, ho, ex)
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(ho)])
    cols = np.concatenate(ho)
    mask = E.excluded_mask(ex, n, C)
    if what is None:
        assert 0 < E.check_bounds(rows, cols, ranks, scores, s64, bound, mask) <= 1
        return
    e = int(np.nonzero(ranks > 20)[0][0])
    if what == 'rank far off':
        ranks[e] -= 3
    elif what == 'counts an excluded column':
        ranks[e] = E.sort_ranks(S[rows[e]:rows[e] + 1], [cols[e:e + 1]], None)[0][0]
        assert ranks[e] > E.sort_ranks(S, ho, ex)[0][e] + 2
    elif what == 'missing -1':
        ranks[int(np.nonzero(ranks == -1)[0][0])] = 4
    else:
        scores[e] *= np.float32(1.001)
    with pytest.raises(AssertionError):
        E.check_bounds(rows, cols, ranks, scores, s64, bound, mask)
