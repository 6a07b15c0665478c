"""A numpy model of full-ranking evaluation: the definition, the procedure of csrc/nmfmu_rank.hip, the checkers the GPU tests
use, and the metric formulas.

The definition (``sort_ranks``): per row a stable sort of the admissible columns under (score descending, column ascending);
the rank of a held-out pair is its column's position in that list, -1 when the exclusion pattern stores the pair itself.

The procedure (``emulate_ranks``) follows the kernels step by step.  The columns are cut into ``nsplit`` ranges of whole
tiles.  Extract pass: per (row, range) a forward-only cursor over the row's held-out columns, set by a binary search at the
range's first column, copies ``tile[c]`` of every pair inside the tile out of the UNMASKED tile, and a binary search in the
row's stored columns sets the pair's flag.  Count pass: the exclusion cursor (same search, forward only) overwrites the stored
columns inside the tile with ``-inf``; the row's thresholds are taken in chunks of 64; per chunk either form counts the
tile's scores that come before each threshold -- ``ballot``: per threshold, over the two 64-column halves of the tile with
``-inf`` past the range's end, as ``(x > s) | ((x >= s) & lanes whose column is below c)``; ``scan``: per threshold, over the columns of the tile inside the range -- and the count is
added to the (range, pair) word.  Merge: the ranges' words are added, flagged pairs become -1, ``admissible = C - stored``.

Bounds for random factors are ``topk_emulation.topk_bound``'s: the score tile is the same k-ordered fmaf chain.
"""
import numpy as np

NINF = np.float32(-np.inf)
SCAN_ABOVE = 24          # scoring.RANK_SCAN_ABOVE


def _before(s1, i1, s2, i2):
    return s1 > s2 or (s1 == s2 and i1 < i2)


# ---- the definition -------------------------------------------------------------------------------------------------------------
def sort_ranks(S, heldout, excluded=None):
    """(ranks int64 [n], scores fp32 [n], admissible int64 [n_rows]) of the pairs in row-major order, from the fp32 score
    matrix S [n_rows, C].  ``heldout`` / ``excluded``: per row an ascending array of columns (``excluded`` may be None)."""
    S = np.asarray(S, dtype=np.float32)
    n_rows, C = S.shape
    ranks, scores, adm_n = [], [], np.zeros(n_rows, dtype=np.int64)
    for r in range(n_rows):
        adm = np.ones(C, dtype=bool)
        if excluded is not None:
            adm[np.asarray(excluded[r], dtype=np.int64)] = False
        adm_n[r] = adm.sum()
        cols = np.nonzero(adm)[0]
        order = cols[np.argsort(-S[r, cols].astype(np.float64), kind='stable')]
        pos = np.full(C, -1, dtype=np.int64)
        pos[order] = np.arange(len(order))
        for c in np.asarray(heldout[r], dtype=np.int64):
            ranks.append(pos[c])
            scores.append(S[r, c])
    return np.asarray(ranks, dtype=np.int64), np.asarray(scores, dtype=np.float32), adm_n


def sorted_lists(S, excluded=None):
    """Per row the admissible columns in ranking order (the lists the metrics are defined on)."""
    S = np.asarray(S, dtype=np.float32)
    out = []
    for r in range(S.shape[0]):
        adm = np.ones(S.shape[1], dtype=bool)
        if excluded is not None:
            adm[np.asarray(excluded[r], dtype=np.int64)] = False
        cols = np.nonzero(adm)[0]
        out.append(cols[np.argsort(-S[r, cols].astype(np.float64), kind='stable')])
    return out


# ---- the procedure of the kernels -----------------------------------------------------------------------------------------------
def emulate_ranks(S, heldout, excluded=None, nsplit=1, form=0, tile_cols=128, scan_above=SCAN_ABOVE):
    """As ``sort_ranks``, by the kernels' procedure.  form 0: per row by its number of pairs; 1: ballot; 2: scan."""
    S = np.asarray(S, dtype=np.float32)
    n_rows, C = S.shape
    n_tiles = (C + tile_cols - 1) // tile_cols
    half = tile_cols // 2
    ho = [np.asarray(h, dtype=np.int64) for h in heldout]
    ex = [np.zeros(0, dtype=np.int64) if excluded is None else np.asarray(excluded[r], dtype=np.int64) for r in range(n_rows)]
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in ho])]).astype(np.int64)
    n = int(ptr[-1])
    score = np.full(n, np.nan, dtype=np.float32)
    flag = np.full(n, -7, dtype=np.int64)
    ws = np.full((nsplit, n), -7, dtype=np.int64)
    splits = [(sp * n_tiles // nsplit, (sp + 1) * n_tiles // nsplit) for sp in range(nsplit)]

    # extract pass: nothing is masked
    for t0, t1 in splits:
        c_end = min(C, t1 * tile_cols)
        for r in range(n_rows):
            cur = int(np.searchsorted(ho[r], t0 * tile_cols, side='left'))
            for t in range(t0, t1):
                c0 = t * tile_cols
                hi = min(c0 + tile_cols, c_end)
                tile = S[r, c0:hi]
                while cur < len(ho[r]) and ho[r][cur] < hi:
                    c = ho[r][cur]
                    assert c >= c0
                    score[ptr[r] + cur] = tile[c - c0]
                    lo = int(np.searchsorted(ex[r], c, side='left'))
                    flag[ptr[r] + cur] = -1 if lo < len(ex[r]) and ex[r][lo] == c else 0
                    cur += 1

    # count pass
    for sp, (t0, t1) in enumerate(splits):
        c_end = min(C, t1 * tile_cols)
        for r in range(n_rows):
            nt = len(ho[r])
            cnt = np.zeros(nt, dtype=np.int64)
            scan = form == 2 or (form == 0 and nt > scan_above)
            cur = int(np.searchsorted(ex[r], t0 * tile_cols, side='left'))
            for t in range(t0, t1):
                c0 = t * tile_cols
                hi = min(c0 + tile_cols, c_end)
                tile = np.full(tile_cols, NINF, dtype=np.float32)      # -inf past the range's end
                tile[:hi - c0] = S[r, c0:hi]
                while cur < len(ex[r]) and ex[r][cur] < hi:
                    if ex[r][cur] >= c0:
                        tile[ex[r][cur] - c0] = NINF
                    cur += 1
                for base in range(0, nt, 64):
                    for u in range(base, min(base + 64, nt)):
                        se, ce = score[ptr[r] + u], int(ho[r][u])
                        if scan:
                            cnt[u] += sum(1 for c in range(hi - c0) if _before(tile[c], c0 + c, se, ce))
                        else:
                            # per half: ballot(x > se) | (ballot(x >= se) & the lanes whose column is below ce)
                            for h0 in (0, half):
                                x = tile[h0:h0 + half]
                                below = np.arange(half) < ce - c0 - h0
                                cnt[u] += int(np.sum((x > se) | ((x >= se) & below)))
            ws[sp, ptr[r]:ptr[r + 1]] = cnt

    # merge
    assert np.all(flag != -7) and np.all(ws != -7), 'a pair or a (range, pair) word was never written'
    ranks = np.where(flag == -1, -1, ws.sum(0))
    adm = np.array([C - len(ex[r]) for r in range(n_rows)], dtype=np.int64)
    return ranks.astype(np.int64), score, adm


# ---- the checkers ---------------------------------------------------------------------------------------------------------------
def check_exact(ranks, scores, admissible, S, heldout, excluded=None):
    """The device's answer against the definition on a score matrix that is EXACT in fp32: every pair, exactly."""
    ranks, scores, admissible = np.asarray(ranks), np.asarray(scores), np.asarray(admissible)
    ref_r, ref_s, ref_a = sort_ranks(S, heldout, excluded)
    assert ranks.dtype == np.int64 and scores.dtype == np.float32 and admissible.dtype == np.int64
    assert ranks.shape == ref_r.shape and scores.shape == ref_s.shape and admissible.shape == ref_a.shape
    assert np.array_equal(admissible, ref_a), ('admissible', admissible, ref_a)
    bad = np.nonzero(ranks != ref_r)[0]
    assert len(bad) == 0, ('rank', bad[:8], ranks[bad[:8]], ref_r[bad[:8]])
    assert np.array_equal(scores.view(np.int32), ref_s.view(np.int32)), 'score bits'


def check_bounds(rows, cols, ranks, scores, s64, bound, excluded_mask=None):
    """Random factors, every pair: lo_e <= rank_e <= hi_e and |score_e - s64| <= bound, with
    lo_e = #{admissible j: s64_j - b_j > s64_c + b_c}, hi_e = #{admissible j != c: s64_j + b_j >= s64_c - b_c}; a pair on an
    excluded column must carry -1 and no other pair may.  Returns the worst |score - s64| / bound."""
    rows, cols, ranks, scores = map(np.asarray, (rows, cols, ranks, scores))
    n_rows, C = s64.shape
    adm = np.ones((n_rows, C), dtype=bool) if excluded_mask is None else ~np.asarray(excluded_mask, dtype=bool)
    worst = 0.0
    for e in range(len(rows)):
        i, c = int(rows[e]), int(cols[e])
        err, b = abs(float(scores[e]) - s64[i, c]), bound[i, c]
        assert err <= b, ('score off', e, i, c, err, b)
        if b > 0:
            worst = max(worst, err / b)
        if not adm[i, c]:
            assert ranks[e] == -1, ('-1 missing', e, i, c, ranks[e])
            continue
        a = adm[i].copy()
        lo = int(np.sum(a & (s64[i] - bound[i] > s64[i, c] + b)))
        a[c] = False
        hi = int(np.sum(a & (s64[i] + bound[i] >= s64[i, c] - b)))
        assert lo <= ranks[e] <= hi, ('rank outside its bounds', e, i, c, int(ranks[e]), lo, hi)
    return worst


# ---- the metrics ----------------------------------------------------------------------------------------------------------------
def metrics_from_ranks(rows, ranks, admissible, ks):
    """The formulas of scoring.ranking_metrics in float64 numpy, from ranks."""
    rows, ranks, admissible = np.asarray(rows), np.asarray(ranks), np.asarray(admissible)
    per = {f'{m}@{k}': [] for k in ks for m in ('recall', 'precision', 'ndcg')}
    per.update(mrr=[], auc=[])
    n_eval = 0
    for i in np.unique(rows):
        r = np.sort(ranks[(rows == i) & (ranks >= 0)]).astype(np.float64)
        t = len(r)
        if t == 0:
            continue
        n_eval += 1
        for k in ks:
            hit = r[r < k]
            per[f'recall@{k}'].append(len(hit) / t)
            per[f'precision@{k}'].append(len(hit) / k)
            per[f'ndcg@{k}'].append(np.sum(1.0 / np.log2(hit + 2.0)) / np.sum(1.0 / np.log2(np.arange(min(k, t)) + 2.0)))
        per['mrr'].append(1.0 / (1.0 + r[0]))
        neg = int(admissible[i]) - t
        if neg > 0:
            per['auc'].append(1.0 - (r.sum() - t * (t - 1) / 2.0) / (t * neg))
    out = {key: (float(np.mean(v)) if v else float('nan')) for key, v in per.items()}
    out['rows'] = float(n_eval)
    return out


def metrics_brute(lists, heldout, ks):
    """The same metrics from the sorted lists, by their textbook definitions: hits among the first k of the list, DCG over
    the list's positions, the reciprocal position of the first relevant column, and the AUC as the fraction of (relevant,
    irrelevant) pairs of admissible columns that the list orders correctly."""
    per = {f'{m}@{k}': [] for k in ks for m in ('recall', 'precision', 'ndcg')}
    per.update(mrr=[], auc=[])
    n_eval = 0
    for order, h in zip(lists, heldout):
        rel = np.isin(order, np.asarray(h, dtype=np.int64))      # held-out columns that are excluded are not in the list
        t = int(rel.sum())
        if t == 0:
            continue
        n_eval += 1
        for k in ks:
            top = rel[:k]
            per[f'recall@{k}'].append(top.sum() / t)
            per[f'precision@{k}'].append(top.sum() / k)
            dcg = sum(1.0 / np.log2(p + 2.0) for p in range(len(top)) if top[p])
            per[f'ndcg@{k}'].append(dcg / sum(1.0 / np.log2(p + 2.0) for p in range(min(k, t))))
        per['mrr'].append(1.0 / (1.0 + int(np.nonzero(rel)[0][0])))
        neg = len(order) - t
        if neg > 0:
            good = sum(int(np.sum(~rel[p + 1:])) for p in np.nonzero(rel)[0])      # irrelevant columns behind each relevant one
            per['auc'].append(good / (t * neg))
    out = {key: (float(np.mean(v)) if v else float('nan')) for key, v in per.items()}
    out['rows'] = float(n_eval)
    return out


# ---- the problems both test files use ---------------------------------------------------------------------------------------------
TR, TC = 64, 128                         # scoring.TILE_ROWS / TILE_COLS
N_ALL, C_ALL = 2 * TR + 3, 3 * TC + 17
N_ROWS = [1, TR - 1, TR + 1, N_ALL]
COLS = [1, TC - 1, TC, TC + 1, C_ALL]
RANKS = [1, 3, 33, 100, 256]
HELD = [0, 1, 2, SCAN_ABOVE, SCAN_ABOVE + 1, 63, 64, 65, 130, -1]      # pairs per row, cycling; -1: every column


def heldout_cycle(n_rows, C, seed=0, shift=0):
    """Per row an ascending array of held-out columns, the counts cycling through HELD (capped at C)."""
    g = np.random.default_rng(1000 * seed + C)
    out = []
    for r in range(n_rows):
        k = HELD[(r + shift) % len(HELD)]
        k = C if k < 0 else min(k, C)
        out.append(np.sort(g.choice(C, size=k, replace=False)).astype(np.int64))
    return out


def exact_factors(order, C=C_ALL, n=N_ALL):
    """Integer-valued rank-3 factors: every score is exact in fp32 whatever the summation order, and ties abound."""
    col = np.arange(C, dtype=np.float32)
    if order == 'ascending':
        w0 = col
    elif order == 'descending':
        w0 = C - col
    elif order == 'equal':
        w0 = np.full(C, 3, dtype=np.float32)
    else:                               # 'duplicated': equal rows of W in different tiles and splits
        w0 = col % TC
    W = np.stack([w0, np.ones(C, dtype=np.float32), 2 * np.ones(C, dtype=np.float32)], 1)
    H = np.stack([np.arange(1, n + 1) % 7, np.ones(n), np.arange(n) % 5], 1).astype(np.float32)
    S = (H.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    assert np.array_equal(S.astype(np.float64), H.astype(np.float64) @ W.astype(np.float64).T)
    return H, W, S


def exclusion_pattern():
    """The 37 x C_ALL pattern of the top-k tests: rows cycle through 0, 1, 4, 5, 8, 9, 20 stored columns; row 3 stores a run
    across the first tile edge, row 4 a run of 75 across the second tile edge (a split edge for nsplit = 3 and 2), row 5 every
    column, row 6 all but 2."""
    g = np.random.default_rng(37)
    counts = [0, 1, 4, 5, 8, 9, 20]
    ex = [np.sort(g.choice(C_ALL, size=counts[r % 7], replace=False)) for r in range(37)]
    ex[3] = np.arange(TC - 3, TC + 4)
    ex[4] = np.arange(2 * TC - 70, 2 * TC + 5)
    ex[5] = np.arange(C_ALL)
    ex[6] = np.setdiff1d(np.arange(C_ALL), [TC - 1, 2 * TC])
    return [np.asarray(e, dtype=np.int64) for e in ex]


def heldout_for_pattern(ex):
    """Held-out columns for ``exclusion_pattern``: the first and last column of every tile and split, the neighbours of the
    excluded runs, pairs that are excluded themselves, and random ones."""
    g = np.random.default_rng(38)
    edges = np.array([0, TC - 1, TC, 2 * TC - 1, 2 * TC, 3 * TC - 1, 3 * TC, C_ALL - 1])
    ho = []
    for r, e in enumerate(ex):
        h = g.choice(C_ALL, size=[6, 0, 30, 70][r % 4], replace=False)
        if r % 3 == 0:
            h = np.concatenate([h, edges])
        if len(e) and r % 2 == 0:
            h = np.concatenate([h, e[:1], e[-1:]])                 # excluded themselves: rank -1
        ho.append(h)
    ho[3] = np.array([TC - 4, TC - 3, TC + 3, TC + 4])             # next to the run, and its two ends
    ho[4] = np.array([2 * TC - 71, 2 * TC - 1, 2 * TC, 2 * TC + 5, 0, C_ALL - 1])
    ho[5] = np.array([0, 5, TC, C_ALL - 1])                        # everything is excluded
    ho[6] = np.array([TC - 1, TC, 2 * TC])                         # the two admissible columns and an excluded one
    return [np.unique(h).astype(np.int64) for h in ho]


def excluded_mask(excluded, n, C):
    mask = np.zeros((n, C), dtype=bool)
    if excluded is not None:
        for r in range(n):
            mask[r, np.asarray(excluded[r], dtype=np.int64)] = True
    return mask
