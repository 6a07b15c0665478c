"""A numpy model of the top-k selection as csrc/nmfmu_score.hip performs it, the checker the GPU tests use, and the float64
error bounds of both scoring kernels.

The selection (``emulate_topk``) follows the kernels step by step: the columns are cut into ``nsplit`` ranges of whole tiles;
inside a range the tiles are scanned in column order; per row an exclusion cursor -- set by a binary search at the range's
first column, moving forward only -- overwrites the stored columns inside the tile with ``-inf``; the threshold test
``score > the list's k-th score`` picks the candidates and each is inserted into the sorted list under the total order
(score descending, equal scores by ascending column); the ranges' lists are then inserted in range order into an empty list
by the same routine.  The oracle it must agree with exactly is a full stable sort (``sort_topk``).

Bounds, derived from the kernel source, not from a run (u = 2^-24):

  top k   the MFMA is a k-ordered fmaf chain over the R rank columns (zero padding adds exact zeros): one rounding per
          step, so |got - s| <= gamma_R sum_r |h_ir w_jr| with gamma_R = R u / (1 - R u).
  pairs   a lane adds its RL products (RL roundings: RL - 1 additions after the first product, or RL fused steps), the xor
          butterfly adds 6 levels, and one more unit covers the products' own roundings when they are not fused:
          (RL + 7) u sum_r |h w|  (DESIGN.md section 19's count for the butterfly).
"""
import numpy as np

U = 2.0 ** -24
NINF = np.float32(-np.inf)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def rl_of(R):
    """Rank slots per lane of the sparse kernels: padded rank 32 / 64 -> 1, 128 -> 2, 256 -> 4."""
    return 1 if R <= 64 else 2 if R <= 128 else 4


def scores64(H, W):
    return np.asarray(H, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T


def topk_bound(H, W):
    R = np.shape(H)[1]
    gamma = R * U / (1.0 - R * U)
    return gamma * (np.abs(np.asarray(H, dtype=np.float64)) @ np.abs(np.asarray(W, dtype=np.float64)).T)


def pairs_ref_bound(H, W, rows, cols):
    """(float64 dot products, bounds) of the pairs."""
    h = np.asarray(H, dtype=np.float64)[rows]
    w = np.asarray(W, dtype=np.float64)[cols]
    R = np.shape(H)[1]
    return (h * w).sum(1), (rl_of(R) + 7) * U * np.abs(h * w).sum(1)


# ---- the selection as the kernels perform it ------------------------------------------------------------------------------------
def _before(s1, i1, s2, i2):
    return s1 > s2 or (s1 == s2 and i1 < i2)


def _insert(ls, li, cs, ci, k):
    """list_insert: the candidate enters when fewer than k entries come before it, behind the last of them; the rest moves
    down by one position and the last entry leaves.  (The kernel decides per position -- keep, take the candidate, take the
    entry one position up -- which is this insertion.)"""
    m = sum(1 for s, i in zip(ls, li) if _before(s, i, cs, ci))
    if m >= k:
        return
    ls.insert(m, cs)
    li.insert(m, ci)
    ls.pop()
    li.pop()


def emulate_topk(S, k, excluded=None, nsplit=1, tile_cols=128):
    """(values fp32 [n, k], indices int64 [n, k]) from the fp32 score matrix S [n, C].  ``excluded``: per row an ascending
    array of stored columns, or None."""
    S = np.asarray(S, dtype=np.float32)
    n, C = S.shape
    slots = 64 * ((k + 63) // 64)                      # the list holds whole lanes' worth of positions
    n_tiles = (C + tile_cols - 1) // tile_cols
    part = []
    for sp in range(nsplit):
        t0, t1 = sp * n_tiles // nsplit, (sp + 1) * n_tiles // nsplit
        c_end = min(C, t1 * tile_cols)
        rows_out = []
        for r in range(n):
            ls, li = [NINF] * slots, [-1] * slots
            ex = None if excluded is None else np.asarray(excluded[r])
            cur = 0 if ex is None else int(np.searchsorted(ex, t0 * tile_cols, side='left'))
            for t in range(t0, t1):
                c0 = t * tile_cols
                hi = min(c0 + tile_cols, c_end)
                tile = S[r, c0:hi].copy()
                if ex is not None:
                    while cur < len(ex) and ex[cur] < hi:
                        if ex[cur] >= c0:
                            tile[ex[cur] - c0] = NINF
                        cur += 1
                thr = ls[k - 1]
                for c in np.nonzero(tile > thr)[0]:      # ascending columns
                    _insert(ls, li, tile[c], c0 + int(c), k)
            rows_out.append((ls[:k], li[:k]))
        part.append(rows_out)
    vals = np.full((n, k), NINF, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int64)
    for r in range(n):
        if nsplit == 1:
            ls, li = part[0][r]
        else:
            ls, li = [NINF] * slots, [-1] * slots
            for sp in range(nsplit):
                for s, i in zip(*part[sp][r]):
                    if i >= 0:
                        _insert(ls, li, s, i, k)
        vals[r], idx[r] = ls[:k], li[:k]
    return vals, idx


def sort_topk(S, k, excluded=None):
    """The oracle: a full stable sort of the admissible columns by descending score (ties: ascending column)."""
    S = np.asarray(S, dtype=np.float32)
    n, C = S.shape
    vals = np.full((n, k), NINF, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int64)
    for r in range(n):
        adm = np.ones(C, dtype=bool)
        if excluded is not None:
            adm[np.asarray(excluded[r], dtype=np.int64)] = False
        cols = np.nonzero(adm & (S[r] > NINF))[0]
        order = cols[np.argsort(-S[r, cols].astype(np.float64), kind='stable')][:k]
        vals[r, :len(order)], idx[r, :len(order)] = S[r, order], order
    return vals, idx


def excluded_mask(excluded, n, C):
    mask = np.zeros((n, C), dtype=bool)
    if excluded is not None:
        for r in range(n):
            mask[r, np.asarray(excluded[r], dtype=np.int64)] = True
    return mask


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def check_topk(values, indices, s64, bound, k, excluded=None):
    """Asserts (a)-(d) of DESIGN.md section 21 for every row, no element left out; returns the worst |value - s64| / bound.
    s64 / bound: float64 [n, C] of the requested rows; excluded: bool [n, C] or None."""
    values, indices = np.asarray(values), np.asarray(indices)
    n, C = s64.shape
    assert values.shape == (n, k) and indices.shape == (n, k), (values.shape, indices.shape, (n, k))
    assert values.dtype == np.float32 and indices.dtype == np.int64, (values.dtype, indices.dtype)
    adm = np.ones((n, C), dtype=bool) if excluded is None else ~np.asarray(excluded, dtype=bool)
    worst = 0.0
    for i in range(n):
        val, idx = values[i], indices[i]
        cnt = min(k, int(adm[i].sum()))
        head = idx[:cnt]
        # (a)
        assert np.all((head >= 0) & (head < C)), ('index out of range', i, idx)
        assert len(np.unique(head)) == cnt, ('repeated column', i, idx)
        assert np.all(adm[i, head]), ('excluded column returned', i, idx)
        assert np.all(idx[cnt:] == -1) and np.all(np.isneginf(val[cnt:])), ('tail is not (-inf, -1)', i, idx, val)
        v = val[:cnt].astype(np.float64)
        assert np.all(np.isfinite(v)), ('non-finite value', i, val)
        # (b)
        err, b = np.abs(v - s64[i, head]), bound[i, head]
        assert np.all(err <= b), ('value off', i, float((err - b).max()))
        if cnt:
            worst = max(worst, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0))))
        # (c)
        assert np.all(v[:-1] >= v[1:]), ('values increase', i, val)
        eq = v[:-1] == v[1:]
        assert np.all(head[:-1][eq] < head[1:][eq]), ('equal values, indices not ascending', i, idx, val)
        # (d)
        if cnt == k:
            rest = adm[i].copy()
            rest[head] = False
            assert np.all(s64[i, rest] <= v[-1] + bound[i, rest]), ('a better column was left out', i)
    return worst
