"""Full-ranking evaluation on the device (csrc/nmfmu_rank.hip, scoring.rank_scores / ranking_metrics, NMF / PLCA methods)
against the numpy definition, against ``topk_scores`` and against float64, under the checkers of tests/rank_emulation.py --
every pair, nothing left out.

Shapes (rank_emulation.N_ROWS / COLS / RANKS / HELD): 1, 63, 65, 131 requested rows (rows with a held-out pair; rows without
one lie between them); 1, 127, 128, 129, 401 columns; ranks 1, 3, 33, 100, 256; 0, 1, 2, 24, 25 (the two sides of
scoring.RANK_SCAN_ABOVE), 63, 64, 65, 130 and every column held out per row.  Every answer is computed with the chosen split,
with forced splits 1 / 2 / 3, with both forms of the count forced and twice, outputs and workspace pre-filled with NaN /
garbage, and all of them must be bitwise equal.

Measured on an MI355X (worst |score - float64| / bound): DESIGN.md section 29.
"""
import functools

import numpy as np
import pytest
import torch

import rank_emulation as E
import topk_emulation as T
from conftest import record

pytestmark = pytest.mark.gpu

from torchnmf_amd import scoring  # noqa: E402

TR, TC = scoring.TILE_ROWS, scoring.TILE_COLS
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _coo(lists, n, C, dev, zeros=False):
    ri = np.concatenate([np.full(len(e), r) for r, e in enumerate(lists)]).astype(np.int64)
    ci = np.concatenate(lists).astype(np.int64)
    v = np.ones(len(ri), dtype=np.float32)
    if zeros:
        v[::2] = 0          # a stored zero counts
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([ri, ci])), torch.from_numpy(v), (n, C)).to(dev).coalesce()


def _flat(lists):
    return (np.concatenate([np.full(len(h), r) for r, h in enumerate(lists)]).astype(np.int64),
            np.concatenate(lists).astype(np.int64))


def _np(r):
    return tuple(x.cpu().numpy() for x in r)


def _same(a, b):
    return (torch.equal(a.ranks, b.ranks) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
            and torch.equal(a.admissible, b.admissible) and torch.equal(a.rows, b.rows) and torch.equal(a.cols, b.cols))


def _run_variants(Hd, Wd, heldout, exclude, tag):
    """The chosen split, forced splits 1 / 2 / 3, both forms of the count, and a second call: all bitwise equal, outputs and
    workspace pre-filled.  Returns (rows, cols, ranks, scores, admissible) as numpy."""
    first = scoring.rank_scores(Hd, Wd, heldout, exclude, _fill=NAN)
    assert first.ranks.dtype == torch.int64 and first.scores.dtype == torch.float32 and first.admissible.dtype == torch.int64
    assert first.rows.dtype == torch.int64 and first.cols.dtype == torch.int64 and not first.scores.requires_grad
    for ns in (1, 2, 3):
        assert _same(first, scoring.rank_scores(Hd, Wd, heldout, exclude, _nsplit=ns, _fill=NAN)), ('nsplit', ns, tag)
    for form in (1, 2):
        assert _same(first, scoring.rank_scores(Hd, Wd, heldout, exclude, _nsplit=2, _fill=NAN, _form=form)), ('form', form, tag)
    assert _same(first, scoring.rank_scores(Hd, Wd, heldout, exclude, _fill=NAN)), ('second call', tag)
    return _np(first)


def _heldout_requesting(n_req, C, seed):
    """Held-out lists (counts cycling through E.HELD, rows without a pair among them) with exactly n_req non-empty rows."""
    n = n_req
    while True:
        ho = E.heldout_cycle(n, C, seed)
        if sum(1 for h in ho if len(h)) == n_req and len(ho[-1]):
            return ho
        n += 1


# ---- exact scores: the definition, every pair -----------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['ascending', 'descending', 'equal', 'duplicated'])
def test_rank_exact(dev, order):
    """Integer-valued factors: every score is exact in fp32 whatever the summation order and ties abound, so ranks, scores
    and admissible counts must equal the stable sort exactly."""
    for C in E.COLS:
        for n_req in E.N_ROWS:
            ho = _heldout_requesting(n_req, C, seed=n_req)
            n = len(ho)
            H, W, S = E.exact_factors(order, C, n)
            Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
            rows, cols, ranks, scores, adm = _run_variants(Hd, Wd, _coo(ho, n, C, dev), None, (order, C, n_req))
            fr, fc = _flat(ho)
            assert np.array_equal(rows, fr) and np.array_equal(cols, fc)
            E.check_exact(ranks, scores, adm, S, ho)
    # with the exclusion pattern
    ex = E.exclusion_pattern()
    ho = E.heldout_for_pattern(ex)
    H, W, S = E.exact_factors(order, E.C_ALL, len(ex))
    Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    _, _, ranks, scores, adm = _run_variants(Hd, Wd, _coo(ho, len(ex), E.C_ALL, dev), _coo(ex, len(ex), E.C_ALL, dev, zeros=True),
                                             (order, 'pattern'))
    E.check_exact(ranks, scores, adm, S, ho, ex)


# ---- random factors: against topk and against float64 ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(R):
    g = np.random.default_rng(2000 + R)
    H = g.random((E.N_ALL, R), dtype=np.float32) + np.float32(0.01)
    W = g.random((E.C_ALL, R), dtype=np.float32) + np.float32(0.01)
    return H, W, T.scores64(H, W), T.topk_bound(H, W)


def _check_against_topk(Hd, Wd, exclude, rows, cols, ranks, scores):
    for k in (1, 5, 64, 128):
        top = scoring.topk_scores(Hd, Wd, k, exclude=exclude)
        idx, val = top.indices.cpu().numpy(), top.values.cpu().numpy()
        inside = (idx[rows] == cols[:, None]).any(1)
        assert np.array_equal(inside, (ranks >= 0) & (ranks < k)), ('rank < k <=> among the k best', k)
        if k == 128:
            e = np.nonzero(inside)[0]
            assert np.array_equal(idx[rows[e], ranks[e]], cols[e])
            assert np.array_equal(val[rows[e], ranks[e]].view(np.int32), scores[e].view(np.int32)), 'score bits differ from topk'


@pytest.mark.parametrize('R', E.RANKS)
def test_rank_against_topk_and_float64(dev, R):
    H, W, s64, bound = _problem(R)
    worst = 0.0
    for C in E.COLS:
        n = E.N_ALL if C == E.C_ALL else TR + 1
        g = np.random.default_rng(R + C)
        ho = E.heldout_cycle(n, C, seed=R)
        ex = [np.sort(g.choice(C, size=min(C, int(g.integers(0, 12))), replace=False)) for _ in range(n)]
        for r in range(0, n, 3):      # some held-out pairs are excluded as well
            if len(ex[r]) and len(ho[r]):
                ho[r] = np.union1d(ho[r], ex[r][:2])
        Hd, Wd = torch.from_numpy(H[:n]).to(dev), torch.from_numpy(W[:C]).to(dev)
        Vh, Ve = _coo(ho, n, C, dev), _coo(ex, n, C, dev)
        for exclude, exl in ((Ve, ex), (None, None)):
            rows, cols, ranks, scores, adm = _run_variants(Hd, Wd, Vh, exclude, (R, C))
            mask = E.excluded_mask(exl, n, C)
            assert np.array_equal(adm, C - mask.sum(1))
            _check_against_topk(Hd, Wd, exclude, rows, cols, ranks, scores)
            worst = max(worst, E.check_bounds(rows, cols, ranks, scores, s64[:n, :C], bound[:n, :C], mask))
    record('rank_scores', worst_fraction_of_bound=worst, R=R)
    print(f'rank_scores R={R}: worst |score - ref| / bound = {worst:.3f}')


# ---- the exclusion pattern ------------------------------------------------------------------------------------------------------
def test_rank_exclusion_pattern(dev):
    from torchnmf_amd.metrics import SparseTarget
    R, n, C = 33, 37, E.C_ALL
    H, W, s64, bound = _problem(R)
    Hd, Wd = torch.from_numpy(H[:n]).to(dev), torch.from_numpy(W).to(dev)
    ex = E.exclusion_pattern()
    ho = E.heldout_for_pattern(ex)
    mask = E.excluded_mask(ex, n, C)
    Vh, Ve = _coo(ho, n, C, dev), _coo(ex, n, C, dev, zeros=True)
    rows, cols, ranks, scores, adm = _run_variants(Hd, Wd, Vh, Ve, 'pattern')
    frac = E.check_bounds(rows, cols, ranks, scores, s64[:n], bound[:n], mask)
    assert np.array_equal(ranks == -1, mask[rows, cols]) and np.any(ranks == -1)
    assert np.all(ranks[rows == 5] == -1) and adm[5] == 0 and adm[6] == 2 and adm[0] == C
    assert sorted(ranks[rows == 6]) == [-1, 0, 1]
    _check_against_topk(Hd, Wd, Ve, rows, cols, ranks, scores)
    # prepared patterns give the same bits
    first = scoring.rank_scores(Hd, Wd, Vh, Ve)
    for h, e in ((SparseTarget(Vh), SparseTarget(Ve)), (Vh, SparseTarget(Ve)), (SparseTarget(Vh), Ve)):
        assert _same(first, scoring.rank_scores(Hd, Wd, h, e, _fill=NAN, _nsplit=3))
    # an empty pattern excludes nothing
    none = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (n, C)).to(dev)
    free = scoring.rank_scores(Hd, Wd, Vh, none, _fill=NAN)
    assert _same(free, scoring.rank_scores(Hd, Wd, Vh, _fill=NAN)) and bool((free.ranks >= 0).all())
    E.check_bounds(*_np(free)[:4], s64[:n], bound[:n])
    # no held-out pair at all
    empty = scoring.rank_scores(Hd, Wd, none, Ve)
    assert empty.ranks.shape == (0,) and empty.scores.shape == (0,) and empty.rows.shape == (0,)
    assert np.array_equal(empty.admissible.cpu().numpy(), adm)
    record('rank_exclusion', worst_fraction_of_bound=frac)


# ---- the promises ---------------------------------------------------------------------------------------------------------------
def test_rank_promises(dev):
    R, n, C = 100, E.N_ALL, E.C_ALL
    H, W, _, _ = _problem(R)
    Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    g = np.random.default_rng(11)
    ho = E.heldout_cycle(n, C, seed=4, shift=2)
    ex = [np.sort(g.choice(C, size=15, replace=False)) for _ in range(n)]
    Vh, Ve = _coo(ho, n, C, dev), _coo(ex, n, C, dev)
    keep = [Hd.clone(), Wd.clone(), Vh.indices().clone(), Vh.values().clone(), Ve.indices().clone(), Ve.values().clone()]
    rows, cols, ranks, scores, adm = _run_variants(Hd, Wd, Vh, Ve, 'promises')
    for a, b in zip(keep, [Hd, Wd, Vh.indices(), Vh.values(), Ve.indices(), Ve.values()]):
        assert torch.equal(a, b), 'an input changed'
    # a subset of the rows, run alone
    sub = np.sort(g.choice(n, size=40, replace=False))
    ho_sub = [ho[r] if r in set(sub.tolist()) else ho[r][:0] for r in range(n)]
    r2 = _np(scoring.rank_scores(Hd, Wd, _coo(ho_sub, n, C, dev), Ve, _fill=NAN))
    sel = np.isin(rows, sub)
    assert np.array_equal(r2[0], rows[sel]) and np.array_equal(r2[1], cols[sel]) and np.array_equal(r2[2], ranks[sel])
    assert np.array_equal(r2[3].view(np.int32), scores[sel].view(np.int32)) and np.array_equal(r2[4], adm)
    # the other held-out pairs of a row do not enter a pair's rank
    ho_one = [h[len(h) // 2:len(h) // 2 + 1] for h in ho]
    r3 = _np(scoring.rank_scores(Hd, Wd, _coo(ho_one, n, C, dev), Ve, _fill=NAN))
    pos = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(rows, cols))}
    at = np.array([pos[(int(a), int(b))] for a, b in zip(r3[0], r3[1])])
    assert np.array_equal(r3[2], ranks[at]) and np.array_equal(r3[3].view(np.int32), scores[at].view(np.int32))


# ---- the models -----------------------------------------------------------------------------------------------------------------
def _recall_from_topk(top, ho, ex_mask, k):
    idx = top.indices.cpu().numpy()
    per = []
    for r, h in enumerate(ho):
        h = h[~ex_mask[r, h]]
        if len(h):
            per.append(np.isin(h, idx[r]).sum() / len(h))
    return float(np.mean(per))


def _check_model(m, Hn, Wn, Vtest, Vtrain, ho, ex, n, C, name):
    ks = (1, 10, 200)      # 200: beyond scoring.MAX_K
    mask = E.excluded_mask(ex, n, C)
    r = m.rank_scores(Vtest, exclude=Vtrain)
    rows, cols, ranks, scores, adm = _np(r)
    frac = E.check_bounds(rows, cols, ranks, scores, T.scores64(Hn, Wn), T.topk_bound(Hn, Wn), mask)
    got = m.ranking_metrics(Vtest, ks=ks, exclude=Vtrain)
    ref = E.metrics_from_ranks(rows, ranks, adm, ks)
    assert set(got) == set(ref)
    for key, v in got.items():
        assert v.dtype == torch.float64 and v.dim() == 0 and v.device.type == 'cuda'
        assert abs(float(v) - ref[key]) <= 1e-12, (name, key, float(v), ref[key])
    assert abs(float(got['recall@10']) - _recall_from_topk(m.topk(10, exclude=Vtrain), ho, mask, 10)) <= 1e-12
    assert 0 <= float(got['auc']) <= 1 and float(got['rows']) == sum(1 for r_, h in enumerate(ho) if len(h[~mask[r_, h]]))
    record('rank_model', model=name, worst_fraction_of_bound=frac, **{k_: float(v) for k_, v in got.items()})
    return r, got


def test_nmf_ranking_metrics(dev):
    from torchnmf_amd.nmf import NMF
    R, n, C = 8, 40, 2 * TC + 9
    g = np.random.default_rng(12)
    H0, W0 = g.random((n, R), dtype=np.float32) + 0.1, g.random((C, R), dtype=np.float32) + 0.1
    both = [np.sort(g.choice(C, size=30, replace=False)) for _ in range(n)]
    ex = [b[g.random(len(b)) < 0.8] for b in both]                       # the train / test split
    ho = [np.setdiff1d(b, e) for b, e in zip(both, ex)]
    ho[3] = np.union1d(ho[3], ex[3][:1])                                # a test pair that the training set stores
    ho[4] = ho[4][:0]
    Vtrain, Vtest = _coo(ex, n, C, dev) * 2.5, _coo(ho, n, C, dev)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    m.fit(Vtrain, beta=1, max_iter=5, tol=-1e9, unstored='missing')
    Hn, Wn = m.H.detach().cpu().numpy(), m.W.detach().cpu().numpy()
    r, got = _check_model(m, Hn, Wn, Vtest, Vtrain, ho, ex, n, C, 'NMF')
    # a module in float64 is scored from fp32 copies
    md = NMF(W=torch.from_numpy(Wn), H=torch.from_numpy(Hn)).double().to(dev)
    assert _same(r, md.rank_scores(Vtest, exclude=Vtrain))
    gd = md.ranking_metrics(Vtest, ks=(1, 10, 200), exclude=Vtrain)
    assert all(torch.equal(gd[k], got[k]) or abs(float(gd[k]) - float(got[k])) <= 1e-12 for k in got)


def test_plca_ranking_metrics(dev):
    from torchnmf_amd.plca import PLCA
    R, n, C = 5, TR + 6, 2 * TC + 3
    g = np.random.default_rng(13)
    H0, W0, Z0 = g.random((n, R), dtype=np.float32), g.random((C, R), dtype=np.float32), g.random(R, dtype=np.float32)
    m = PLCA(W=torch.from_numpy(W0 / W0.sum(0)), H=torch.from_numpy(H0 / H0.sum(0)), Z=torch.from_numpy(Z0 / Z0.sum())).to(dev)
    HZ = (m.H.detach() * m.Z.detach()).cpu().numpy()
    Wn = m.W.detach().cpu().numpy()
    ex = [np.sort(g.choice(C, size=20, replace=False)) for _ in range(n)]
    ho = [np.setdiff1d(np.sort(g.choice(C, size=7, replace=False)), e) for e in ex]
    _check_model(m, HZ, Wn, _coo(ho, n, C, dev), _coo(ex, n, C, dev), ho, ex, n, C, 'PLCA')
