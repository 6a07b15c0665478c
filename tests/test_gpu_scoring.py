"""Scoring on the device (csrc/nmfmu_score.hip, torchnmf_amd/scoring.py, NMF / PLCA .predict and .topk) against float64
arithmetic on the CPU, under the checker and the bounds of tests/topk_emulation.py -- every row, no element left out.

The shapes are derived from the kernel's tile (TR x TC = scoring.TILE_ROWS x TILE_COLS): one row, one short of a row block,
one over, more than two blocks; one column, one short of a tile, a whole tile, one over, three tiles and a ragged fourth;
every padded-rank / RL family of the sparse kernels and odd ranks for the 2-wide MFMA; k at the list's lane boundaries.  The
factors of one rank are drawn once and the float64 scores computed once; every case reads slices of them.

Measured on an MI355X (worst |got - ref| / bound; whether topk values equal m()[i, idx] bit for bit): DESIGN.md section 21.
"""
import functools

import numpy as np
import pytest
import torch

import topk_emulation as E
from conftest import record

pytestmark = pytest.mark.gpu

from torchnmf_amd import scoring  # noqa: E402

TR, TC = scoring.TILE_ROWS, scoring.TILE_COLS
N_ALL, C_ALL = 2 * TR + 3, 3 * TC + 17
N_ROWS = [1, TR - 1, TR + 1, 2 * TR + 3]
COLS = [1, TC - 1, TC, TC + 1, 3 * TC + 17]
RANKS = [1, 3, 33, 100, 200, 256]
KS = [1, 5, 64, 65, 128]
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(R):
    """(H, W fp32; float64 scores and bound of all rows x all columns); treated as read-only."""
    g = np.random.default_rng(1000 + R)
    H = g.random((N_ALL, R), dtype=np.float32) + np.float32(0.01)
    W = g.random((C_ALL, R), dtype=np.float32) + np.float32(0.01)
    return H, W, E.scores64(H, W), E.topk_bound(H, W)


@functools.lru_cache(maxsize=None)
def _rows(n_rows):
    """A shuffled, repeating request of n_rows rows out of N_ALL."""
    g = np.random.default_rng(n_rows)
    r = g.integers(0, N_ALL, size=n_rows)
    if n_rows > 2:
        r[1] = r[0]
    return r


def _same(a, b):
    return torch.equal(a.values.view(torch.int32), b.values.view(torch.int32)) and torch.equal(a.indices, b.indices)


def _run_variants(Hd, Wd, k, rows_d, exclude, C, n_rows):
    """The chosen split and forced 1 / 2 / 3, outputs and workspace pre-filled with NaN: all bitwise equal, and a second call
    equal to the first.  Returns the answer as numpy."""
    first = scoring.topk_scores(Hd, Wd, k, rows=rows_d, exclude=exclude, _fill=NAN)
    assert first.values.dtype == torch.float32 and first.indices.dtype == torch.int64
    assert not first.values.requires_grad
    for ns in (1, 2, 3):
        other = scoring.topk_scores(Hd, Wd, k, rows=rows_d, exclude=exclude, _nsplit=ns, _fill=NAN)
        assert _same(first, other), ('nsplit', ns, C, n_rows, k)
    assert _same(first, scoring.topk_scores(Hd, Wd, k, rows=rows_d, exclude=exclude, _fill=NAN))
    return first.values.cpu().numpy(), first.indices.cpu().numpy()


# ---- the basic sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('R', RANKS)
def test_topk_sweep(dev, R, k):
    H, W, s64, bound = _problem(R)
    Hd_all, Wd_all = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    worst = 0.0
    for C in COLS:
        Wd = Wd_all[:C].contiguous()
        for n_rows in N_ROWS:
            for by_rows in (False, True):
                if by_rows:
                    r = _rows(n_rows)
                    Hd, rows_d = Hd_all, torch.from_numpy(r).to(dev)
                    if n_rows % 2:
                        rows_d = rows_d.int()
                else:
                    r = np.arange(n_rows)
                    Hd, rows_d = Hd_all[:n_rows].contiguous(), None
                vals, idx = _run_variants(Hd, Wd, k, rows_d, None, C, n_rows)
                worst = max(worst, E.check_topk(vals, idx, s64[r][:, :C], bound[r][:, :C], k))
    record('topk_sweep', worst_fraction_of_bound=worst, R=R, k=k)
    print(f'topk R={R} k={k}: worst |got - ref| / bound = {worst:.3f}')


# ---- exclusion ----------------------------------------------------------------------------------------------------------------
def _pattern():
    """37 x C_ALL: rows cycle through 0, 1, 4, 5, 8, 9, 20 stored columns; row 3 stores a run across the first tile edge, row
    4 a run of more than 64 columns across the second tile edge (a split edge for nsplit = 3 and 2), row 5 every column, row
    6 all but 2."""
    g = np.random.default_rng(37)
    counts = [0, 1, 4, 5, 8, 9, 20]
    ex = [np.sort(g.choice(C_ALL, size=counts[r % 7], replace=False)) for r in range(37)]
    ex[3] = np.arange(TC - 3, TC + 4)
    ex[4] = np.arange(2 * TC - 70, 2 * TC + 5)
    ex[5] = np.arange(C_ALL)
    ex[6] = np.setdiff1d(np.arange(C_ALL), [TC - 1, 2 * TC])
    return ex


def _coo(ex, n, C, dev, zeros=False):
    ri = np.concatenate([np.full(len(e), r) for r, e in enumerate(ex)]).astype(np.int64)
    ci = np.concatenate(ex).astype(np.int64)
    v = np.ones(len(ri), dtype=np.float32)
    if zeros:
        v[::2] = 0          # a stored zero counts
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([ri, ci])), torch.from_numpy(v), (n, C)).to(dev)


@pytest.mark.parametrize('k', [5, 65])
def test_topk_exclusion(dev, k):
    from torchnmf_amd.metrics import SparseTarget
    R, n = 33, 37
    H, W, s64, bound = _problem(R)
    Hd, Wd = torch.from_numpy(H[:n]).to(dev), torch.from_numpy(W).to(dev)
    ex = _pattern()
    mask = E.excluded_mask(ex, n, C_ALL)
    Vs = _coo(ex, n, C_ALL, dev, zeros=True)
    vals, idx = _run_variants(Hd, Wd, k, None, Vs, C_ALL, n)
    frac = E.check_topk(vals, idx, s64[:n], bound[:n], k, mask)
    assert np.all(idx[5] == -1) and np.all(np.isneginf(vals[5]))
    assert sorted(idx[6][:2]) == [TC - 1, 2 * TC] and np.all(idx[6][2:] == -1)
    # the same pattern prepared once, and through a shuffled request
    T = SparseTarget(Vs)
    again = scoring.topk_scores(Hd, Wd, k, exclude=T, _fill=NAN)
    assert np.array_equal(again.values.cpu().numpy().view(np.int32), vals.view(np.int32))
    assert np.array_equal(again.indices.cpu().numpy(), idx)
    r = np.random.default_rng(k).integers(0, n, size=50)
    sub = scoring.topk_scores(Hd, Wd, k, rows=torch.from_numpy(r).to(dev), exclude=T, _nsplit=3, _fill=NAN)
    assert np.array_equal(sub.indices.cpu().numpy(), idx[r])
    assert np.array_equal(sub.values.cpu().numpy().view(np.int32), vals[r].view(np.int32))
    # an empty pattern excludes nothing
    none = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (n, C_ALL)).to(dev)
    free = scoring.topk_scores(Hd, Wd, k, exclude=none, _fill=NAN)
    assert _same(free, scoring.topk_scores(Hd, Wd, k, _fill=NAN))
    E.check_topk(free.values.cpu().numpy(), free.indices.cpu().numpy(), s64[:n], bound[:n], k)
    record('topk_exclusion', worst_fraction_of_bound=frac, k=k)


# ---- the order, on scores that are exact in fp32 --------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['ascending', 'descending', 'equal', 'duplicated'])
def test_topk_order_exact(dev, order):
    """Integer-valued factors: every score is exact in fp32 whatever the summation order, so the expected output is the
    stable sort, compared exactly."""
    C = C_ALL
    col = np.arange(C, dtype=np.float32)
    if order == 'ascending':            # every column is inserted
        w0 = col
    elif order == 'descending':         # nothing enters after the first k
        w0 = C - col
    elif order == 'equal':
        w0 = np.full(C, 3, dtype=np.float32)
    else:                               # equal rows of W in different tiles and splits
        w0 = np.concatenate([col[:TC], col[:TC], col[:TC], col[:17]])
    W = np.stack([w0, np.ones(C, dtype=np.float32), 2 * np.ones(C, dtype=np.float32)], 1)       # rank 3
    H = np.stack([np.arange(1, TR + 3), np.ones(TR + 2), np.arange(TR + 2) % 5], 1).astype(np.float32)
    S = (H.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    assert np.array_equal(S.astype(np.float64), H.astype(np.float64) @ W.astype(np.float64).T)
    Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    for k in (5, 65, 128):
        ref = E.sort_topk(S, k)
        if order == 'equal':
            assert np.array_equal(ref[1], np.tile(np.arange(k), (TR + 2, 1)))
        vals, idx = _run_variants(Hd, Wd, k, None, None, C, TR + 2)
        assert np.array_equal(idx, ref[1]), (order, k)
        assert np.array_equal(vals, ref[0]), (order, k)


# ---- pairs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
def test_score_pairs(dev, R):
    H, W, _, _ = _problem(R)
    Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    worst = 0.0
    for n in (0, 1, 63, 64, 65, 1000):
        g = np.random.default_rng(n)
        rows, cols = g.integers(0, N_ALL, size=n), g.integers(0, C_ALL, size=n)
        if n > 2:
            rows[1], cols[1] = rows[0], cols[0]
        rd, cd = torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)
        got = scoring.score_pairs(Hd, Wd, rd, cd)
        assert got.shape == (n,) and got.dtype == torch.float32 and not got.requires_grad
        assert torch.equal(got, scoring.score_pairs(Hd, Wd, rd.int(), cd.int()))
        ref, bound = E.pairs_ref_bound(H, W, rows, cols)
        err = np.abs(got.double().cpu().numpy() - ref)
        assert np.all(err <= bound), (R, n, float((err / bound).max()))
        if n:
            worst = max(worst, float((err / bound).max()))
    record('score_pairs', worst_fraction_of_bound=worst, R=R)
    print(f'score_pairs R={R}: worst |got - ref| / bound = {worst:.3f}')


def test_index_range(dev):
    H, W, _, _ = _problem(3)
    Hd, Wd = torch.from_numpy(H).to(dev), torch.from_numpy(W).to(dev)
    ok = torch.zeros(2, dtype=torch.int64, device=dev)
    for bad in (torch.tensor([0, N_ALL], device=dev), torch.tensor([-1, 0], device=dev)):
        with pytest.raises(IndexError):
            scoring.score_pairs(Hd, Wd, bad, ok)
        with pytest.raises(IndexError):
            scoring.topk_scores(Hd, Wd, 2, rows=bad)
    with pytest.raises(IndexError):
        scoring.score_pairs(Hd, Wd, ok, torch.tensor([0, C_ALL], device=dev))
    empty = scoring.topk_scores(Hd, Wd, 2, rows=ok[:0])
    assert empty.values.shape == (0, 2) and empty.indices.shape == (0, 2) and empty.indices.dtype == torch.int64


# ---- the models ---------------------------------------------------------------------------------------------------------------
def test_nmf_predict_and_topk(dev):
    from torchnmf_amd.nmf import NMF
    R, n, C, k = 8, 40, TC + 9, 6
    g = np.random.default_rng(8)
    H0, W0 = g.random((n, R), dtype=np.float32) + 0.1, g.random((C, R), dtype=np.float32) + 0.1
    ex = [np.sort(g.choice(C, size=12, replace=False)) for _ in range(n)]
    V = _coo(ex, n, C, dev) * 2.5
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    m.fit(V, beta=1, max_iter=5, tol=-1e9, unstored='missing')
    Hn, Wn = m.H.detach().cpu().numpy(), m.W.detach().cpu().numpy()
    s64, bound = E.scores64(Hn, Wn), E.topk_bound(Hn, Wn)
    # predict against the entries of m() and against float64
    rows, cols = g.integers(0, n, size=200), g.integers(0, C, size=200)
    got = m.predict(torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev))
    ref, pb = E.pairs_ref_bound(Hn, Wn, rows, cols)
    assert np.all(np.abs(got.double().cpu().numpy() - ref) <= pb)
    with torch.no_grad():
        full = m().double().cpu().numpy()
    assert np.all(np.abs(got.double().cpu().numpy() - full[rows, cols]) <= pb + bound[rows, cols])
    # the k best unobserved columns
    out = m.topk(k, exclude=V)
    vals, idx = out.values.cpu().numpy(), out.indices.cpu().numpy()
    frac = E.check_topk(vals, idx, s64, bound, k, E.excluded_mask(ex, n, C))
    # recorded, not asserted: are the values the bits of m()?
    same_bits = bool(np.array_equal(vals.view(np.int32), np.take_along_axis(full.astype(np.float32), idx, 1).view(np.int32)))
    record('nmf_topk_model', worst_fraction_of_bound=frac, bitwise_equal_to_forward=same_bits)
    print(f'NMF.topk: worst fraction {frac:.3f}; values bitwise equal to m()[i, idx]: {same_bits}')
    # a module in float64 is scored from fp32 copies
    md = NMF(W=torch.from_numpy(Wn), H=torch.from_numpy(Hn)).double().to(dev)
    outd = md.topk(k, exclude=V)
    assert outd.values.dtype == torch.float32 and _same(out, outd)
    assert torch.equal(md.predict(torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)), got)


def test_plca_predict_and_topk(dev):
    from torchnmf_amd.plca import PLCA
    R, n, C, k = 5, TR + 6, TC + 3, 4
    g = np.random.default_rng(9)
    H0, W0, Z0 = g.random((n, R), dtype=np.float32), g.random((C, R), dtype=np.float32), g.random(R, dtype=np.float32)
    m = PLCA(W=torch.from_numpy(W0 / W0.sum(0)), H=torch.from_numpy(H0 / H0.sum(0)), Z=torch.from_numpy(Z0 / Z0.sum())).to(dev)
    HZ = (m.H.detach() * m.Z.detach()).cpu().numpy()
    Wn = m.W.detach().cpu().numpy()
    s64, bound = E.scores64(HZ, Wn), E.topk_bound(HZ, Wn)
    rows_np = g.integers(0, n, size=20)
    rows = torch.from_numpy(rows_np).to(dev)
    out = m.topk(k, rows=rows)
    frac = E.check_topk(out.values.cpu().numpy(), out.indices.cpu().numpy(), s64[rows_np], bound[rows_np], k)
    cols_np = g.integers(0, C, size=20)
    cols = torch.from_numpy(cols_np).to(dev)
    ref, pb = E.pairs_ref_bound(HZ, Wn, rows_np, cols_np)
    got = m.predict(rows, cols)
    assert np.all(np.abs(got.double().cpu().numpy() - ref) <= pb)
    scaled = m.predict(rows, cols, norm=3.0)
    assert torch.equal(scaled, got * 3.0)
    record('plca_topk_model', worst_fraction_of_bound=frac)
