"""``NTF.fit(solver='ccd')`` on the device (csrc/nmfmu_sparse_ntf_ccd.hip, ``ntf.ntf_ccd_sweep``, ``ntf._CcdNtf``).

The sweep is ``nmfmu_sp_ccd_sweep``'s recurrence with ``q_e,k = fp32(Pa[a_e, k] Pb[b_e, k])`` as the panel value, so the checks of
tests/test_gpu_ccd.py apply to the materialised rows: the ``rows x nnz`` matrix whose entry e names row e of ``P_eff``.
1. per element, none left out: the counted bound of ``ccd_emulation.sweep_check`` with ``P_eff`` as the panel;
2. bitwise: equal to ``ccd.ccd_sweep`` on the materialised target, repeatable, independent of ``_order``, ``_limit``, ``_vec``;
3. the fit against a float64 loop of ``ccd_emulation.sweep`` on float64 ``P_eff``, initial scale included.
The owner mode has 5 and 257 rows with the counts of ``test_gpu_ccd._counts``; the other two modes are 23 x 29, so that a row of
513 entries has distinct (a, b)."""
import functools

import numpy as np
import pytest
import torch

import ccd_emulation as E
from conftest import record, rel_err
from test_gpu_ccd import GARBAGE, REG, TOL, WG_LOW, _counts

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 33, 64, 256]      # both gather forms (64, 256: four-wide) and the padded tail
MODES = [0, 1, 2]
DA, DB = 23, 29


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case(rows, rank):
    """(F, Pa, Pb, ptr, ia, ib, vals, P_eff): ``sweep_case`` over DA * DB panel rows, each split into its (a, b)."""
    F, _, ptr, cols, vals = E.sweep_case(_counts(rows), DA * DB, rank)
    rng = np.random.default_rng(rows + rank)
    Pa = (np.abs(rng.standard_normal((DA, rank))) + 0.05).astype(np.float32)
    Pb = (np.abs(rng.standard_normal((DB, rank))) + 0.05).astype(np.float32)
    ia, ib = cols // DB, cols % DB
    return F, Pa, Pb, ptr, ia, ib, vals, Pa[ia] * Pb[ib]      # (float32 * float32: one rounding)


def _run(dev, case, mode, reg, **kw):
    """The kernel on guarded storage -> out [rows, rank] numpy.  Asserts that the panels, the index and value arrays and the
    floats behind F are bitwise what they were."""
    from torchnmf_amd import ntf
    F, Pa, Pb, ptr, ia, ib, vals, _ = case
    rows, rank = F.shape
    own = np.repeat(np.arange(rows), np.diff(ptr))
    idx = np.stack([own, ia, ib])[[[0, 1, 2], [1, 0, 2], [1, 2, 0]][mode]]
    shape = [DA, DB]
    shape.insert(mode, rows)
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).coalesce()   # (stored zeros stay stored)
    T = ntf.SparseNtfTarget(V.to(dev))
    m = T.modes[mode]
    assert np.array_equal(m['rowptr'].cpu().numpy(), ptr) and m['vals'].cpu().numpy().tobytes() == vals.tobytes()
    assert np.array_equal(m['idx_a'].cpu().numpy(), ia) and np.array_equal(m['idx_b'].cpu().numpy(), ib)   # the same work list
    fbuf = torch.full((rows * rank + 64,), GARBAGE, device=dev)
    fbuf[:rows * rank] = torch.from_numpy(F).to(dev).reshape(-1)
    fs = [torch.from_numpy(Pa).to(dev), torch.from_numpy(Pb).to(dev)]
    fs.insert(mode, fbuf[:rows * rank].view(rows, rank))
    fixed = [f for n, f in enumerate(fs) if n != mode] + [m['rowptr'], m['idx_a'], m['idx_b'], m['vals']]
    keep = [t.clone() for t in fixed]
    assert ntf.ntf_ccd_sweep(T, fs, mode, *reg, **kw) is fs[mode]
    assert all(torch.equal(t, k) for t, k in zip(fixed, keep)) and bool((fbuf[rows * rank:] == GARBAGE).all())
    return fs[mode].cpu().numpy()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_per_element(dev, rank, mode):
    eps32, worst = np.float32(E.EPS), 0.0
    for rows in (5, 257):
        case = _case(rows, rank)
        F, _, _, ptr, _, _, vals, P_eff = case
        counts, z, every = np.diff(ptr), E.zero_row(np.diff(ptr)), np.arange(len(vals))
        assert (vals == 0).any() and (vals[ptr[z]:ptr[z + 1]] == 0).all()
        for reg, wg in (((0.0, 0.0), 0), (REG, WG_LOW)):
            got = _run(dev, case, mode, reg, _wg_rows=wg)
            assert np.isfinite(got).all() and (got >= eps32).all()
            frac = E.fraction(*E.sweep_check(got, F, P_eff, ptr, every, vals, *reg, wg_rows=wg or E.LIMIT))
            worst = max(worst, float(frac.max()))
            assert frac.max() <= 1.0, (rows, reg, wg, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
            assert got[counts == 0].tobytes() == F[counts == 0].tobytes()      # a row without data is not touched
            assert (got[z] == eps32).all()                                      # the all-zero row ends on the floor
    record('ntf_ccd_sweep_per_element', rank=rank, mode=mode, worst_fraction_of_bound=worst)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_bitwise(dev, rank, mode):
    from torchnmf_amd import ccd
    case = _case(257, rank)
    F, _, _, ptr, _, _, vals, P_eff = case
    counts, nnz = np.diff(ptr), len(vals)
    ij = torch.from_numpy(np.stack([np.repeat(np.arange(257), counts), np.arange(nnz)]))
    M = torch.sparse_coo_tensor(ij, torch.from_numpy(vals), (257, nnz)).coalesce().to(dev)      # the materialised rows
    Pd = torch.from_numpy(P_eff).to(dev)
    for wg in (0, WG_LOW):                        # (a row's path is a function of its count and this threshold)
        first = _run(dev, case, mode, REG, _wg_rows=wg)
        want = ccd.ccd_sweep(torch.from_numpy(F).to(dev), Pd, M, 'h', *REG, _wg_rows=wg).cpu().numpy()
        assert first.tobytes() == want.tobytes()
        assert _run(dev, case, mode, REG, _wg_rows=wg).tobytes() == first.tobytes()               # repeatable
        order = torch.from_numpy(np.argsort(counts, kind='stable').astype(np.int32)).to(dev)      # shortest first
        assert _run(dev, case, mode, REG, _wg_rows=wg, _order=order).tobytes() == first.tobytes()
        assert _run(dev, case, mode, REG, _wg_rows=wg, _limit=1).tobytes() == first.tobytes()     # every row through scratch
        for vec in (1, 2):                        # (ranks 64 and 256: 4-byte against 16-byte gathers)
            assert _run(dev, case, mode, REG, _wg_rows=wg, _vec=vec).tobytes() == first.tobytes(), vec
            assert _run(dev, case, mode, REG, _wg_rows=wg, _vec=vec, _limit=1).tobytes() == first.tobytes(), vec


# ---- fit(solver='ccd') ---------------------------------------------------------------------------------------------------------
def _objective(idx, vals, fs, l1=0.0, l2=0.0, train=(True,) * 3):
    d = vals - np.einsum('pr,pr,pr->p', *(f[i] for f, i in zip(fs, idx)))
    return 0.5 * float(d @ d) + sum(l1 * f.sum() + 0.5 * l2 * (f ** 2).sum() for f, on in zip(fs, train) if on)


def _emulate(idx, vals, fs, n_iter, l1=0.0, l2=0.0, train=(True,) * 3):
    """``_CcdNtf`` in float64: the once-only scale and clamp, then per trained mode ``ccd_emulation.sweep`` on the materialised
    rows of that mode's sorted copy with the float64 ``P_eff`` as the panel."""
    fs = [np.array(f, dtype=np.float64) for f in fs]
    s = np.einsum('pr,pr,pr->p', *(f[i] for f, i in zip(fs, idx)))
    a = float(vals @ s) / float(s @ s)
    fs = [np.maximum(f * a ** (1.0 / sum(train)), E.EPS) if on else f for f, on in zip(fs, train)]
    for _ in range(n_iter):
        for n in (m for m in range(3) if train[m]):
            o = np.lexsort((*[idx[m] for m in (2, 1, 0) if m != n], idx[n]))      # by (owner, a, b)
            ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[n], minlength=fs[n].shape[0]))])
            (pa, ia), (pb, ib) = ((fs[m], idx[m][o]) for m in range(3) if m != n)
            fs[n] = E.sweep(fs[n], pa[ia] * pb[ib], ptr, np.arange(len(vals)), vals[o], l1, l2)
    return fs


@functools.lru_cache(maxsize=None)
def _problem(full):
    """(idx [3, nnz] lexicographic, vals, shape, start): 20 x 15 x 12 at rank 5 with 30 % stored (row 3 of mode 0 stores
    nothing), or every entry of 12 x 10 x 9 at rank 4; values and start exactly representable in fp32."""
    rng = np.random.default_rng(17 + full)
    shape, rank = ((12, 10, 9), 4) if full else ((20, 15, 12), 5)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    true = [np.abs(rng.standard_normal((d, rank))) for d in shape]
    mask = np.ones(shape, dtype=bool) if full else rng.random(shape) < 0.3
    if not full:
        mask[3] = False
    idx = np.stack(np.nonzero(mask))
    vals = f32(np.einsum('pr,pr,pr->p', *(f[i] for f, i in zip(true, idx))) * (0.8 + 0.4 * rng.random(idx.shape[1])))
    return idx, vals, shape, [f32(np.abs(rng.standard_normal((d, rank)))) for d in shape]


def _fit(dev, full, n_iter, solver='ccd', train=(True,) * 3, **kw):
    from torchnmf_amd.ntf import NTF
    idx, vals, shape, start = _problem(full)
    m = NTF(factors=[torch.from_numpy(f).float() for f in start], trainable=train).to(dev)
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals).float(), shape).coalesce().to(dev)
    unstored = 'missing' if solver == 'ccd' else 'zero'
    assert m.fit(V, beta=2, solver=solver, unstored=unstored, tol=-1e9, max_iter=n_iter, **kw) == n_iter
    return [f.detach().double().cpu().numpy() for f in m.factors]


@pytest.mark.parametrize('reg, train', [(False, (True,) * 3), (True, (True,) * 3), (False, (True, False, True))])
def test_fit_against_float64(dev, reg, train):
    idx, vals, shape, start = _problem(False)
    kw = dict(alpha=0.07, l1_ratio=0.3) if reg else {}        # l1 = 0.021, l2 = 0.049: REG
    r = REG if reg else (0.0, 0.0)
    trace = [_objective(idx, vals, _emulate(idx, vals, start, 0, *r, train), *r, train)]
    for n_iter in (1, 2, 3):                                  # (each fit starts anew: the prefixes of one trajectory)
        got = _fit(dev, False, n_iter, train=train, **kw)
        trace.append(_objective(idx, vals, got, *r, train))
    errs = [rel_err(g, w) for g, w in zip(got, _emulate(idx, vals, start, 3, *r, train))]
    record('ntf_ccd_fit_vs_float64', reg=reg, train=list(train), rel_err=errs, objective=trace, tol=TOL)
    assert max(errs) < TOL, errs
    assert all(np.array_equal(g, s) for g, s, on in zip(got, start, train) if not on)          # a frozen factor stays
    assert all(g.min() >= E.EPS for g, on in zip(got, train) if on)
    assert (np.diff(trace) <= 0).all(), trace                # the float64 objective of the device's factors never rises


def test_fully_stored_target(dev):
    idx, vals, shape, start = _problem(True)
    got, want = _fit(dev, True, 10), _emulate(idx, vals, start, 10)
    errs = [rel_err(g, w) for g, w in zip(got, want)]
    record('ntf_ccd_fully_stored', rel_err=errs, loss=_objective(idx, vals, got), float64_loss=_objective(idx, vals, want),
           hals_loss=_objective(idx, vals, _fit(dev, True, 10, solver='hals')), tol=TOL)
    assert max(errs) < TOL, errs
