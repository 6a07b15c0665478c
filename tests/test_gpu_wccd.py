"""``fit(solver='ccd', unstored=omega)`` on the device (csrc/nmfmu_sparse_wccd.hip, torchnmf_amd/wccd.py, the solver branch of
``fit``).

1. The sweep kernel per element, no element left out: the coordinate fixed point recomputed in float64 from the device's own
   output (and the Gram matrix as the device wrote it) under the running-error bound of tests/wccd_emulation.py, on both
   sides, with row counts on either side of a wave's 64 entries and of the register residency limit, stored zeros, an
   all-zero row and rows without entries -- which are swept like every other row.
2. The bitwise promises: repeatable; a row independent of the other rows of the call, of the order list and of where its
   residuals live (registers or scratch) -- on the one-wave path and on the workgroup path.
3. ``fit(solver='ccd', unstored=omega)`` against the float64 emulation of the whole procedure (initial scale included), the
   loss sequence, the engine's loss against float64, and the rows without data.

Measured on an MI355X: see DESIGN.md section 27.
"""
import functools

import numpy as np
import pytest
import torch

import wccd_emulation as E
from conftest import record, rel_err

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 33, 64, 65, 100, 256]       # 65: the first coordinate in a lane's second slot of q
SIDES = ['h', 'w']
N_PANEL = 600
BASE = (0, 1, 63, 64, 65, 129)             # nothing, one lane, a wave's edge on both sides, three slots with a tail
EDGE = (E.LIMIT - 1, E.LIMIT, E.LIMIT + 1)   # the residency limit of a wave, which is also the default workgroup threshold
WG_LOW = 100                               # a lowered workgroup threshold: the rows of 129 entries and more take a workgroup
OMEGAS = (0.0625, 0.3)                     # one exact in fp32 (c = 1 - omega exact too), one rounded
REG = (0.021, 0.049)
NOREG = (0.0, 0.0)
GARBAGE = -7.0
TOL = 1e-4                                 # the project's bar for factors
# (omega, regularisation, _wg_rows): both weights with and without regularisation, under the default and the lowered threshold
CONFIGS = ((OMEGAS[0], NOREG, 0), (OMEGAS[1], REG, 0), (OMEGAS[1], NOREG, WG_LOW), (OMEGAS[0], REG, WG_LOW))


def _counts(rows):
    if rows == 1:
        return [129]
    if rows == 5:
        return [EDGE[0], 0, EDGE[1], EDGE[2], 64]
    c = [BASE[i % len(BASE)] for i in range(rows)]
    c[100], c[101], c[102] = EDGE
    return c


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case(rows, rank):
    return E.sweep_case(_counts(rows), N_PANEL, rank)


def _target(dev, ptr, cols, vals, rows, side):
    """The sparse-COO target whose `side` work list is (ptr, cols, vals): owner rows are rows of V ('h') or columns ('w')."""
    own = np.repeat(np.arange(rows), np.diff(ptr))
    ij = np.stack([own, cols] if side == 'h' else [cols, own])
    shape = (rows, N_PANEL) if side == 'h' else (N_PANEL, rows)
    V = torch.sparse_coo_tensor(torch.from_numpy(ij), torch.from_numpy(vals), shape).coalesce()   # (stored zeros stay stored)
    assert V._nnz() == len(vals)
    return V.to(dev)


def _gram(Pd):
    """``nmfmu_gram`` of a device panel -> a device [R, R] tensor."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    R = Pd.shape[1]
    part = torch.empty(max(lib.nmfmu_gram_part_bytes(R), 16), dtype=torch.uint8, device=Pd.device)
    G = torch.empty(R, R, dtype=torch.float32, device=Pd.device)
    _capi.check(lib.nmfmu_gram(Pd.data_ptr(), Pd.shape[0], R, part.data_ptr(), G.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), 'nmfmu_gram')
    return G


def _run_sweep(dev, case, side, omega, reg, own_gram=True, **kw):
    """The kernel on guarded storage -> (out [rows, rank], G [rank, rank]) numpy, G as the kernel read it.  Asserts that the
    panel, the Gram matrix, the index and value arrays and the floats behind F are bitwise what they were."""
    from torchnmf_amd.sparse_autograd import SparseTarget
    from torchnmf_amd.wccd import wccd_sweep
    F, P, ptr, cols, vals = case
    rows, rank = F.shape
    T = SparseTarget(_target(dev, ptr, cols, vals, rows, side))
    (tp, ti, tv), _, _, _ = T.side(side)
    assert np.array_equal(tp.cpu().numpy(), ptr) and np.array_equal(ti.cpu().numpy(), cols)        # the same work list
    assert tv.cpu().numpy().tobytes() == vals.tobytes()
    fbuf = torch.full((rows * rank + 64,), GARBAGE, device=dev)
    fbuf[:rows * rank] = torch.from_numpy(F).to(dev).reshape(-1)
    Fv = fbuf[:rows * rank].view(rows, rank)
    Pd = torch.from_numpy(P).to(dev)
    Gd = _gram(Pd)
    assert torch.equal(Gd, Gd.t())                                      # symmetric bit for bit: coordinate k reads row k
    keep = [t.clone() for t in (Pd, Gd, tp, ti, tv)]
    out = wccd_sweep(Fv, Pd, T, side, omega, *reg, G=Gd if own_gram else None, **kw)
    assert out is Fv
    for t, k in zip((Pd, Gd, tp, ti, tv), keep):
        assert torch.equal(t, k)
    assert bool((fbuf[rows * rank:] == GARBAGE).all())
    return Fv.cpu().numpy(), Gd.cpu().numpy()


# ---- 1. the sweep, per element -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_per_element(dev, rank, side):
    worst, worst_empty = 0.0, 0.0
    eps32 = np.float32(E.EPS)
    for rows in (1, 5, 257):
        case = _case(rows, rank)
        F, P, ptr, cols, vals = case
        counts = np.diff(ptr)
        assert (vals == 0).any()
        z = E.zero_row(counts)
        assert (z is None) == (rows == 1)
        if z is not None:
            assert (vals[ptr[z]:ptr[z + 1]] == 0).all()                    # the all-zero row
        for omega, reg, wg in CONFIGS:
            got, G = _run_sweep(dev, case, side, omega, reg, _wg_rows=wg)
            assert np.isfinite(got).all() and (got >= eps32).all()
            err, bound = E.sweep_check(got, F, P, G, ptr, cols, vals, omega, *reg, wg_rows=wg or E.LIMIT)
            assert (bound > 0).all()                                        # every element of every row is judged
            frac = E.fraction(err, bound)
            print(f'wccd sweep rows={rows} rank={rank} side={side} omega={omega} reg={reg} wg={wg}: '
                  f'worst err / bound = {frac.max():.4f}')
            worst = max(worst, float(frac.max()))
            if (counts == 0).any():
                worst_empty = max(worst_empty, float(frac[counts == 0].max()))
            assert frac.max() <= 1.0, (rows, rank, side, omega, reg, wg, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
            if rows == 257 and rank > 1:       # (the data's premise: both sides of the clamp are exercised)
                rest = got[counts > 0]
                assert (rest == eps32).any() and (rest != eps32).any()
    c_res, S, S_q = E.bound_terms(rank, rank - 1, E.LIMIT + 1)
    record('wccd_sweep_per_element', rank=rank, side=side, worst_fraction_of_bound=worst,
           worst_fraction_rows_without_entries=worst_empty, c_res_max=c_res, S_max=S, S_q=S_q)


def test_default_gram_is_nmfmu_gram(dev):
    """``G=None`` computes the Gram matrix with ``nmfmu_gram``: the same bits as the sweep on that matrix handed in."""
    case = _case(5, 33)
    for side in SIDES:
        a, _ = _run_sweep(dev, case, side, 0.3, REG, own_gram=True)
        b, _ = _run_sweep(dev, case, side, 0.3, REG, own_gram=False)
        assert a.tobytes() == b.tobytes()


def test_target_without_entries_is_swept(dev):
    from torchnmf_amd.wccd import wccd_sweep
    V = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (5, 4)).to(dev)
    F, P = torch.rand(5, 3, device=dev) + 0.1, torch.rand(4, 3, device=dev) + 0.1
    old = F.cpu().numpy().copy()
    G = _gram(P)
    got = wccd_sweep(F, P, V, 'h', 0.3, G=G).cpu().numpy()
    ptr = np.zeros(6, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    err, bound = E.sweep_check(got, old, P.cpu().numpy(), G.cpu().numpy(), ptr, none, none.astype(np.float32), 0.3)
    assert E.fraction(err, bound).max() <= 1.0 and (got < old).all()


# ---- 2. the bitwise promises -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_bitwise(dev, rank, side):
    case = _case(257, rank)
    F, P, ptr, cols, vals = case
    counts = np.diff(ptr)
    omega = OMEGAS[1]
    pick = [102, 3, 101, 4, 100, 5, 0, 256]       # the rows around the limit, a few short ones and one without entries
    assert counts[0] == 0
    sptr = np.zeros(len(pick) + 1, dtype=np.int64)
    sptr[1:] = np.cumsum(counts[pick])
    scols = np.concatenate([cols[ptr[i]:ptr[i + 1]] for i in pick])
    svals = np.concatenate([vals[ptr[i]:ptr[i + 1]] for i in pick])
    firsts = []
    for wg in (0, WG_LOW):                        # (a row's path is a function of its count and this threshold)
        first, _ = _run_sweep(dev, case, side, omega, REG, _wg_rows=wg)
        firsts.append(first)
        assert _run_sweep(dev, case, side, omega, REG, _wg_rows=wg)[0].tobytes() == first.tobytes()          # repeatable
        # the order list: reversed (shortest first) and a fixed shuffle
        for order in (np.argsort(counts, kind='stable'), np.random.default_rng(5).permutation(257)):
            got, _ = _run_sweep(dev, case, side, omega, REG, _wg_rows=wg,
                                _order=torch.from_numpy(order.astype(np.int32)).to(dev))
            assert got.tobytes() == first.tobytes()
        # where the residuals live: with `limit` entries per wave in registers, the longer rows go through the scratch buffer
        # (limit 8: every one-wave row above 8 entries and every workgroup row above 128)
        for limit in (8, 64, 128, E.LIMIT - 1):
            assert _run_sweep(dev, case, side, omega, REG, _wg_rows=wg, _limit=limit)[0].tobytes() == first.tobytes(), limit
        # a subset of the rows alone, in another call and other workgroups
        sub, _ = _run_sweep(dev, (F[pick].copy(), P, sptr, scols, svals), side, omega, REG, _wg_rows=wg)
        assert sub.tobytes() == first[pick].tobytes()
    short = counts <= WG_LOW                      # rows on the same path under both thresholds have the same bits
    assert firsts[0][short].tobytes() == firsts[1][short].tobytes()


def test_sweep_argument_checks(dev):
    from torchnmf_amd.wccd import wccd_sweep
    V = torch.sparse_coo_tensor(torch.tensor([[0, 1, 4], [2, 3, 0]]), torch.tensor([1.0, 0.5, 2.0]), (5, 4)).to(dev)
    F, P = torch.rand(5, 3, device=dev), torch.rand(4, 3, device=dev)
    keep = F.clone()
    with pytest.raises(TypeError):
        wccd_sweep(F.double(), P, V, 'h', 0.3)
    with pytest.raises(TypeError):
        wccd_sweep(F, P.double(), V, 'h', 0.3)
    with pytest.raises(TypeError):
        wccd_sweep(F, P, V, 'h', 0.3, G=torch.rand(3, 3, device=dev).double())
    with pytest.raises(ValueError):
        wccd_sweep(F, P, V, 'h', 0.3, G=torch.rand(4, 4, device=dev))
    with pytest.raises(ValueError):
        wccd_sweep(F.t(), P, V, 'h', 0.3)                  # not contiguous: it cannot be updated in place
    with pytest.raises(ValueError):
        wccd_sweep(F, P, V, 'w', 0.3)                      # the shapes of the other side
    with pytest.raises(ValueError):
        wccd_sweep(F, P[:3], V, 'h', 0.3)
    with pytest.raises(ValueError):
        wccd_sweep(F, P, V.to_dense(), 'h', 0.3)
    with pytest.raises(ValueError):
        wccd_sweep(F, P, V, 'h', 0.3, _limit=E.LIMIT + 1)
    for bad in (0.0, 1.0, float('nan'), True):
        with pytest.raises(ValueError):
            wccd_sweep(F, P, V, 'h', bad)
    with pytest.raises(NotImplementedError):
        wccd_sweep(torch.rand(5, 257, device=dev), torch.rand(4, 257, device=dev), V, 'h', 0.3)
    assert torch.equal(F, keep)
    assert wccd_sweep(P.clone(), F, V, 'w', 0.3).shape == (4, 3)


# ---- 3. fit(solver='ccd', unstored=omega) ----------------------------------------------------------------------------------------
OMEGA_FIT = 0.05


@functools.lru_cache(maxsize=None)
def _problem(name):
    return E.fit_case(name)


@functools.lru_cache(maxsize=None)
def _emulated(name, omega, n_iter, tol=-1e300, reg=NOREG, train_W=True):
    idx, vals, shape, W0, H0 = _problem(name)
    return E.fit(idx, vals, shape, W0, H0, omega, n_iter, tol=tol, l1=reg[0], l2=reg[1], train_W=train_W)


def _module(dev, name, **kw):
    from torchnmf_amd.nmf import NMF
    idx, vals, shape, W0, H0 = _problem(name)
    m = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float(), **kw).to(dev)
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals).float(), shape).coalesce().to(dev)
    return m, V


def _np(t):
    return t.detach().double().cpu().numpy()


# alpha, l1_ratio with l1 = alpha l1_ratio = 0.021 and l2 = alpha (1 - l1_ratio) = 0.049
ALPHA = dict(alpha=0.07, l1_ratio=0.3)


@pytest.mark.parametrize('reg', [False, True])
@pytest.mark.parametrize('name', ['small', 'mid'])
def test_fit_against_float64(dev, name, reg):
    """Ten iterations with tol out of the way (no stop decision to agree on), then the same count and the same factors."""
    m, V = _module(dev, name)
    kw = dict(ALPHA) if reg else {}
    r = REG if reg else NOREG
    Wr, Hr, nr = _emulated(name, OMEGA_FIT, 10, -1e300, r)
    n = m.fit(V, beta=2, tol=-1e9, max_iter=10, solver='ccd', unstored=OMEGA_FIT, **kw)
    ew, eh = rel_err(m.W.data.cpu(), Wr), rel_err(m.H.data.cpu(), Hr)
    record('wccd_fit_vs_float64', problem=name, reg=reg, omega=OMEGA_FIT, n_iter=n, emulated_n_iter=nr, rel_err_W=ew,
           rel_err_H=eh, tol=TOL)
    assert n == nr == 10 and m.last_precision == 'fp32'
    assert ew < TOL and eh < TOL, (ew, eh)
    assert float(m.W.data.min()) >= E.EPS and float(m.H.data.min()) >= E.EPS


def test_fit_stops_where_the_emulation_stops(dev):
    """'small' with omega = 0.3 and tol = 1e-2 stops the emulation at 30: the ratios at the checkpoints are 0.42, 0.0120 and
    0.0069 -- every decision has a margin of 17 % or more, against a drift of the fp32 factors of about 1e-6."""
    idx, vals, shape, W0, H0 = _problem('small')
    Wr, Hr, nr = _emulated('small', OMEGAS[1], 200, 1e-2)
    m, V = _module(dev, 'small')
    n = m.fit(V, beta=2, tol=1e-2, max_iter=200, solver='ccd', unstored=OMEGAS[1], precision='bf16')
    ew, eh = rel_err(m.W.data.cpu(), Wr), rel_err(m.H.data.cpu(), Hr)
    record('wccd_fit_stop', omega=OMEGAS[1], n_iter=n, emulated_n_iter=nr, rel_err_W=ew, rel_err_H=eh, tol=TOL)
    assert n == nr and nr < 200 and m.last_precision == 'fp32'
    assert ew < TOL and eh < TOL, (ew, eh)


def test_frozen_W(dev):
    m, V = _module(dev, 'mid', trainable_W=False)
    keep = m.W.data.clone()
    assert m.fit(V, beta=2, tol=-1e9, max_iter=3, solver='ccd', unstored=OMEGAS[1]) == 3
    assert torch.equal(m.W.data, keep) and not m.W.requires_grad
    Wr, Hr, _ = _emulated('mid', OMEGAS[1], 3, train_W=False)
    eh = rel_err(m.H.data.cpu(), Hr)
    record('wccd_frozen_W', omega=OMEGAS[1], rel_err_H=eh, tol=TOL)
    assert eh < TOL, eh


@pytest.mark.parametrize('name', ['small', 'mid'])
def test_loss_sequence_never_increases(dev, name):
    """Ten iterations of the engine.  The objective the sweeps descend on, evaluated on the host in float64 from the device's
    factors after every half-step, and (without regularisation) the engine's own loss: non-increasing within 1e-5 relative.
    The engine's loss against the float64 loss of its factors: 1e-5 relative, at every point."""
    from torchnmf_amd.wccd import WeightedCcdEngine
    idx, vals, shape, _, _ = _problem(name)
    for omega, reg in ((OMEGA_FIT, NOREG), (OMEGAS[1], REG)):
        m, V = _module(dev, name)
        eng = WeightedCcdEngine(V, m.W.data, m.H.data, omega, *reg)
        assert eng.target_flags() == (False, True)
        seq, trace, host = [eng.divergence()], [], []        # (the initial scale happens here, as in fit's loss_init)

        def note():
            trace.append(E.objective(idx, vals, _np(m.W), _np(m.H), omega, *reg))
            host.append(E.divergence(idx, vals, _np(m.W), _np(m.H), omega))
        note()
        for _ in range(10):
            for step in (eng.w_step, eng.h_step):
                step()
                seq.append(eng.divergence())
                note()
        seq, trace, host = np.array(seq), np.array(trace), np.array(host)
        rise = float((np.diff(trace) / trace[:-1]).max())
        rise_own = float((np.diff(seq) / seq[:-1]).max())
        off = float((np.abs(seq - host) / host).max())
        record('wccd_loss_sequence', problem=name, omega=omega, reg=list(reg), worst_relative_rise_objective=rise,
               worst_relative_rise_own_loss=rise_own, loss_vs_float64=off)
        assert rise <= 1e-5, rise
        if reg == NOREG:
            assert rise_own <= 1e-5, rise_own
        assert off <= 1e-5, off
        assert abs(host[-1] - E.dense_divergence(idx, vals, shape, _np(m.W), _np(m.H), omega)) <= 1e-9 * host[-1]
        assert seq[-1] < 0.9 * seq[0]          # (progress: the float64 emulation ends at 0.43 and 0.58 of its start on 'mid', below 0.5 on 'small')


def test_rows_without_data_end_at_the_floor(dev):
    """'mid' stores nothing in column 5 and row 7.  Three iterations of the engine, the last one half-step by half-step: each
    of its two sweeps is checked per element (every row) from the factors before and after it and the Gram matrix the engine
    used, and the rows without data -- whose exact minimiser is the floor -- are within that bound of eps."""
    from torchnmf_amd.wccd import WeightedCcdEngine
    idx, vals, shape, _, _ = _problem('mid')
    omega = OMEGAS[1]
    m, V = _module(dev, 'mid')
    eng = WeightedCcdEngine(V, m.W.data, m.H.data, omega, *REG)
    for _ in range(2):
        eng.w_step()
        eng.h_step()
    f32 = lambda t: t.detach().cpu().numpy()
    for side, step, own, pan, at in (('w', eng.w_step, m.W, m.H, 5), ('h', eng.h_step, m.H, m.W, 7)):
        old, P = f32(own).copy(), f32(pan).copy()
        step()
        got = f32(own)
        G = f32((eng.side_w if side == 'w' else eng.side_h).gram)
        ptr, cols, v = E.side_list(idx, vals, shape, side)
        assert ptr[at + 1] == ptr[at]
        err, bound = E.sweep_check(got, old, P, G, ptr, cols, v.astype(np.float32), omega, *REG)
        frac = E.fraction(err, bound)
        record('wccd_rows_without_data', side=side, worst_fraction_of_bound=float(frac.max()),
               row_max_over_eps=float(got[at].max() / E.EPS))
        assert frac.max() <= 1.0, (side, frac.max())
        want = E.sweep(old[at:at + 1], P, [0, 0], cols[:0], v[:0], float(np.float32(omega)), *np.float32(REG).astype(float), G=G)
        assert (want == E.EPS).all()
        assert (np.abs(got[at].astype(np.float64) - E.EPS) <= bound[at]).all()


def test_bad_target_leaves_the_factors_alone(dev):
    m, V = _module(dev, 'small')
    keep = (m.W.data.clone(), m.H.data.clone())
    bad = torch.sparse_coo_tensor(V.indices(), -V.values(), V.shape).coalesce()
    with pytest.raises(AssertionError, match='non-negative'):
        m.fit(bad, beta=2, solver='ccd', unstored=OMEGA_FIT)
    assert torch.equal(m.W.data, keep[0]) and torch.equal(m.H.data, keep[1])
