"""solver='ccd' on the device (csrc/nmfmu_sparse_ccd.hip, torchnmf_amd/ccd.py, the solver branch of ``fit``).

1. The sweep kernel per element, no element left out: the coordinate fixed point recomputed in float64 from the device's own
   output under the running-error bound of tests/ccd_emulation.py, on both sides, with row counts on either side of a wave's
   64 entries and of the register residency limit, stored zeros, an all-zero row and rows without entries.
2. The bitwise promises: repeatable; a row independent of the other rows of the call, of the order list, of where its
   residuals live (registers or scratch) and of where it fetches the panel from (LDS stage, transposed copy, the panel) --
   on the one-wave path and on the workgroup path.
3. ``fit(solver='ccd', unstored='missing')`` against the float64 emulation of the whole procedure (initial scale included), a
   fully stored target against ``solver='hals'``, and ten iterations against the masked multiplicative update.

Measured on an MI355X: see DESIGN.md section 26.
"""
import functools

import numpy as np
import pytest
import torch

import ccd_emulation as E
from conftest import record, rel_err

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 33, 64, 100, 256]
SIDES = ['h', 'w']
N_PANEL = 600
BASE = (0, 1, 63, 64, 65, 129)             # nothing, one lane, a wave's edge on both sides, three slots with a tail
EDGE = (E.LIMIT - 1, E.LIMIT, E.LIMIT + 1)   # the residency limit of a wave, which is also the default workgroup threshold:
                                           # the last one-wave rows and the first row that takes a workgroup
WG_LOW = 100                               # a lowered workgroup threshold: the rows of 129 entries and more take a workgroup
REG = (0.021, 0.049)
GARBAGE = -7.0
TOL = 1e-4                                 # the project's bar for factors


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


def _run_sweep(dev, case, side, reg, **kw):
    """The kernel on guarded storage -> out [rows, rank] numpy.  Asserts that the panel, the index and value arrays and the
    floats behind F are bitwise what they were."""
    from torchnmf_amd.ccd import ccd_sweep
    from torchnmf_amd.sparse_autograd import SparseTarget
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
    keep = [t.clone() for t in (Pd, tp, ti, tv)]
    out = ccd_sweep(Fv, Pd, T, side, *reg, **kw)
    assert out is Fv
    for t, k in zip((Pd, tp, ti, tv), keep):
        assert torch.equal(t, k)
    assert bool((fbuf[rows * rank:] == GARBAGE).all())
    return Fv.cpu().numpy()


# ---- 1. the sweep, per element -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_per_element(dev, rank, side):
    worst = 0.0
    eps32 = np.float32(E.EPS)
    for rows in (1, 5, 257):
        case = _case(rows, rank)
        F, P, ptr, cols, vals = case
        counts = np.diff(ptr)
        assert (vals == 0).any()
        for reg, wg in (((0.0, 0.0), 0), (REG, 0), (REG, WG_LOW)):
            got = _run_sweep(dev, case, side, reg, _wg_rows=wg)
            assert np.isfinite(got).all() and (got >= eps32).all()
            err, bound = E.sweep_check(got, F, P, ptr, cols, vals, *reg, wg_rows=wg or E.LIMIT)
            frac = E.fraction(err, bound)
            worst = max(worst, float(frac.max()))
            assert frac.max() <= 1.0, (rows, rank, side, reg, wg, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
            for i in np.nonzero(counts == 0)[0]:
                assert got[i].tobytes() == F[i].tobytes()                  # a row without data is not touched
            z = E.zero_row(counts)
            assert (z is None) == (rows == 1)
            if z is not None:
                assert (vals[ptr[z]:ptr[z + 1]] == 0).all() and (got[z] == eps32).all()    # the all-zero row ends on the floor
            if rows == 257:                     # (the data's premise: both sides of the clamp are exercised at every rank)
                rest = np.delete(got, z, axis=0)[np.delete(counts, z) > 0]
                assert (rest == eps32).any() and (rest != eps32).any()
    record('ccd_sweep_per_element', rank=rank, side=side, worst_fraction_of_bound=worst,
           c_res_max=E.bound_terms(rank, rank - 1, E.LIMIT + 1)[0], c_sum_max=E.bound_terms(rank, 0, E.LIMIT + 1)[1])


# ---- 2. the bitwise promises -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_bitwise(dev, rank, side):
    from torchnmf_amd import ccd
    case = _case(257, rank)
    F, P, ptr, cols, vals = case
    counts = np.diff(ptr)
    cap = ccd.lds_rows(rank)
    assert ((counts <= cap) & (counts > 0)).any() and ((counts > cap).any() or rank < 33)
    pick = [102, 3, 101, 4, 100, 5, 0, 256]       # the rows around the limit and a few short ones
    sptr = np.zeros(len(pick) + 1, dtype=np.int64)
    sptr[1:] = np.cumsum(counts[pick])
    scols = np.concatenate([cols[ptr[i]:ptr[i + 1]] for i in pick])
    svals = np.concatenate([vals[ptr[i]:ptr[i + 1]] for i in pick])
    firsts = []
    for wg in (0, WG_LOW):                        # (a row's path is a function of its count and this threshold)
        first = _run_sweep(dev, case, side, REG, _wg_rows=wg)
        firsts.append(first)
        assert _run_sweep(dev, case, side, REG, _wg_rows=wg).tobytes() == first.tobytes()          # repeatable
        # the order list: reversed (shortest first) and a fixed shuffle
        for order in (np.argsort(counts, kind='stable'), np.random.default_rng(5).permutation(257)):
            got = _run_sweep(dev, case, side, REG, _wg_rows=wg, _order=torch.from_numpy(order.astype(np.int32)).to(dev))
            assert got.tobytes() == first.tobytes()
        # where the residuals live: with `limit` entries per wave in registers, the longer rows go through the scratch buffer
        # (limit 8: every one-wave row above 8 entries and every workgroup row above 128)
        for limit in (8, 64, 128, E.LIMIT - 1):
            assert _run_sweep(dev, case, side, REG, _wg_rows=wg, _limit=limit).tobytes() == first.tobytes(), limit
        # where the panel comes from; 'lds' stages the one-wave rows that fit (the cap depends on the rank)
        for layout in ('lds', 'transposed', 'direct'):
            assert _run_sweep(dev, case, side, REG, _wg_rows=wg, _layout=layout).tobytes() == first.tobytes(), layout
            assert _run_sweep(dev, case, side, REG, _wg_rows=wg, _layout=layout, _limit=8).tobytes() == first.tobytes(), layout
        # a subset of the rows alone, in another call and other workgroups
        sub = _run_sweep(dev, (F[pick].copy(), P, sptr, scols, svals), side, REG, _wg_rows=wg)
        assert sub.tobytes() == first[pick].tobytes()
    short = counts <= WG_LOW                      # rows on the same path under both thresholds have the same bits
    assert firsts[0][short].tobytes() == firsts[1][short].tobytes()


def test_sweep_argument_checks(dev):
    from torchnmf_amd.ccd import ccd_sweep
    V = torch.sparse_coo_tensor(torch.tensor([[0, 1, 4], [2, 3, 0]]), torch.tensor([1.0, 0.5, 2.0]), (5, 4)).to(dev)
    F, P = torch.rand(5, 3, device=dev), torch.rand(4, 3, device=dev)
    keep = F.clone()
    with pytest.raises(TypeError):
        ccd_sweep(F.double(), P, V, 'h')
    with pytest.raises(TypeError):
        ccd_sweep(F, P.double(), V, 'h')
    with pytest.raises(ValueError):
        ccd_sweep(F.t(), P, V, 'h')                       # not contiguous: it cannot be updated in place
    with pytest.raises(ValueError):
        ccd_sweep(F, P, V, 'w')                           # the shapes of the other side
    with pytest.raises(ValueError):
        ccd_sweep(F, P[:3], V, 'h')
    with pytest.raises(ValueError):
        ccd_sweep(F, P, V.to_dense(), 'h')
    with pytest.raises(ValueError):
        ccd_sweep(F, P, V, 'h', _limit=E.LIMIT + 1)
    with pytest.raises(NotImplementedError):
        ccd_sweep(torch.rand(5, 257, device=dev), torch.rand(4, 257, device=dev), V, 'h')
    assert torch.equal(F, keep)
    assert ccd_sweep(P.clone(), F, V, 'w').shape == (4, 3)


# ---- 3. fit(solver='ccd') ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(name):
    return E.fit_case(name)


@functools.lru_cache(maxsize=None)
def _emulated(name, n_iter, tol=-1e300, reg=(0.0, 0.0), train_W=True):
    idx, vals, shape, W0, H0 = _problem(name)
    return E.fit(idx, vals, shape, W0, H0, n_iter, tol=tol, l1=reg[0], l2=reg[1], train_W=train_W)


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
    """'small': tol = 1e-2 stops the emulation at 30 (the ratios at the checkpoints are 0.92, 0.024, 0.0079 without
    regularisation, 0.92, 0.021, 0.0091 with: every decision has a margin of 9 % or more, against a drift of the fp32
    factors of about 1e-6); 'mid': ten iterations."""
    m, V = _module(dev, name)
    kw = dict(ALPHA) if reg else {}
    r = REG if reg else (0.0, 0.0)
    if name == 'small':
        Wr, Hr, nr = _emulated(name, 200, 1e-2, r)
        n = m.fit(V, beta=2, tol=1e-2, max_iter=200, solver='ccd', unstored='missing', precision='bf16', **kw)
    else:
        Wr, Hr, nr = _emulated(name, 10, -1e300, r)
        n = m.fit(V, beta=2, tol=-1e9, max_iter=10, solver='ccd', unstored='missing', **kw)
    ew, eh = rel_err(m.W.data.cpu(), Wr), rel_err(m.H.data.cpu(), Hr)
    record('ccd_fit_vs_float64', problem=name, reg=reg, n_iter=n, emulated_n_iter=nr, rel_err_W=ew, rel_err_H=eh, tol=TOL)
    assert n == nr and m.last_precision == 'fp32'
    assert ew < TOL and eh < TOL, (ew, eh)
    assert float(m.W.data.min()) >= E.EPS and float(m.H.data.min()) >= E.EPS


def test_frozen_W(dev):
    m, V = _module(dev, 'mid', trainable_W=False)
    keep = m.W.data.clone()
    assert m.fit(V, beta=2, tol=-1e9, max_iter=3, solver='ccd', unstored='missing') == 3
    assert torch.equal(m.W.data, keep) and not m.W.requires_grad
    Wr, Hr, _ = _emulated('mid', 3, train_W=False)
    eh = rel_err(m.H.data.cpu(), Hr)
    record('ccd_frozen_W', rel_err_H=eh, tol=TOL)
    assert eh < TOL, eh


def test_double_module_keeps_its_dtype(dev):
    m, V = _module(dev, 'small')
    m = m.double()
    assert m.fit(V, beta=2, tol=-1e9, max_iter=2, solver='ccd', unstored='missing') == 2
    assert m.W.dtype == torch.float64 and m.H.dtype == torch.float64 and m.last_precision == 'fp32'
    Wr, Hr, _ = _emulated('small', 2)
    assert rel_err(m.W.data.cpu(), Wr) < TOL and rel_err(m.H.data.cpu(), Hr) < TOL


@pytest.mark.parametrize('name', ['small', 'mid'])
def test_loss_sequence_never_increases(dev, name):
    """Ten iterations of the engine.  Without regularisation the engine's own loss after every half-step: non-increasing within
    1e-5 of the loss (each evaluation rounds every entry's term in fp32, about 1e-6 relative, so two of them may differ by
    2e-6 without any rise).  With regularisation the objective the sweeps descend on, evaluated on the host in float64 from
    the device's factors, under the same bar.  The engine's loss against the float64 loss of its factors: 1e-5."""
    from torchnmf_amd.ccd import CcdEngine
    idx, vals, shape, _, _ = _problem(name)
    for reg in ((0.0, 0.0), REG):
        m, V = _module(dev, name)
        eng = CcdEngine(V, m.W.data, m.H.data, *reg)
        assert eng.target_flags() == (False, bool((vals == 0).any()))
        seq, trace = [eng.divergence()], []                  # (the initial scale happens here, as in fit's loss_init)
        trace.append(E.objective(idx, vals, _np(m.W), _np(m.H), *reg))
        for _ in range(10):
            for step in (eng.w_step, eng.h_step):
                step()
                seq.append(eng.divergence())
                trace.append(E.objective(idx, vals, _np(m.W), _np(m.H), *reg))
        seq, trace = np.array(seq), np.array(trace)
        rise = float((np.diff(trace) / trace[:-1]).max())
        rise_own = float((np.diff(seq) / seq[:-1]).max())
        host = E.divergence(idx, vals, _np(m.W), _np(m.H))
        record('ccd_loss_sequence', problem=name, reg=list(reg), worst_relative_rise_objective=rise,
               worst_relative_rise_own_loss=rise_own, loss_vs_float64=abs(seq[-1] - host) / host)
        assert rise <= 1e-5, rise
        if reg == (0.0, 0.0):
            assert rise_own <= 1e-5, rise_own
        assert abs(seq[-1] - host) <= 1e-5 * host, (seq[-1], host)
        assert seq[-1] < 0.5 * seq[0]


def test_fully_stored_target_agrees_with_hals(dev):
    """Every entry stored: the quadratic of each row is the Gram form and solver='hals' on the dense V is the same procedure
    (tests/test_ccd_emulation.py holds the two float64 emulations to 1e-6 at E.FULL_ITERS iterations)."""
    from torchnmf_amd.nmf import NMF
    idx, vals, shape, Vd, W0, H0 = E.full_case()
    fits = []
    for solver in ('ccd', 'hals'):
        m = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float()).to(dev)
        V = torch.from_numpy(Vd).float().to(dev)
        if solver == 'ccd':
            V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals).float(), shape).coalesce().to(dev)
            assert V._nnz() == shape[0] * shape[1]
        kw = dict(unstored='missing') if solver == 'ccd' else {}
        assert m.fit(V, beta=2, tol=-1e9, max_iter=E.FULL_ITERS, solver=solver, **kw, **ALPHA) == E.FULL_ITERS
        fits.append((m.W.data.cpu(), m.H.data.cpu()))
    ew, eh = rel_err(fits[0][0], fits[1][0]), rel_err(fits[0][1], fits[1][1])
    record('ccd_vs_hals_fully_stored', rel_err_W=ew, rel_err_H=eh, tol=TOL)
    assert ew < TOL and eh < TOL, (ew, eh)


def test_ccd_10_beats_masked_mu_10(dev):
    """From the same factors (the scaled start), ten iterations each: tests/test_ccd_emulation.py shows the float64 emulations
    apart by more than 20 % of MU's loss on this problem."""
    from torchnmf_amd.ccd import CcdEngine
    from torchnmf_amd.sparse_engine import MaskedMU
    idx, vals, shape, _, _ = _problem('mid')
    m, V = _module(dev, 'mid')
    eng = CcdEngine(V, m.W.data, m.H.data)
    eng.divergence()
    W2, H2 = m.W.data.clone(), m.H.data.clone()
    mu = MaskedMU(V, W2, H2, 2.0)
    for e in (eng, mu):
        for _ in range(10):
            e.w_step()
            e.h_step()
    c, u = eng.divergence(), mu.divergence()
    record('ccd_10_vs_masked_mu_10', ccd=c, mu=u, host_ccd=E.divergence(idx, vals, _np(m.W), _np(m.H)),
           host_mu=E.divergence(idx, vals, _np(W2), _np(H2)))
    assert c < u, (c, u)


def test_bad_target_leaves_the_factors_alone(dev):
    m, V = _module(dev, 'small')
    keep = (m.W.data.clone(), m.H.data.clone())
    bad = torch.sparse_coo_tensor(V.indices(), -V.values(), V.shape).coalesce()
    with pytest.raises(AssertionError, match='non-negative'):
        m.fit(bad, beta=2, solver='ccd', unstored='missing')
    assert torch.equal(m.W.data, keep[0]) and torch.equal(m.H.data, keep[1])
