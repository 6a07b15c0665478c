"""solver='hals' on the device (csrc/nmfmu_hals.hip, torchnmf_amd/hals.py, the solver branch of ``fit``).

1. The sweep kernel per element, no element left out: the Gauss-Seidel fixed point recomputed in float64 from the device's own
   output under the running-error bound of tests/hals_emulation.py (a float64 sweep of the whole row would compound its error
   by about sum_j |G[j, r]| / G[r, r] per coordinate and bound nothing at rank 128).
2. The bitwise promises: repeatable, a row independent of the rows around it and of the launch size, inputs and storage
   around the outputs untouched.
3. ``fit(solver='hals')`` on the two targets of tests/test_hals_emulation.py, dense and as sparse-COO, against the float64
   emulation of the whole procedure (initial scale included).

Measured on an MI355X: see DESIGN.md section 23.
"""
import functools

import numpy as np
import pytest
import torch

import hals_emulation as E
from conftest import record, rel_err

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257, 1000]          # one partial wave, the wave's edge on both sides, several workgroups
RANKS = [1, 3, 33, 100, 200, 256]          # LDS requests for 32 / 32 / 64 / 128 / 256 / 256
REG = (0.021, 0.049)
GARBAGE = -7.0
TOL = 1e-4                                 # the project's bar for factors
CASES = ['dense', 'sparse']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _run_sweep(dev, F, A, G, lda, reg):
    """The kernel on guarded storage -> (out [rows, rank] numpy).  Asserts that A, G, A's padding and the floats behind F are
    bitwise what they were."""
    from torchnmf_amd.hals import hals_sweep
    rows, rank = F.shape
    fbuf = torch.full((rows * rank + 64,), GARBAGE, device=dev)
    fbuf[:rows * rank] = torch.from_numpy(F).to(dev).reshape(-1)
    Fv = fbuf[:rows * rank].view(rows, rank)
    abuf = torch.full((rows, lda), GARBAGE, device=dev)
    abuf[:, :rank] = torch.from_numpy(A).to(dev)
    Gd = torch.from_numpy(G).to(dev)
    keep_a, keep_g = abuf.clone(), Gd.clone()
    out = hals_sweep(Fv, abuf[:, :rank], Gd, *reg)
    assert out is Fv
    assert torch.equal(abuf, keep_a) and torch.equal(Gd, keep_g)
    assert bool((fbuf[rows * rank:] == GARBAGE).all())
    return Fv.cpu().numpy()


# ---- 1. the sweep, per element -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_per_element(dev, rank):
    from torchnmf_amd import _capi
    r_pad = _capi.load().nmfmu_pad_rank(rank)
    worst = 0.0
    for rows in ROWS:
        F, A, G = E.sweep_case(rows, rank)
        for lda in sorted({rank, r_pad}):
            for reg in ((0.0, 0.0), REG):
                got = _run_sweep(dev, F, A, G, lda, reg)
                assert np.isfinite(got).all() and (got >= np.float32(E.EPS)).all()
                err, bound = E.sweep_check(got, F, A, G, *reg)
                frac = float((err / bound).max())
                worst = max(worst, frac)
                assert frac <= 1.0, (rows, rank, lda, reg, frac, np.unravel_index((err / bound).argmax(), err.shape))
                clamped = got == np.float32(E.EPS)
                assert (got[rows // 2] == np.float32(E.EPS)).all()           # the all-zero row of A ends on the floor
                if rows > 1:
                    assert clamped.any() and (~clamped).any()
    record('hals_sweep_per_element', rank=rank, worst_fraction_of_bound=worst, c=E.bound_c(rank))


# ---- 2. the bitwise promises -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rank', RANKS)
def test_sweep_bitwise(dev, rank):
    F, A, G = E.sweep_case(1000, rank)
    first = _run_sweep(dev, F, A, G, rank, REG)
    again = _run_sweep(dev, F, A, G, rank, REG)
    assert first.tobytes() == again.tobytes()
    padded = _run_sweep(dev, F, A, G, rank + 5, REG)                       # the stride of A is not part of the arithmetic
    assert first.tobytes() == padded.tobytes()
    head = _run_sweep(dev, F[:63].copy(), A[:63].copy(), G, rank, REG)     # 63 rows alone: another grid, a partial wave
    assert head.tobytes() == first[:63].tobytes()
    mid = _run_sweep(dev, F[100:165].copy(), A[100:165].copy(), G, rank, REG)   # rows that sat in other lanes and waves
    assert mid.tobytes() == first[100:165].tobytes()


def test_sweep_argument_checks(dev):
    from torchnmf_amd.hals import hals_sweep
    F, A, G = torch.rand(5, 3, device=dev), torch.rand(5, 3, device=dev), torch.eye(3, device=dev)
    keep = F.clone()
    with pytest.raises(TypeError):
        hals_sweep(F.double(), A, G)
    with pytest.raises(ValueError):
        hals_sweep(F.t(), A.t().contiguous()[:, :5], torch.eye(5, device=dev))    # not contiguous: it cannot be updated in place
    with pytest.raises(ValueError):
        hals_sweep(F, A[:4], G)
    with pytest.raises(ValueError):
        hals_sweep(F, A, torch.eye(4, device=dev))
    with pytest.raises(NotImplementedError):
        hals_sweep(torch.rand(2, 257, device=dev), torch.rand(2, 257, device=dev), torch.eye(257, device=dev))
    assert torch.equal(F, keep)


# ---- 3. fit(solver='hals') -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    return E.fit_case(name)


@functools.lru_cache(maxsize=None)
def _emulated(name, n_iter, tol=-1e300, train_W=True):
    V, W0, H0 = _case(name)
    return E.fit(V, W0, H0, n_iter, tol=tol, train_W=train_W)


def _module(dev, name, **kw):
    from torchnmf_amd.nmf import NMF
    V, W0, H0 = _case(name)
    m = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float(), **kw).to(dev)
    return m, torch.from_numpy(V).float().to(dev)


def _np(t):
    return t.detach().double().cpu().numpy()


@pytest.mark.parametrize('layout', ['dense', 'coo'])
@pytest.mark.parametrize('name', CASES)
def test_one_iteration_against_float64(dev, name, layout):
    m, V = _module(dev, name)
    n = m.fit(V if layout == 'dense' else V.to_sparse(), beta=2, max_iter=1, solver='hals', precision='bf16')
    Wr, Hr, nr = _emulated(name, 1)
    ew, eh = rel_err(m.W.data.cpu(), Wr), rel_err(m.H.data.cpu(), Hr)
    record('hals_fit_one_iteration', target=name, layout=layout, rel_err_W=ew, rel_err_H=eh, tol=TOL)
    assert n == nr == 1 and m.last_precision == 'fp32'
    assert ew < TOL and eh < TOL, (ew, eh)
    assert float(m.W.data.min()) >= E.EPS and float(m.H.data.min()) >= E.EPS


@pytest.mark.parametrize('layout', ['dense', 'coo'])
@pytest.mark.parametrize('name', CASES)
def test_objective_never_increases_and_loss_matches(dev, name, layout):
    """Ten iterations of the engine, the regularised objective evaluated on the host in float64 from the device's factors after
    every half-step: non-increasing within 1e-5 of the objective (the emulation gains more than 1e-3 per iteration there).  The
    engine's own loss at the end against metrics.beta_div of the reconstruction: 1e-4 relative (the residual on these targets
    is above a tenth of 1/2 |V|^2, so the cancellation in the Gram form costs one digit at most)."""
    from torchnmf_amd.hals import HalsEngine
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    for reg in ((0.0, 0.0), REG):
        m, V = _module(dev, name)
        Vn = _case(name)[0]
        eng = HalsEngine(V if layout == 'dense' else V.to_sparse(), m.W.data, m.H.data, *reg)
        assert eng.target_flags() == (False, bool((Vn == 0).any()))
        trace = [None]
        eng.divergence()                          # (the initial scale happens here, as in fit's loss_init)
        trace[0] = E.objective(Vn, _np(m.W), _np(m.H), *reg)
        for _ in range(10):
            eng.w_step()
            trace.append(E.objective(Vn, _np(m.W), _np(m.H), *reg))
            eng.h_step()
            trace.append(E.objective(Vn, _np(m.W), _np(m.H), *reg))
        trace = np.array(trace)
        worst_rise = float((np.diff(trace) / trace[:-1]).max())
        assert worst_rise <= 1e-5, worst_rise
        loss = eng.divergence()
        ref = float(beta_div(NMF.reconstruct(m.H.data, m.W.data), V, 2))
        host = E.divergence(Vn, _np(m.W), _np(m.H))
        record('hals_objective_and_loss', target=name, layout=layout, reg=list(reg), worst_relative_rise=worst_rise,
               loss_vs_beta_div=abs(loss - ref) / ref, loss_vs_float64=abs(loss - host) / host,
               residual_over_half_v2=host / (0.5 * float((Vn ** 2).sum())))
        assert host > 0.1 * 0.5 * float((Vn ** 2).sum())               # (the premise of the tolerance)
        assert abs(loss - ref) <= 1e-4 * ref, (loss, ref)


@pytest.mark.parametrize('layout', ['dense', 'coo'])
@pytest.mark.parametrize('name', CASES)
def test_hals_20_beats_mu_40(dev, name, layout):
    m, V = _module(dev, name)
    Vt = V if layout == 'dense' else V.to_sparse()
    start = {k: v.clone() for k, v in m.state_dict().items()}
    Vn = _case(name)[0]
    assert m.fit(Vt, beta=2, tol=-1e9, max_iter=20, solver='hals') == 20
    h = E.divergence(Vn, _np(m.W), _np(m.H))
    m.load_state_dict(start)
    assert m.fit(Vt, beta=2, tol=-1e9, max_iter=40, solver='mu', precision='bf16x3') == 40
    mu = E.divergence(Vn, _np(m.W), _np(m.H))
    Wr, Hr, _ = _emulated(name, 20)
    record('hals_20_vs_mu_40', target=name, layout=layout, hals=h, mu=mu, emulated_hals=E.divergence(Vn, Wr, Hr))
    assert h < mu, (h, mu)


@pytest.mark.parametrize('name', CASES)
def test_dense_and_sparse_fits_agree(dev, name):
    m, V = _module(dev, name)
    m2, _ = _module(dev, name)
    assert m.fit(V, beta=2, tol=-1e9, max_iter=5, solver='hals', alpha=0.07, l1_ratio=0.3) == 5
    assert m2.fit(V.to_sparse(), beta=2, tol=-1e9, max_iter=5, solver='hals', alpha=0.07, l1_ratio=0.3) == 5
    ew, eh = rel_err(m2.W.data.cpu(), m.W.data.cpu()), rel_err(m2.H.data.cpu(), m.H.data.cpu())
    record('hals_dense_vs_sparse', target=name, rel_err_W=ew, rel_err_H=eh, tol=TOL)
    assert ew < TOL and eh < TOL, (ew, eh)


@pytest.mark.parametrize('layout', ['dense', 'coo'])
@pytest.mark.parametrize('name', CASES)
def test_stop_rule(dev, name, layout):
    """tol = 1e-2 stops the emulation at 30 (dense target: the ratios at the checkpoints are 0.278, 0.0147, 0.0056) and at 20
    (5 %-dense target: 0.274, 0.0086): every decision has a margin of 14 % or more."""
    m, V = _module(dev, name)
    want = _emulated(name, 200, 1e-2)[2]
    assert want == (30 if name == 'dense' else 20)
    assert m.fit(V if layout == 'dense' else V.to_sparse(), beta=2, tol=1e-2, max_iter=200, solver='hals') == want


@pytest.mark.parametrize('layout', ['dense', 'coo'])
def test_frozen_W(dev, layout):
    m, V = _module(dev, 'dense', trainable_W=False)
    keep = m.W.data.clone()
    assert m.fit(V if layout == 'dense' else V.to_sparse(), beta=2, tol=-1e9, max_iter=3, solver='hals') == 3
    assert torch.equal(m.W.data, keep) and not m.W.requires_grad
    Wr, Hr, _ = _emulated('dense', 3, train_W=False)
    eh = rel_err(m.H.data.cpu(), Hr)
    record('hals_frozen_W', layout=layout, rel_err_H=eh, tol=TOL)
    assert eh < TOL, eh


def test_double_module_keeps_its_dtype(dev):
    m, V = _module(dev, 'dense')
    m = m.double()
    assert m.fit(V, beta=2, tol=-1e9, max_iter=2, solver='hals') == 2
    assert m.W.dtype == torch.float64 and m.H.dtype == torch.float64 and m.last_precision == 'fp32'
    Wr, Hr, _ = _emulated('dense', 2)
    assert rel_err(m.W.data.cpu(), Wr) < TOL and rel_err(m.H.data.cpu(), Hr) < TOL


def test_bad_target_leaves_the_factors_alone(dev):
    m, V = _module(dev, 'dense')
    keep = (m.W.data.clone(), m.H.data.clone())
    V = V.clone()
    V[3, 4] = -1.0
    with pytest.raises(AssertionError, match='non-negative'):
        m.fit(V, beta=2, solver='hals')
    assert torch.equal(m.W.data, keep[0]) and torch.equal(m.H.data, keep[1])
