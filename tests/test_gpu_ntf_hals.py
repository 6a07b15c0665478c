"""HALS for 3-way tensors on the device: ``ntf_mttkrp`` per element against float64 numpy at the shapes where its two walks,
the flat stages, the load widths, the two wave arrangements and the split can go wrong, then ``NTF.fit(solver='hals')`` against
the chain of its public pieces, its objective in float64 and MU.

Bound of the MTTKRP (derived in test_gpu_ntf, not measured): every summand is non-negative, so whatever the order of the sum
the relative error is at most ``(R + L + 64) 2^-24`` with ``L`` the mode's contraction length; asserted with a factor 2."""
import functools

import numpy as np
import pytest
import torch

from conftest import record
from test_gpu_ntf import U, dev, host, planted, problem
from torchnmf_amd import _capi, hals, ntf
from torchnmf_amd.constants import eps

pytestmark = pytest.mark.gpu
SHAPES = [(131, 6, 11), (5, 132, 36), (7, 70, 2), (3, 5, 131), (33, 6, 11)]


@functools.lru_cache(maxsize=None)
def reference(shape, R):
    """The three MTTKRPs of ``problem(shape, R)`` in float64."""
    fs, V = problem(shape, R)[:2]
    f64 = [f.astype(np.float64) for f in fs]
    return [np.einsum('oab,ar,br->or', np.moveaxis(V.astype(np.float64), n, 0), *(f for m, f in enumerate(f64) if m != n))
            for n in range(3)]


@pytest.mark.parametrize('mode', (0, 1, 2))
@pytest.mark.parametrize('nsplit', (1, 3))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', SHAPES)
def test_mttkrp_against_float64(shape, R, nsplit, mode):
    fs, V = problem(shape, R)[:2]
    T, dfs, ref = ntf.NtfTarget(dev(V)), [dev(f) for f in fs], reference(shape, R)[mode]
    bound = 2 * (R + V.size // shape[mode] + 64) * U
    got, worst = {}, {}
    for tile in ('wide', 'short'):
        g = ntf._mttkrp_call(T, dfs, mode, nsplit=nsplit, tile=tile, _fill=float('nan'))
        again = ntf._mttkrp_call(T, dfs, mode, nsplit=nsplit, tile=tile, _fill=7.0)
        assert torch.equal(g, again), 'a repeated call is bitwise identical whatever the workspace and the output held'
        g = host(g)
        assert g.shape == (shape[mode], _capi.load().nmfmu_pad_rank(R)) and (g[:, R:] == 0).all(), 'padded rank columns'
        got[tile] = g[:, :R]
        worst[tile] = float((np.abs(got[tile] - ref) / (bound * ref)).max())
        assert worst[tile] <= 1, (tile, worst[tile])
    assert (np.abs(got['wide'] - got['short']) <= 2 * bound * ref).all()
    record('ntf_mttkrp', shape=shape, R=R, nsplit=nsplit, mode=mode, **worst)


def masked(V):
    """``V`` with half of its entries zeroed: the dense statement of the sparse 'zero' target ``dev(masked(V)).to_sparse()``."""
    return V * (np.random.default_rng(11).random(V.shape) < 0.5)


def loss64(V, factors):
    return 0.5 * float(((V.astype(np.float64) - np.einsum('ir,jr,kr->ijk', *[host(f) for f in factors])) ** 2).sum())


def target(sparse):
    """(the fit's target, the keywords that go with it, its dense float64 statement, the start)."""
    V, _, start = planted(False)
    if not sparse:
        return dev(V), {}, V, start
    return dev(masked(V)).to_sparse(), {'unstored': 'zero'}, masked(V), start


@pytest.mark.parametrize('case', ('dense', 'frozen', 'sparse'))
def test_one_iteration_is_the_chain_of_public_pieces(case):
    Vd, kw, _, start = target(case == 'sparse')
    train = (True, False, True) if case == 'frozen' else (True, True, True)
    alpha, l1_ratio = 0.07, 0.3
    m = ntf.NTF(factors=[torch.from_numpy(s) for s in start], trainable=train).cuda()
    assert m.fit(Vd, beta=2, tol=-1e9, max_iter=1, solver='hals', alpha=alpha, l1_ratio=l1_ratio, **kw) == 1
    fs, lib, R = [dev(s) for s in start], _capi.load(), start[0].shape[1]
    if case == 'sparse':
        Ts = ntf.SparseNtfTarget(Vd)
        numerator = lambda n: ntf.sparse_ntf_terms(Ts, fs, n, 2, 'zero')[0]      # noqa: E731
    else:
        numerator = lambda n: ntf.ntf_mttkrp(Vd, fs, n)      # noqa: E731
    g = [ntf._gram(lib, f).double() for f in fs]
    a = float((numerator(0)[:, :R].double() * fs[0].double()).sum().item()) / float((g[0] * g[1] * g[2]).sum().item())
    assert a > 0
    for f, on in zip(fs, train):
        if on:
            f.mul_(a ** (1.0 / sum(train))).clamp_(min=eps)
    for n in range(3):
        if train[n]:
            pa, pb = (f for k, f in enumerate(fs) if k != n)
            hals.hals_sweep(fs[n], numerator(n), (ntf._gram(lib, pa) * ntf._gram(lib, pb)).view(R, R), alpha * l1_ratio,
                            alpha * (1 - l1_ratio))
    assert all(torch.equal(f.data, c) for f, c in zip(m.factors, fs))
    assert case != 'frozen' or torch.equal(m.factors[1].data, dev(start[1])), 'the frozen factor keeps its bits'


@pytest.mark.parametrize('sparse', (False, True))
def test_objective_never_increases_and_loss_matches(sparse):
    """Ten iterations, one ``fit`` each, the float64 loss on the host after each: it never rises by more than 1e-5 relative.
    The loss ``fit`` tracks against float64 within 1e-4 where the residual exceeds a tenth of 1/2 |V|^2 (asserted): at the scaled
    start (no half-step yet: the numerator of mode 0) and after the half-step of mode 0 alone (the numerator of that half-step).
    In float64 the residual at the two points is 0.55 and 0.34 of 1/2 |V|^2 on the dense target (0.77 and 0.67 on the sparse
    one); a whole iteration brings the dense one to 0.056, below the premise."""
    Vd, kw, Vn, start = target(sparse)
    m = ntf.NTF(factors=[torch.from_numpy(s) for s in start]).cuda()
    trace = []
    for _ in range(10):
        assert m.fit(Vd, beta=2, tol=-1e9, max_iter=1, solver='hals', **kw) == 1
        trace.append(loss64(Vn, [f.data for f in m.factors]))
    worst_rise = float((np.diff(trace) / np.array(trace[:-1])).max())
    assert worst_rise <= 1e-5, trace
    fs = [dev(s) for s in start]
    eng = ntf._HalsNtf(ntf.SparseNtfTarget(Vd) if sparse else ntf.NtfTarget(Vd), fs, (True, True, True), 0.0, 0.0)
    half_v2, errs = 0.5 * float((Vn.astype(np.float64) ** 2).sum()), []
    for half_step in (None, 0):
        if half_step is not None:
            eng.half_step(half_step)
        got, ref = eng.divergence(), loss64(Vn, fs)
        assert ref > 0.1 * half_v2, 'the premise of the tolerance'
        errs.append(abs(got - ref) / ref)
        assert errs[-1] <= 1e-4, (got, ref)
    record('ntf_hals_objective', sparse=sparse, worst_relative_rise=worst_rise, loss_vs_float64=errs)


@pytest.mark.parametrize('sparse', (False, True))
def test_hals_20_beats_mu_40(sparse):
    Vd, kw, Vn, start = target(sparse)
    out = {}
    for solver, iters in (('hals', 20), ('mu', 40)):
        m = ntf.NTF(factors=[torch.from_numpy(s) for s in start]).cuda()
        assert m.fit(Vd, beta=2, tol=-1e9, max_iter=iters, solver=solver, **kw) == iters
        out[solver] = loss64(Vn, [f.data for f in m.factors])
    record('ntf_hals_20_vs_mu_40', sparse=sparse, **out)
    assert out['hals'] < out['mu'], out


def test_unchanged_paths():
    V, _, start = planted(False)
    out = []
    for kw in ({}, {'solver': 'mu'}):
        m = ntf.NTF(factors=[torch.from_numpy(s) for s in start]).cuda()
        assert m.fit(dev(V), beta=2, tol=-1e9, max_iter=3, **kw) == 3
        out.append([f.data for f in m.factors])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    m = ntf.NTF(factors=[torch.from_numpy(s) for s in start]).double().cuda()
    assert m.fit(dev(V), beta=2, tol=-1e9, max_iter=2, solver='hals') == 2
    assert all(f.dtype == torch.float64 and bool(torch.isfinite(f).all()) for f in m.factors)
