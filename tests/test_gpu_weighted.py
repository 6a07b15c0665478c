"""Weighted NMF on the device (csrc/nmfmu_wmu.hip, wmu.WeightedMU, ``fit(V, weights=M)``, ``metrics.weighted_beta_div``):
terms, step and loss per element against the float64 reference under the bounds derived in tests/weighted_emulation.py (no
element left out), indifference to what V holds where the weight is 0, the reference's recorded runs (golden g23), agreement
with the dense and the missing-data paths, reproducibility, a monotone loss and autograd.

The per-element targets: 131 x 70 (one full row tile plus 3 rows, two full stages plus 6 columns, rows not 16-byte aligned:
the scalar loads; the W side sees 70 owner rows over 4 stages plus 3) and 132 x 72 (aligned: the 16-byte loads, tails of 4 and
8).  The split count is forced to 1, 2 and 3: a part boundary, a short last part and a part that holds only the tail, on both
sides.  Weights real in [0.25, 4) with about 30 % exact zeros, one weightless row and one weightless column; V holds NaN,
Inf, -1 or 1000 wherever the weight is 0.

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 30.
"""
import functools

import numpy as np
import pytest
import torch

import weighted_emulation as WE
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(131, 70), (132, 72)]
RANKS = [3, 33, 100, 200]             # r_pad 32 / 64 / 128 / 256 (the last: two rank tiles)
BETAS = [-1, 0, 0.5, 1, 2, 3]
SPLITS = [1, 2, 3]
REG = (0.07 * 0.3, 0.07 * 0.7)
TOL = 1e-4                            # the project's bar for factors after a recorded run
UP = -1.75                            # the incoming gradient of the autograd tests: signed, not 1, exact in fp32
NAN = float('nan')
DEAD_ROW, DEAD_COL = 5, 3             # weighted_emulation.make_problem


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(N, C, R):
    return WE.make_problem(N, C, R)


def _target(V, M, dev):
    from torchnmf_amd.metrics import WeightedTarget
    return WeightedTarget(torch.from_numpy(V).to(dev), torch.from_numpy(M).to(dev))


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (name, info)
    err = WE.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


# ---- per element against the float64 reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('nsplit', SPLITS)
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('shape', SHAPES)
def test_terms_step_loss_per_element(dev, shape, beta, R, nsplit):
    from torchnmf_amd import _capi
    from torchnmf_amd import wmu
    N, C = shape
    lib = _capi.load()
    r_pad = lib.nmfmu_pad_rank(R)
    V, M, W0, H0 = _problem(N, C, R)
    info = dict(shape=f'{N}x{C}', beta=beta, R=R, nsplit=nsplit)
    T = _target(V, M, dev)
    assert (T.V.data_ptr() % 16 == 0) and ((C % 4 == 0) == (shape == (132, 72)))      # which load path runs
    assert (T.bad, T.has_zero) == (False, False)                       # the junk lies under zero weights only
    Hd, Wd = torch.from_numpy(H0).to(dev), torch.from_numpy(W0).to(dev)
    for side, owner, panel, dead in (('h', Hd, Wd, DEAD_ROW), ('w', Wd, Hd, DEAD_COL)):
        rows, contraction = (N, C) if side == 'h' else (C, N)
        assert lib.nmfmu_wmu_ws(rows, contraction, r_pad, nsplit) == WE.workspace_floats(rows, contraction, r_pad, nsplit)
        # terms: every element of both planes is written (they and the workspace start as NaN), padded columns exactly 0
        ref = WE.terms(V, M, H0, W0, beta, side, nsplit)
        assert ref['parts'] == nsplit
        num, den = wmu._wmu_call(T, side, owner, panel, float(beta), nsplit=nsplit, _fill=NAN)
        assert num.shape == den.shape == (rows, r_pad)
        assert bool((num[:, R:] == 0).all()) and bool((den[:, R:] == 0).all())
        _check('weighted_terms_num', num[:, :R], ref['num'], ref['num_bound'], side=side, **info)
        _check('weighted_terms_den', den[:, :R], ref['den'], ref['den_bound'], side=side, **info)
        assert bool((num[dead] == 0).all()) and bool((den[dead] == 0).all())
        # step, without and with regularisers, on a copy of the owner
        for l1, l2 in ((0.0, 0.0), REG):
            new_ref, bound, _ = WE.step(V, M, H0, W0, beta, side, l1, l2, nsplit)
            f = owner.clone()
            before = panel.clone()
            wmu._wmu_call(T, side, f, panel, float(beta), step=(l1, l2, WE.gamma_of(beta)), nsplit=nsplit, _fill=NAN)
            _check('weighted_step', f, new_ref, bound, side=side, reg=l1 > 0, **info)
            assert torch.equal(panel, before)
            if l1 == 0:
                assert torch.equal(f[dead], owner[dead])                # nothing weighted there: bitwise unchanged
    ref_loss, loss_bound = WE.loss(V, M, H0, W0, beta)
    part = torch.full((lib.nmfmu_wmu_loss_parts(N, C),), NAN, dtype=torch.float64, device=dev)
    got = wmu._wmu_loss(Hd, Wd, T, float(beta), part=part)
    assert got.dtype == torch.float64 and lib.nmfmu_wmu_loss_parts(N, C) == WE.loss_parts(N, C)
    _check('weighted_loss', got.reshape(()), ref_loss, loss_bound, **info)


# ---- indifference to what lies under a zero weight ---------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0, 0.5, 1, 2])
def test_weightless_entries_are_ignored(dev, beta):
    """Two targets equal wherever m > 0; one holds NaN, Inf, -1 and 1000 at the weightless positions, the other zeros."""
    from torchnmf_amd.nmf import NMF
    V, M, W0, H0 = _problem(131, 70, 33)
    Vz = np.where(M > 0, V, 0.0).astype(np.float32)
    assert np.isnan(V).any() and np.isinf(V).any() and (V == -1).any() and (V == 1000).any() and (Vz == 0).any()
    Md = torch.from_numpy(M).to(dev)
    fits = []
    for target in (V, Vz):
        m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
        assert m.fit(torch.from_numpy(target).to(dev), beta=beta, tol=-1e9, max_iter=10, weights=Md) == 10
        assert m.last_precision == 'fp32'
        fits.append((m.W.data.clone(), m.H.data.clone()))
    assert torch.equal(fits[0][0], fits[1][0]) and torch.equal(fits[0][1], fits[1][1])
    assert bool(torch.isfinite(fits[0][0]).all()) and bool(torch.isfinite(fits[0][1]).all())
    assert not torch.equal(fits[0][0], torch.from_numpy(W0).to(dev))


def test_beta_zero_looks_at_weighted_entries_only(dev):
    from torchnmf_amd.metrics import weighted_beta_div
    from torchnmf_amd.nmf import NMF
    V, M, W0, H0 = _problem(131, 70, 3)
    Vz = np.where(M > 0, V, 0.0).astype(np.float32)                 # zeros, but only where nothing is weighted
    Md = torch.from_numpy(M).to(dev)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    assert m.fit(torch.from_numpy(Vz).to(dev), beta=0, tol=-1e9, max_iter=3, weights=Md) == 3
    assert bool(torch.isfinite(m.H.data).all())
    i, j = np.argwhere(M > 0)[7]
    Vz[i, j] = 0.0                                                  # a weighted zero: the reference's refusal
    for beta in (0, -1):
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            m.fit(torch.from_numpy(Vz).to(dev), beta=beta, max_iter=2, weights=Md)
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            weighted_beta_div(m.H, m.W, torch.from_numpy(Vz).to(dev), Md, beta)
    assert m.fit(torch.from_numpy(Vz).to(dev), beta=1, tol=-1e9, max_iter=2, weights=Md) == 2     # data for beta > 0
    Vz[i, j] = -0.5                                                 # a weighted negative value
    with pytest.raises(AssertionError, match='non-negative'):
        m.fit(torch.from_numpy(Vz).to(dev), beta=1, max_iter=2, weights=Md)


# ---- the reference's recorded runs ----------------------------------------------------------------------------------------------
G23 = load_golden('g23_weighted_fit')


@pytest.mark.parametrize('case', [str(c) for c in G23['cases']])
def test_golden_g23(dev, case):
    from torchnmf_amd.metrics import weighted_beta_div
    from torchnmf_amd.nmf import NMF
    g = G23
    beta, alpha, l1_ratio, update_W = (float(x) for x in g[case + '_par'])
    V, M = torch.from_numpy(g['V']).to(dev), torch.from_numpy(g['M']).to(dev)          # integer weights as they are
    m = NMF(W=torch.from_numpy(g['W0']), H=torch.from_numpy(g['H0']), trainable_W=bool(update_W)).to(dev)
    k = int(g['iterations'])
    n = m.fit(V, beta=beta, tol=-1e9, max_iter=k, alpha=alpha, l1_ratio=l1_ratio, weights=M)
    assert n == k and m.last_precision == 'fp32'
    ew, eh = rel_err(m.W.data.cpu(), g[case + '_W']), rel_err(m.H.data.cpu(), g[case + '_H'])
    loss = float(weighted_beta_div(m.H.data, m.W.data, V, M, beta))
    el = abs(loss - float(g[case + '_loss'])) / abs(float(g[case + '_loss']))
    record('weighted_g23', case=case, W=ew, H=eh, loss=el)
    print(f'weighted_g23 {case}: W {ew:.2e} H {eh:.2e} loss {el:.2e}')
    assert ew < TOL and eh < TOL, (case, ew, eh)
    assert el < 1e-5, (case, loss, float(g[case + '_loss']))
    if not update_W:
        assert torch.equal(m.W.data.cpu(), torch.from_numpy(g['W0']))


# ---- against the existing paths ------------------------------------------------------------------------------------------------
def _small(seed=5):
    g = torch.Generator().manual_seed(seed)
    Vd = torch.rand(64, 96, generator=g) * 1.9 + 0.1
    W0, H0 = torch.rand(96, 8, generator=g) * 0.9 + 0.1, torch.rand(64, 8, generator=g) * 0.9 + 0.1
    mask = torch.rand(64, 96, generator=g) < 0.5
    return Vd, W0, H0, mask


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_unit_weights_agree_with_the_dense_fit(dev, beta):
    from torchnmf_amd.nmf import NMF
    Vd, W0, H0, _ = _small()
    a = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    b = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    a.fit(Vd.to(dev), beta=beta, tol=-1e9, max_iter=20, weights=torch.ones(64, 96, device=dev))
    b.fit(Vd.to(dev), beta=beta, tol=-1e9, max_iter=20, precision='bf16x3')
    ew, eh = rel_err(a.W.data.cpu(), b.W.data.cpu()), rel_err(a.H.data.cpu(), b.H.data.cpu())
    record('weighted_vs_dense', beta=beta, W=ew, H=eh)
    print(f'weighted_vs_dense beta {beta}: W {ew:.2e} H {eh:.2e}')
    assert ew < TOL and eh < TOL, (beta, ew, eh)


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_binary_weights_agree_with_the_missing_data_fit(dev, beta):
    from torchnmf_amd.nmf import NMF
    Vd, W0, H0, mask = _small()
    a = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    b = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    a.fit(Vd.to(dev), beta=beta, tol=-1e9, max_iter=20, weights=mask.to(dev))           # a bool mask as it is
    Vs = Vd.to(dev).sparse_mask(mask.float().to(dev).to_sparse().coalesce())
    b.fit(Vs, beta=beta, tol=-1e9, max_iter=20, unstored='missing')
    ew, eh = rel_err(a.W.data.cpu(), b.W.data.cpu()), rel_err(a.H.data.cpu(), b.H.data.cpu())
    record('weighted_vs_masked', beta=beta, W=ew, H=eh)
    print(f'weighted_vs_masked beta {beta}: W {ew:.2e} H {eh:.2e}')
    assert ew < TOL and eh < TOL, (beta, ew, eh)


@pytest.mark.parametrize('nsplit', [0, 3])
def test_step_is_reproducible(dev, nsplit):
    from torchnmf_amd import wmu
    V, M, W0, H0 = _problem(131, 70, 200)
    T = _target(V, M, dev)
    Hd, Wd = torch.from_numpy(H0).to(dev), torch.from_numpy(W0).to(dev)
    for beta in (0.5, 1.0):
        runs = []
        for fill in (NAN, 7.0):            # whatever the workspace held before
            h, w = Hd.clone(), Wd.clone()
            for _ in range(2):
                wmu._wmu_call(T, 'w', w, h, beta, step=(*REG, WE.gamma_of(beta)), nsplit=nsplit, _fill=fill)
                wmu._wmu_call(T, 'h', h, w, beta, step=(*REG, WE.gamma_of(beta)), nsplit=nsplit, _fill=fill)
            runs.append((h, w))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert bool(torch.isfinite(runs[0][0]).all()) and not torch.equal(runs[0][0], Hd)


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_loss_is_monotone(dev, beta):
    """515 x 1030, rank 40, the library's own split count (more than one part on the H side): the weighted loss does not
    increase over 10 iterations; 1e-6 of the loss is the allowance for its rounding."""
    from torchnmf_amd import _capi
    from torchnmf_amd.metrics import WeightedTarget, weighted_beta_div
    from torchnmf_amd.wmu import WeightedMU
    N, C, R = 515, 1030, 40
    assert _capi.load().nmfmu_wmu_nsplit(N, C, 64) > 1 and _capi.load().nmfmu_wmu_nsplit(C, N, 64) > 1
    g = torch.Generator().manual_seed(11)
    V = (torch.rand(N, C, generator=g) * 1.9 + 0.1).to(dev)
    M = (torch.rand(N, C, generator=g) * 3.75 + 0.25) * (torch.rand(N, C, generator=g) < 0.7)
    W = (torch.rand(C, R, generator=g) * 0.9 + 0.1).to(dev)
    H = (torch.rand(N, R, generator=g) * 0.9 + 0.1).to(dev)
    T = WeightedTarget(V, M.to(dev))
    eng = WeightedMU(T, None, W, H, beta)
    losses = [float(weighted_beta_div(H, W, T, None, beta))]
    for _ in range(10):
        eng.w_step()
        eng.h_step()
        losses.append(float(weighted_beta_div(H, W, T, None, beta)))
    print(f'weighted monotone beta {beta}:', losses)
    record('weighted_monotone', beta=beta, first=losses[0], last=losses[-1])
    assert all(b <= a + 1e-6 * a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.9 * losses[0]
    assert abs(eng.divergence() - losses[-1]) <= 1e-6 * losses[-1]


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def _dense_weighted_loss(H, W, V, Mw, beta):
    """sum m d_beta(v | y), metrics.py:60-96 entry by entry, float64 torch (autograd gives the reference gradients)."""
    sel = Mw > 0
    x, y, m = (H @ W.T)[sel], V[sel], Mw[sel]
    eps = WE.EPS
    if beta == 2:
        return 0.5 * (m @ (x - y) ** 2)
    if beta == 1:
        return m @ (y * ((y + eps).log() - (x + eps).log()) - y + x)
    if beta == 0:
        return m @ ((y + eps) / (x + eps) - (y + eps).log() + (x + eps).log() - 1)
    x = x + eps
    return m @ (y ** beta + (beta - 1) * x ** beta - beta * y * x ** (beta - 1)) / (beta * (beta - 1))


@pytest.mark.parametrize('R', [3, 200])
@pytest.mark.parametrize('beta', [0, 0.5, 1, 2])
def test_autograd_gradients(dev, beta, R):
    from torchnmf_amd.metrics import weighted_beta_div
    N, C = 131, 70
    V, M, W0, H0 = _problem(N, C, R)
    T = _target(V, M, dev)
    H64 = torch.from_numpy(H0).double().requires_grad_()
    W64 = torch.from_numpy(W0).double().requires_grad_()
    ref = _dense_weighted_loss(H64, W64, torch.from_numpy(V).double(), torch.from_numpy(M).double(), beta)
    (ref * UP).backward()
    H = torch.from_numpy(H0).to(dev).requires_grad_()
    W = torch.from_numpy(W0).to(dev).requires_grad_()
    loss = weighted_beta_div(H, W, T, None, beta)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    (loss * UP).backward()
    ref_loss, loss_bound = WE.loss(V, M, H0, W0, beta)
    info = dict(beta=beta, R=R)
    assert abs(float(ref) - ref_loss) <= 1e-11 * abs(ref_loss)
    _check('weighted_autograd_value', loss.detach().reshape(()), ref_loss, loss_bound + WE.U * abs(ref_loss), **info)
    for side, got, want in (('h', H.grad, H64.grad), ('w', W.grad, W64.grad)):
        t = WE.terms(V, M, H0, W0, beta, side)
        # up (den - num): the two planes' bounds, the subtraction, the multiply
        bound = abs(UP) * (t['num_bound'] + t['den_bound'] + 2 * WE.U * np.abs(t['den'] - t['num']))
        # (the emulation's planes against autograd: two float64 routes to the same gradient.  beta == 0: metrics.py:56 adds
        # eps to the TARGET, the update rule of nmf.py:68-70 does not, so den - num misses eps / (y + eps)^2 per entry --
        # eps / v of the entry's numerator term, at most 2^-23 / 0.1 here)
        same = 1e-10 if beta != 0 else WE.EPS / 0.1
        assert np.abs(UP * (t['den'] - t['num']) - want.numpy()).max() <= same * np.abs(want.numpy()).max()
        _check('weighted_autograd_grad', got, want.numpy(), bound, side=side, **info)


def test_autograd_records_nothing_without_grad(dev, monkeypatch):
    from torchnmf_amd import wmu
    from torchnmf_amd.metrics import weighted_beta_div
    from torchnmf_amd.nmf import NMF
    V, M, W0, H0 = _problem(131, 70, 3)
    T = _target(V, M, dev)
    sides = []
    orig = wmu._wmu_call

    def tap(T_, side, *a, **k):
        sides.append(side)
        return orig(T_, side, *a, **k)
    monkeypatch.setattr(wmu, '_wmu_call', tap)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0), trainable_W=False).to(dev)
    with torch.no_grad():
        quiet = weighted_beta_div(m.H, m.W, T, None, 0.5)
    plain = weighted_beta_div(m.H.data, m.W.data, T, None, 0.5)
    assert quiet.grad_fn is None and not quiet.requires_grad and plain.grad_fn is None and sides == []
    assert torch.equal(quiet, plain)
    weighted_beta_div(m.H, m.W, T, None, 0.5).backward()                 # a frozen W launches no W side
    assert sides == ['h'] and m.W.grad is None and m.H.grad is not None
    # a tensor pair and a prepared target are the same loss
    assert torch.equal(weighted_beta_div(m.H.data, m.W.data, T.V, T.M, 0.5), plain)


def test_sparsity_proj_on_a_weighted_target(dev):
    from torchnmf_amd.hoyer import hoyer_project, slice_norms
    from torchnmf_amd.metrics import sparseness, weighted_beta_div
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import SparsityProj
    N = 37                                 # (small: the projection to sparseness 0.3 leaves no row of H all zero, so the
    V, M, W0, H0 = _problem(N, 29, 3)      #  loss at beta = 0.5 stays away from its pole at y = 0)
    T = _target(V, M, dev)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    sigma = 0.3
    with torch.no_grad():                  # start ON the constraint set, so that the step is a projected gradient step
        norms = slice_norms(m.H.data, 1)
        l1 = N ** 0.5 * (1 - sigma) + sigma
        hoyer_project(m.H.data, l1 * norms, norms * norms, 1, out=m.H.data)
    opt = SparsityProj([m.H], sigma)

    def closure():
        opt.zero_grad()
        return weighted_beta_div(m.H, m.W, T, None, 0.5)
    with torch.no_grad():
        before = float(closure())
    after = float(opt.step(closure))
    print(f'weighted SparsityProj: {before} -> {after}')
    assert after <= before and bool(torch.isfinite(m.H.data).all())
    assert abs(float(sparseness(m.H.data[:, 0])) - sigma) < 1e-4
