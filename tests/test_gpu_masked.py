"""Missing-data NMF on the device (csrc/nmfmu_sparse_masked.hip, sparse_engine.MaskedMU, ``fit(..., unstored='missing')``,
``sparse_beta_div(..., unstored='missing')``): terms, step and loss per element against the float64 reference under the bounds
derived in tests/masked_emulation.py (no element left out), the reference's recorded runs (golden g20), agreement with the
dense path on a target that stores everything, indifference to what lies outside the stored set, reproducibility, beta <= 0
and autograd.

The per-element target is 37 x 29; the owner axis cycles through 0, 1, 4, 5, 8, 9 and 20 stored entries (unroll tails, whole
trips, and with chunk = 8 a row of exactly one chunk and rows split in two and three), once drawn on the rows of V and once on
its columns, so that both sides meet every count; one index of the other axis holds no entry.

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 19.
"""
import functools

import numpy as np
import pytest
import torch

import masked_emulation as M
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

N, C = 37, 29
RANKS = [3, 33, 100, 200]             # r_pad 32 / 64 / 128 / 256, RL 1 / 1 / 2 / 4
BETAS = [-1, 0, 0.5, 1, 2, 3]
CHUNKS = [512, 8]
REG = (0.07 * 0.3, 0.07 * 0.7)
TOL = 1e-4                            # the project's bar for factors after a recorded run
UP = -1.75                            # the incoming gradient of the autograd tests: signed, not 1, exact in fp32
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(R, axis):
    return M.make_problem(N, C, R, axis)


def _sparse(idx, vals, shape, dev):
    return torch.sparse_coo_tensor(torch.from_numpy(np.asarray(idx)), torch.from_numpy(np.asarray(vals)), shape).to(dev)


def _target(idx, vals, shape, dev, chunk=512):
    from torchnmf_amd.metrics import SparseTarget
    return SparseTarget(_sparse(idx, vals, shape, dev), chunk=chunk)


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (name, info)
    err = M.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


# ---- per element against the float64 reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('beta', BETAS)
def test_terms_step_loss_per_element(dev, beta, R, chunk):
    from torchnmf_amd import _capi
    from torchnmf_amd import sparse_autograd as SA
    r_pad = _capi.load().nmfmu_pad_rank(R)
    for axis in (0, 1):
        idx, vals, W0, H0 = _problem(R, axis)
        info = dict(beta=beta, R=R, chunk=chunk, axis=axis)
        T = _target(idx, vals, (N, C), dev, chunk)
        split = (T.n_ws_w if axis else T.n_ws_h) > 0
        assert split == (chunk == 8)
        Hd, Wd = torch.from_numpy(H0).to(dev), torch.from_numpy(W0).to(dev)
        for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
            # terms: every element of both planes is written (they start as NaN), padded columns exactly 0
            ref = M.terms(idx, vals, (N, C), H0, W0, beta, side, chunk)
            num, den = SA._masked_call(T, side, owner, panel, float(beta), _fill=NAN)
            assert num.shape == den.shape == (owner.shape[0], r_pad)
            assert bool((num[:, R:] == 0).all()) and bool((den[:, R:] == 0).all())
            _check('masked_terms_num', num[:, :R], ref['num'], ref['num_bound'], side=side, **info)
            _check('masked_terms_den', den[:, :R], ref['den'], ref['den_bound'], side=side, **info)
            empty = torch.from_numpy(ref['count'] == 0).to(dev)
            assert bool(empty.any()) and bool((num[empty] == 0).all()) and bool((den[empty] == 0).all())
            # step, without and with regularisers, on a copy of the owner
            for l1, l2 in ((0.0, 0.0), REG):
                new_ref, bound, _ = M.step(idx, vals, (N, C), H0, W0, beta, side, l1, l2, chunk)
                f = owner.clone()
                before = panel.clone()
                SA._masked_call(T, side, f, panel, float(beta), step=(l1, l2, M.gamma_of(beta)), _fill=NAN)
                _check('masked_step', f, new_ref, bound, side=side, reg=l1 > 0, **info)
                assert torch.equal(panel, before)
                if l1 == 0:
                    assert torch.equal(f[empty], owner[empty])          # nothing measured there: unchanged
        ref_loss, loss_bound = M.loss(idx, vals, H0, W0, beta)
        got = SA._masked_loss(Hd, Wd, T, float(beta))
        assert got.dtype == torch.float64
        _check('masked_loss', got.reshape(()), ref_loss, loss_bound, **info)


@pytest.mark.parametrize('beta', BETAS)
def test_target_without_entries(dev, beta):
    from torchnmf_amd import sparse_autograd as SA
    _, _, W0, H0 = _problem(33, 0)
    none = np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.float32)
    T = _target(*none, (N, C), dev)
    Hd, Wd = torch.from_numpy(H0).to(dev), torch.from_numpy(W0).to(dev)
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        num, den = SA._masked_call(T, side, owner, panel, float(beta), _fill=NAN)
        assert bool((num == 0).all()) and bool((den == 0).all())
        f = owner.clone()
        SA._masked_call(T, side, f, panel, float(beta), step=(0.0, 0.0, M.gamma_of(beta)))
        assert torch.equal(f, owner)
    assert float(SA._masked_loss(Hd, Wd, T, float(beta))) == 0.0


# ---- the reference's recorded runs ----------------------------------------------------------------------------------------------
G20 = load_golden('g20_masked_fit')


@pytest.mark.parametrize('case', [str(c) for c in G20['cases']])
def test_golden_g20(dev, case):
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    g = G20
    beta, alpha, l1_ratio, update_W = (float(x) for x in g[case + '_par'])
    V = _sparse(g['indices'], g['values'], tuple(int(x) for x in g['shape']), dev)
    m = NMF(W=torch.from_numpy(g['W0']), H=torch.from_numpy(g['H0']), trainable_W=bool(update_W)).to(dev)
    k = int(g['iterations'])
    n = m.fit(V, beta=beta, tol=-1e9, max_iter=k, alpha=alpha, l1_ratio=l1_ratio, unstored='missing')
    assert n == k and m.last_precision == 'fp32'
    ew, eh = rel_err(m.W.data.cpu(), g[case + '_W']), rel_err(m.H.data.cpu(), g[case + '_H'])
    loss = float(sparse_beta_div(m.H.data, m.W.data, V, beta, unstored='missing'))
    el = abs(loss - float(g[case + '_loss'])) / abs(float(g[case + '_loss']))
    record('masked_g20', case=case, W=ew, H=eh, loss=el)
    print(f'masked_g20 {case}: W {ew:.2e} H {eh:.2e} loss {el:.2e}')
    assert ew < TOL and eh < TOL, (case, ew, eh)
    assert el < 1e-5, (case, loss, float(g[case + '_loss']))
    if not update_W:
        assert torch.equal(m.W.data.cpu(), torch.from_numpy(g['W0']))


# ---- against the existing path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_full_target_agrees_with_the_dense_fit(dev, beta):
    """A target that stores ALL N x C entries: the masked and the dense problem coincide."""
    from torchnmf_amd.nmf import NMF
    g = torch.Generator().manual_seed(5)
    Vd = torch.rand(64, 96, generator=g) * 1.9 + 0.1
    W0, H0 = torch.rand(96, 8, generator=g) * 0.9 + 0.1, torch.rand(64, 8, generator=g) * 0.9 + 0.1
    Vs = Vd.to_sparse().coalesce()
    assert Vs._nnz() == 64 * 96
    a = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    b = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    a.fit(Vs.to(dev), beta=beta, tol=-1e9, max_iter=20, unstored='missing')
    b.fit(Vd.to(dev), beta=beta, tol=-1e9, max_iter=20, precision='bf16x3')
    ew, eh = rel_err(a.W.data.cpu(), b.W.data.cpu()), rel_err(a.H.data.cpu(), b.H.data.cpu())
    record('masked_vs_dense', beta=beta, W=ew, H=eh)
    print(f'masked_vs_dense beta {beta}: W {ew:.2e} H {eh:.2e}')
    assert ew < TOL and eh < TOL, (beta, ew, eh)


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_unstored_entries_are_ignored(dev, beta):
    """Two targets that agree on the stored set; the second held large values everywhere else before a sparse_mask."""
    from torchnmf_amd.nmf import NMF
    idx, vals, W0, H0 = _problem(33, 0)
    Va = _sparse(idx, vals, (N, C), dev).coalesce()
    dense = torch.full((N, C), 1000.0, device=dev)
    dense[Va.indices()[0], Va.indices()[1]] = Va.values()
    Vb = dense.sparse_mask(Va)
    assert Vb._nnz() == Va._nnz() and float(dense.max()) == 1000.0
    fits = []
    for V in (Va, Vb):
        m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
        m.fit(V, beta=beta, tol=-1e9, max_iter=10, unstored='missing')
        fits.append((m.W.data.clone(), m.H.data.clone()))
    assert torch.equal(fits[0][0], fits[1][0]) and torch.equal(fits[0][1], fits[1][1])
    assert not torch.equal(fits[0][0], torch.from_numpy(W0).to(dev))
    # ... while the default reads the unstored entries as zeros: another fit altogether
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    m.fit(Va, beta=beta, tol=-1e9, max_iter=10)
    assert rel_err(m.H.data.cpu(), fits[0][1].cpu()) > 1e-2


@pytest.mark.parametrize('chunk', CHUNKS)
def test_step_is_reproducible(dev, chunk):
    from torchnmf_amd import sparse_autograd as SA
    idx, vals, W0, H0 = _problem(200, 0)
    T = _target(idx, vals, (N, C), dev, chunk)
    assert (T.n_ws_h > 0) == (chunk == 8)
    Hd, Wd = torch.from_numpy(H0).to(dev), torch.from_numpy(W0).to(dev)
    for beta in (0.5, 1.0):
        runs = []
        for fill in (NAN, 7.0):            # whatever the workspace held before
            h, w = Hd.clone(), Wd.clone()
            for _ in range(2):
                SA._masked_call(T, 'w', w, h, beta, step=(*REG, M.gamma_of(beta)), _fill=fill)
                SA._masked_call(T, 'h', h, w, beta, step=(*REG, M.gamma_of(beta)), _fill=fill)
            runs.append((h, w))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert bool(torch.isfinite(runs[0][0]).all()) and not torch.equal(runs[0][0], Hd)


# ---- beta <= 0 ----------------------------------------------------------------------------------------------------------------
def test_beta_zero_fits_positive_entries(dev):
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.sparse_engine import MaskedMU
    idx, vals, W0, H0 = _problem(3, 0)
    V = _sparse(idx, vals, (N, C), dev)
    W, H = torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev)
    eng = MaskedMU(V, W, H, 0.0)
    assert eng.target_flags() == (False, False)
    losses = [eng.divergence()]
    for _ in range(20):
        eng.w_step()
        eng.h_step()
        losses.append(eng.divergence())
    print('masked beta 0 losses', losses)
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.9 * losses[0]
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    assert m.fit(V, beta=0, tol=-1e9, max_iter=20, unstored='missing') == 20
    assert torch.equal(m.W.data, W) and torch.equal(m.H.data, H)       # fit drives the same engine
    with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
        m.fit(V, beta=0, max_iter=2)                                     # the default: unstored entries are zeros


def test_beta_zero_refuses_a_stored_zero(dev):
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    idx, vals, W0, H0 = _problem(3, 0)
    vals = vals.copy()
    vals[5] = 0.0
    V = _sparse(idx, vals, (N, C), dev)
    assert V.coalesce()._nnz() == len(vals)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    for beta in (0, -1):
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            m.fit(V, beta=beta, max_iter=2, unstored='missing')
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            sparse_beta_div(m.H, m.W, V, beta, unstored='missing')
    assert m.fit(V, beta=1, tol=-1e9, max_iter=2, unstored='missing') == 2      # a stored zero is data for beta > 0
    assert bool(torch.isfinite(m.H.data).all())


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def _dense_masked_loss(H, W, V, Mk, beta):
    """metrics.py:60-96 on the gathered vectors, float64 torch (autograd gives the reference gradients)."""
    x, y = (H @ W.T)[Mk], V[Mk]
    eps = M.EPS
    if beta == 2:
        return 0.5 * ((x - y) ** 2).sum()
    if beta == 1:
        return y @ ((y + eps).log() - (x + eps).log()) - y.sum() + x.sum()
    if beta == 0:
        return ((y + eps) / (x + eps)).sum() - (y + eps).log().sum() + (x + eps).log().sum() - y.numel()
    x = x + eps
    return ((y ** beta).sum() + (beta - 1) * (x ** beta).sum() - beta * (y @ x ** (beta - 1))) / (beta * (beta - 1))


@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('R', [3, 200])
@pytest.mark.parametrize('beta', [0, 0.5, 1, 2])
def test_autograd_gradients(dev, beta, R, chunk):
    from torchnmf_amd.metrics import sparse_beta_div
    idx, vals, W0, H0 = _problem(R, 0)
    T = _target(idx, vals, (N, C), dev, chunk)
    Vn, Mn = M.dense(idx, vals, (N, C))
    H64 = torch.from_numpy(H0).double().requires_grad_()
    W64 = torch.from_numpy(W0).double().requires_grad_()
    ref = _dense_masked_loss(H64, W64, torch.from_numpy(Vn), torch.from_numpy(Mn), beta)
    (ref * UP).backward()
    H = torch.from_numpy(H0).to(dev).requires_grad_()
    W = torch.from_numpy(W0).to(dev).requires_grad_()
    loss = sparse_beta_div(H, W, T, beta, unstored='missing')
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    (loss * UP).backward()
    ref_loss, loss_bound = M.loss(idx, vals, H0, W0, beta)
    info = dict(beta=beta, R=R, chunk=chunk)
    assert abs(float(ref) - ref_loss) <= 1e-11 * abs(ref_loss)
    _check('masked_autograd_value', loss.detach().reshape(()), ref_loss, loss_bound + M.U * abs(ref_loss), **info)
    for side, got, want in (('h', H.grad, H64.grad), ('w', W.grad, W64.grad)):
        t = M.terms(idx, vals, (N, C), H0, W0, beta, side, chunk)
        # up (den - num): the two planes' bounds, the subtraction, the multiply
        bound = abs(UP) * (t['num_bound'] + t['den_bound'] + 2 * M.U * np.abs(t['den'] - t['num']))
        # (the emulation's planes against autograd: two float64 routes to the same gradient.  beta == 0: metrics.py:56 adds
        # eps to the TARGET, the update rule of nmf.py:68-70 does not, so den - num misses eps / (s + eps)^2 per entry --
        # eps / v of the entry's numerator term, at most 2^-23 / 0.1 here)
        same = 1e-10 if beta != 0 else M.EPS / 0.1
        assert np.abs(UP * (t['den'] - t['num']) - want.numpy()).max() <= same * np.abs(want.numpy()).max()
        _check('masked_autograd_grad', got, want.numpy(), bound, side=side, **info)


def test_autograd_records_nothing_without_grad(dev, monkeypatch):
    from torchnmf_amd import sparse_autograd as SA
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    idx, vals, W0, H0 = _problem(3, 0)
    T = _target(idx, vals, (N, C), dev)
    sides = []
    orig = SA._masked_call

    def tap(T_, side, *a, **k):
        sides.append(side)
        return orig(T_, side, *a, **k)
    monkeypatch.setattr(SA, '_masked_call', tap)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0), trainable_W=False).to(dev)
    with torch.no_grad():
        quiet = sparse_beta_div(m.H, m.W, T, 0.5, unstored='missing')
    plain = sparse_beta_div(m.H.data, m.W.data, T, 0.5, unstored='missing')
    assert quiet.grad_fn is None and not quiet.requires_grad and plain.grad_fn is None and sides == []
    assert torch.equal(quiet, plain)
    sparse_beta_div(m.H, m.W, T, 0.5, unstored='missing').backward()     # a frozen W launches no W side
    assert sides == ['h'] and m.W.grad is None and m.H.grad is not None
    # the default path is untouched by the keyword's presence
    assert torch.equal(sparse_beta_div(m.H.data, m.W.data, T, 2), sparse_beta_div(m.H.data, m.W.data, T, 2, unstored='zero'))


def test_sparsity_proj_on_a_masked_target(dev):
    from torchnmf_amd.hoyer import hoyer_project, slice_norms
    from torchnmf_amd.metrics import sparse_beta_div, sparseness
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import SparsityProj
    idx, vals, W0, H0 = _problem(3, 0)
    T = _target(idx, vals, (N, C), dev)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    sigma = 0.3
    with torch.no_grad():                  # start ON the constraint set, so that the step is a projected gradient step
        norms = slice_norms(m.H.data, 1)
        l1 = N ** 0.5 * (1 - sigma) + sigma
        hoyer_project(m.H.data, l1 * norms, norms * norms, 1, out=m.H.data)
    opt = SparsityProj([m.H], sigma)

    def closure():
        opt.zero_grad()
        return sparse_beta_div(m.H, m.W, T, 0.5, unstored='missing')
    with torch.no_grad():
        before = float(closure())
    after = float(opt.step(closure))
    print(f'masked SparsityProj: {before} -> {after}')
    assert after <= before
    assert abs(float(sparseness(m.H.data[:, 0])) - sigma) < 1e-4
