"""``sparse_beta_div`` on the device: value and both gradients per element against the float64 reference under the bounds
derived in tests/sparse_autograd_reference.py (no element left out), determinism and subsets, sparse == dense through the
existing autograd kernels, the reference's recorded runs (golden g19) and end-to-end use with torch.optim / SparsityProj.

The large target (1100 x 1200) has row 3 and column 7 full (three segments each at the default chunk of 512), row 5 with
exactly 512 and row 6 with 513 entries, a row (10) and a column (20) with one entry; a full row and a full column leave
no row or column of THAT target empty, so rows and columns without an entry are on the 37 x 53 target (which also has
one-entry rows and columns) and on the target without any stored entry.

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 18.
"""
import functools

import numpy as np
import pytest
import torch

import sparse_autograd_reference as A
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

UP = -1.75            # the incoming gradient of the per-element tests: signed, not 1, exact in fp32
RANKS = [5, 33, 100, 130]          # r_pad 32 / 64 / 128 / 256, RL 1 / 1 / 2 / 4
TOL_FACTORS = 1e-4    # the project's bar for factors after a recorded run (tests/test_gpu_hoyer.py)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


# ---- problems (built once, shared, never modified) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pattern(name):
    """(idx [2, nnz] int64 sorted by (row, col), vals fp32 on a 2^-10 grid in (0, 1], (N, C))."""
    g = np.random.default_rng({'big': 11, 'small': 12, 'empty': 13}[name])
    if name == 'big':
        N, C = 1100, 1200
        mask = g.random((N, C)) < 0.01
        for row, n in ((5, 511), (6, 512)):               # + column 7 below: 512 and 513 entries
            mask[row] = False
            mask[row, g.choice(np.setdiff1d(np.arange(C), [7, 20]), size=n, replace=False)] = True
        mask[10] = False                                   # one entry (column 7)
        mask[:, 20] = False                                # one entry (row 3)
        mask[3] = True
        mask[:, 7] = True
    elif name == 'small':
        N, C = 37, 53
        mask = g.random((N, C)) < 0.2
        mask[4] = False                                    # an empty row, an empty column
        mask[:, 9] = False
        mask[8] = False                                    # a row and a column with one entry
        mask[:, 30] = False
        mask[8, 2] = True
        mask[20, 30] = True
    else:
        N, C = 10, 9
        mask = np.zeros((N, C), dtype=bool)
    idx = np.stack(np.nonzero(mask)).astype(np.int64)
    vals = ((np.floor(g.random(idx.shape[1]) * 1024) + 1) / 1024).astype(np.float32)
    return idx, vals, (N, C)


def test_patterns_have_the_structure_they_claim():
    idx, _, (N, C) = _pattern('big')
    rc, cc = np.bincount(idx[0], minlength=N), np.bincount(idx[1], minlength=C)
    assert rc[3] == C and cc[7] == N and rc[5] == 512 and rc[6] == 513 and rc[10] == 1 and cc[20] == 1
    assert -(-rc[3] // 512) == 3 and -(-cc[7] // 512) == 3
    assert 0.008 < idx.shape[1] / (N * C) < 0.02
    idx, _, (N, C) = _pattern('small')
    rc, cc = np.bincount(idx[0], minlength=N), np.bincount(idx[1], minlength=C)
    assert rc[4] == 0 and cc[9] == 0 and rc[8] == 1 and cc[30] == 1
    assert _pattern('empty')[0].shape[1] == 0


@functools.lru_cache(maxsize=None)
def _factors(name, R):
    _, _, (N, C) = _pattern(name)
    g = torch.Generator().manual_seed(N * 7 + C * 3 + R)
    return torch.rand(N, R, generator=g) + 0.05, torch.rand(C, R, generator=g) + 0.05


@functools.lru_cache(maxsize=None)
def _reference(name, R, beta, up, chunk):
    idx, vals, shape = _pattern(name)
    H, W = _factors(name, R)
    return A.evaluate(idx, vals, shape, H.numpy(), W.numpy(), beta, up=up, chunk=chunk)


def _target(name, dev, chunk=512):
    from torchnmf_amd.metrics import SparseTarget
    idx, vals, shape = _pattern(name)
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).to(dev)
    return SparseTarget(V, chunk=chunk)


def _run(T, H0, W0, beta, dev, up=None, need_h=True, need_w=True):
    """(loss, grad_H | None, grad_W | None) on the device."""
    from torchnmf_amd.metrics import sparse_beta_div
    H = H0.to(dev).requires_grad_(need_h)
    W = W0.to(dev).requires_grad_(need_w)
    loss = sparse_beta_div(H, W, T, beta)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == 'cuda'
    (loss if up is None else loss * up).backward()
    return loss.detach(), H.grad, W.grad


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy()
    assert got.shape == np.shape(ref), (name, info)
    err = S_bound_err(got, ref, bound)
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


def S_bound_err(got, ref, bound):
    import sparse_emulation as S
    return S.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))


# ---- per element against the float64 reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('beta', [1, 2])
@pytest.mark.parametrize('name', ['big', 'small', 'empty'])
def test_per_element_against_float64(dev, name, beta, R):
    ref = _reference(name, R, beta, UP, 512)
    H0, W0 = _factors(name, R)
    T = _target(name, dev)
    if name == 'big':
        assert T.multi_h.shape[0] == 2 and T.multi_w.shape[0] == 1      # rows 3 and 6; column 7
        assert T.multi_h.tolist() == [[3, 0, 3], [6, 3, 2]] and T.multi_w.tolist() == [[7, 0, 3]]
    loss, gH, gW = _run(T, H0, W0, beta, dev, up=UP)
    info = dict(target=name, beta=beta, R=R)
    _check('sparse_autograd_value', loss.reshape(()), ref['loss'], ref['loss_bound'], **info)
    _check('sparse_autograd_grad_H', gH, ref['gH'], ref['gH_bound'], **info)
    _check('sparse_autograd_grad_W', gW, ref['gW'], ref['gW_bound'], **info)


# ---- determinism and subsets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1, 2])
@pytest.mark.parametrize('R', [33, 130])
def test_determinism_subsets_and_nan_prefill(dev, beta, R):
    from torchnmf_amd import sparse_autograd as SA
    H0, W0 = _factors('big', R)
    T = _target('big', dev)
    loss, gH, gW = _run(T, H0, W0, beta, dev, up=UP)
    loss2, gH2, gW2 = _run(T, H0, W0, beta, dev, up=UP)
    assert torch.equal(loss, loss2) and torch.equal(gH, gH2) and torch.equal(gW, gW2)
    _, gH1, none_w = _run(T, H0, W0, beta, dev, up=UP, need_w=False)
    _, none_h, gW1 = _run(T, H0, W0, beta, dev, up=UP, need_h=False)
    assert none_w is None and none_h is None
    assert torch.equal(gH, gH1) and torch.equal(gW, gW1)
    # outputs and workspace pre-filled with NaN: an element nobody wrote cannot pass
    Hc, Wc = H0.to(dev), W0.to(dev)
    _, s, (small_h, small_w) = SA._forward(Hc, Wc, T, float(beta), want_s=beta == 1)
    up = torch.tensor([UP], device=dev)
    nan = float('nan')
    gHn = SA._backward_side(Hc, Wc, small_w, T, 'h', float(beta), s, up, _fill=nan)
    gWn = SA._backward_side(Wc, Hc, small_h, T, 'w', float(beta), s, up, _fill=nan)
    assert torch.equal(gH, gHn) and torch.equal(gW, gWn)


def test_nonfinite_panel_row0_reaches_only_rows_that_store_column0(dev):
    """The kernels hand the panel rows of four entries to the wave per trip; an entry past the end of a row's last group
    takes no panel row at all (nmfmu_sparse_common.h: fetch_group), so it is not row 0 times g = 0.  With W[0, 2] = +inf
    (the same finite pos and s) every row of grad_H that does not store column 0 keeps its bits; 0 * inf = NaN would
    reach each of them whose entry count is not a multiple of four (one segment per row at chunk 512)."""
    from torchnmf_amd import sparse_autograd as SA
    R, beta = 33, 1.0
    idx, _, (N, _) = _pattern('small')
    H0, W0 = _factors('small', R)
    T = _target('small', dev)
    Hc, Wc = H0.to(dev), W0.to(dev)
    _, s, (_, small_w) = SA._forward(Hc, Wc, T, beta, want_s=True)
    up = torch.tensor([UP], device=dev)
    Winf = Wc.clone()
    Winf[0, 2] = float('inf')
    g_fin = SA._backward_side(Hc, Wc, small_w, T, 'h', beta, s, up)
    g_inf = SA._backward_side(Hc, Winf, small_w, T, 'h', beta, s, up)
    with0 = np.unique(idx[0][idx[1] == 0])
    without0 = np.setdiff1d(np.arange(N), with0)
    counts = np.bincount(idx[0], minlength=N)
    assert len(with0) and np.any(counts[without0] % 4 != 0) and T.multi_h.shape[0] == 0
    assert not torch.isfinite(g_inf[torch.from_numpy(with0).to(dev), 2]).any()       # the value did go in
    rows = torch.from_numpy(without0).to(dev)
    same = (g_fin[rows].view(torch.int32) == g_inf[rows].view(torch.int32)).all(dim=1)
    assert bool(same.all()), ('rows that differ', without0[(~same).cpu().numpy()].tolist())


@pytest.mark.parametrize('beta', [1, 2])
def test_chunk4_against_chunk512(dev, beta):
    """chunk = 4 sends every row with more than four entries through the workspace and the finishing kernel; both chunkings
    lie within their own bound of the float64 reference, hence within the sum of the two bounds of each other."""
    R = 33
    H0, W0 = _factors('big', R)
    T4 = _target('big', dev, chunk=4)
    assert T4.multi_h.shape[0] > 1000 and T4.multi_w.shape[0] > 1000
    ref4, ref512 = _reference('big', R, beta, UP, 4), _reference('big', R, beta, UP, 512)
    loss4, gH4, gW4 = _run(T4, H0, W0, beta, dev, up=UP)
    loss, gH, gW = _run(_target('big', dev), H0, W0, beta, dev, up=UP)
    info = dict(beta=beta, R=R, chunk=4)
    _check('sparse_autograd_chunk4_value', loss4.reshape(()), ref4['loss'], ref4['loss_bound'], **info)
    _check('sparse_autograd_chunk4_grad_H', gH4, ref4['gH'], ref4['gH_bound'], **info)
    _check('sparse_autograd_chunk4_grad_W', gW4, ref4['gW'], ref4['gW_bound'], **info)
    for a, b, k in ((gH4, gH, 'gH'), (gW4, gW, 'gW')):
        d = (a.double() - b.double()).abs().cpu().numpy()
        assert np.all(d <= ref4[k + '_bound'] + ref512[k + '_bound'])
    # the unsplit plan (chunk = None) has no split row and agrees in the same way
    from torchnmf_amd.metrics import SparseTarget
    idx, vals, shape = _pattern('big')
    Tn = SparseTarget(torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).to(dev), chunk=None)
    assert Tn.multi_h.shape[0] == 0 and Tn.multi_w.shape[0] == 0 and Tn.n_ws_h == 0
    refn = _reference('big', R, beta, UP, Tn.chunk)
    _, gHn, gWn = _run(Tn, H0, W0, beta, dev, up=UP)
    _check('sparse_autograd_unsplit_grad_H', gHn, refn['gH'], refn['gH_bound'], beta=beta, R=R)
    _check('sparse_autograd_unsplit_grad_W', gWn, refn['gW'], refn['gW_bound'], beta=beta, R=R)


# ---- sparse == dense on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1, 2])
@pytest.mark.parametrize('name', ['big', 'small'])
def test_sparse_equals_dense_on_the_device(dev, name, beta):
    """The reference's own style of test (tests/test_nmf_sparse.py): the sparse loss and gradients against
    ``beta_div(NMF.reconstruct(H, W), V.to_dense(), beta)`` through the existing autograd kernels.  Tolerance: the sum of
    the two paths' bounds against float64 (the dense one: ``_single_layer_bounds`` of tests/test_gpu_autograd.py and
    ``dense_value_bound``); at beta == 1 the dense value holds v log(v + eps) where the sparse one has v log v -- that
    difference is computed and taken out."""
    from test_gpu_autograd import _single_layer_bounds
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    R = 33
    idx, vals, shape = _pattern(name)
    H0, W0 = _factors(name, R)
    ref = _reference(name, R, beta, 1.0, 512)
    loss, gH, gW = _run(_target(name, dev), H0, W0, beta, dev)
    Vd = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).to_dense()
    H = H0.to(dev).requires_grad_()
    W = W0.to(dev).requires_grad_()
    dense = beta_div(NMF.reconstruct(H, W), Vd.to(dev), beta)
    dense.backward()
    _, bH, _, bW = _single_layer_bounds(H0, W0, Vd, beta)
    known = A.known_log_eps_term(vals) if beta == 1 else 0.0
    tol = A.dense_value_bound(H0.numpy(), W0.numpy(), Vd.numpy(), beta) + ref['loss_bound']
    dv = abs(float(dense.detach().double()) - float(loss.double()) - known)
    record('sparse_autograd_vs_dense_value', target=name, beta=beta, difference=dv, tolerance=tol, known_term=known)
    print(f'sparse vs dense {name} beta {beta}: |dense - sparse - known| = {dv:.3e}, tolerance {tol:.3e}, known {known:.3e}')
    assert dv <= tol, (dv, tol, known)
    for tag, a, b, bd, bs in (('H', H.grad, gH, bH, ref['gH_bound']), ('W', W.grad, gW, bW, ref['gW_bound'])):
        d = (a.double() - b.double()).abs().cpu().numpy()
        lim = bd.numpy() + bs
        frac = float(np.max(d / lim))
        record('sparse_autograd_vs_dense_grad', target=name, beta=beta, output=tag, worst_fraction_of_bound=frac)
        assert np.all(d <= lim), (tag, frac)


# ---- golden g19 ---------------------------------------------------------------------------------------------------------------------
def _g19_target(g, dev):
    from torchnmf_amd.metrics import SparseTarget
    shape = tuple(int(x) for x in g['shape'])
    V = torch.sparse_coo_tensor(torch.from_numpy(g['indices']), torch.from_numpy(g['values']), shape).to(dev)
    return SparseTarget(V), shape


@pytest.mark.parametrize('beta', [1, 2])
def test_golden_g19_loss_and_gradients(dev, beta):
    """(a): the reference's float64 sparse loss with autograd; the device results lie within the derived bounds of it."""
    g = load_golden('g19_sparse_autograd')
    T, shape = _g19_target(g, dev)
    b = A.evaluate(g['indices'], g['values'], shape, g['H0'], g['W0'], beta, up=1.0)
    loss, gH, gW = _run(T, torch.from_numpy(g['H0']), torch.from_numpy(g['W0']), beta, dev)
    _check('sparse_autograd_g19_value', loss.reshape(()), float(g[f'a_loss_b{beta}']), b['loss_bound'], beta=beta)
    _check('sparse_autograd_g19_grad_H', gH, g[f'a_gH_b{beta}'], b['gH_bound'], beta=beta)
    _check('sparse_autograd_g19_grad_W', gW, g[f'a_gW_b{beta}'], b['gW_bound'], beta=beta)


@pytest.mark.parametrize('attr', ['W', 'H'])
def test_golden_g19_sparsity_proj(dev, attr):
    """(b): SparsityProj over sparse_beta_div reproduces the reference's run over beta_div(m(), V.to_dense(), 2): the lr
    sequence exactly (the fixture is screened: every line-search decision has a margin three orders above fp32 rounding),
    the factors within the project's 1e-4 bar."""
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import SparsityProj
    g = load_golden('g19_sparse_autograd')
    T, _ = _g19_target(g, dev)
    m = NMF(W=torch.from_numpy(g['W0']), H=torch.from_numpy(g['H0'])).to(dev)
    opt = SparsityProj([getattr(m, attr)], 0.3)

    def closure():
        opt.zero_grad()
        return sparse_beta_div(m.H, m.W, T, 2)
    lrs = []
    for step in range(1, 11):
        loss = opt.step(closure)
        lrs.append(opt.param_groups[0]['lr'])
        if step in (1, 10):
            ew = rel_err(m.W.data.cpu(), g[f'b_{attr}_W{step}'])
            eh = rel_err(m.H.data.cpu(), g[f'b_{attr}_H{step}'])
            record(f'sparse_autograd_g19_sparsity_proj[{attr}-{step}]', W=ew, H=eh)
            assert ew < TOL_FACTORS and eh < TOL_FACTORS, (step, ew, eh)
    assert lrs == list(g[f'b_{attr}_lr']), (lrs, list(g[f'b_{attr}_lr']))
    assert loss.device.type == 'cuda' and loss.dim() == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1, 2])
def test_sgd_lowers_the_loss(dev, beta):
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    H0, W0 = _factors('small', 5)
    T = _target('small', dev)
    m = NMF(W=W0.clone(), H=H0.clone()).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = sparse_beta_div(m.H, m.W, T, beta)
        loss.backward()
        opt.step()
        with torch.no_grad():
            for p in m.parameters():
                p.clamp_(min=0)
        losses.append(float(loss))
    with torch.no_grad():
        losses.append(float(sparse_beta_div(m.H, m.W, T, beta)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_frozen_w_float64_module_no_grad_and_raw_tensor(dev, monkeypatch):
    from torchnmf_amd import sparse_autograd as SA
    from torchnmf_amd.metrics import sparse_beta_div
    from torchnmf_amd.nmf import NMF
    H0, W0 = _factors('small', 5)
    T = _target('small', dev)
    sides = []
    orig = SA._backward_side

    def tap(owner, panel, small, T_, side, *a, **k):
        sides.append(side)
        return orig(owner, panel, small, T_, side, *a, **k)
    monkeypatch.setattr(SA, '_backward_side', tap)
    # a frozen W gets no gradient and launches no W side
    m = NMF(W=W0.clone(), H=H0.clone(), trainable_W=False).to(dev)
    sparse_beta_div(m.H, m.W, T, 1).backward()
    assert sides == ['h'] and m.W.grad is None and m.H.grad is not None
    _, gH, _ = _run(T, H0, W0, 1, dev)
    assert torch.equal(m.H.grad, gH)
    # a float64 module: fp32 work, gradients cast back
    m64 = NMF(W=W0.clone(), H=H0.clone()).double().to(dev)
    loss64 = sparse_beta_div(m64.H, m64.W, T, 2)
    loss64.backward()
    _, gH2, gW2 = _run(T, H0, W0, 2, dev)
    assert loss64.dtype == torch.float32 and m64.H.grad.dtype == torch.float64 and m64.W.grad.dtype == torch.float64
    assert torch.equal(m64.H.grad.float(), gH2) and torch.equal(m64.W.grad.float(), gW2)
    # no_grad records nothing; neither does a call whose factors do not require grad
    sides.clear()
    with torch.no_grad():
        quiet = sparse_beta_div(m.H, m.W, T, 1)
    plain = sparse_beta_div(H0.to(dev), W0.to(dev), T, 1)
    assert quiet.grad_fn is None and not quiet.requires_grad and plain.grad_fn is None and sides == []
    assert torch.equal(quiet, plain)
    # a sparse tensor in place of the prepared target builds one for the call
    idx, vals, shape = _pattern('small')
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).to(dev)
    assert torch.equal(sparse_beta_div(H0.to(dev), W0.to(dev), V, 1), plain)


def test_sparse_fit_still_raises_and_points_here(dev):
    from torchnmf_amd.nmf import NMF
    idx, vals, shape = _pattern('small')
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), shape).to(dev)
    m = NMF(shape, 4).to(dev)
    with pytest.raises(NotImplementedError, match='SparsityProj.*sparse_beta_div'):
        m.sparse_fit(V, sW=0.4)
