"""Fold-in by coordinate descent on the device (csrc/nmfmu_fold_in_cd.hip, ``fold_in_cd(solver='ccd' | 'hals')``,
``NMF.transform_cd``): one iteration per element against float64 under the bound counted in
tests/fold_in_cd_emulation.py (no element left out), the bitwise properties the kernel promises, the per-row stop rule on the
device's own states, ten iterations against the float64 model and against the chained sweeps the project already has, the
descent of the float64 objective along the device's states, the end-to-end route, and the checks that need the data.

Targets, those of tests/test_gpu_fold_in.py: (a) 37 x 29, row counts cycling 0, 1, 4, 5, 8, 9, 20 -- with the thresholds forced
small (W rows staged up to a share of 8, the workgroup above 16 entries) rows that are staged, rows that gather, and a
four-wave row; (b) 9 x 700 with rows of 0, 1, 63, 64, 65, 130, 300, 513 and 700 entries -- slot edges, and at every rank
one-wave and four-wave rows, staged and gathering (default thresholds: the workgroup above 128 / 69 / 21 / 6 entries at
rank 3 / 33 / 100 / 256).  (c) one row of 15 700 entries at rank 3: more than the wave's LDS holds residuals for.

Measured on an MI355X: see DESIGN.md section 28.
"""
import functools

import numpy as np
import pytest
import torch

import fold_in_cd_emulation as E
import fold_in_emulation as F
import masked_emulation as M
from conftest import record, rel_err

pytestmark = pytest.mark.gpu

RANKS = [3, 33, 100, 256]
MODES = ['missing', 0.0625, 0.3, 'zero']
ALPHA, L1_RATIO = 0.07, 0.3
REG = (ALPHA * L1_RATIO, ALPHA * (1 - L1_RATIO))
SMALL = dict(_block=8, _long_rows=16)
TOL = 1e-4                            # the project's bar for factors after a run
GARBAGE = -7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(which, R):
    """(idx, vals, W0, H0, shape, (ptr, cols, vals))"""
    if which == 'a':
        p = M.make_problem(37, 29, R, 0) + ((37, 29),)
    elif which == 'b':
        p = F.make_wide(R) + ((9, 700),)
    else:
        g = np.random.default_rng(77 + R)
        C, counts = 15700, (15700, 40, 0)
        rows = np.repeat(np.arange(3), counts)
        cols = np.concatenate([np.sort(g.choice(C, size=k, replace=False)) for k in counts]).astype(np.int64)
        p = (np.stack([rows, cols]), (g.random(len(cols)) * 1.9 + 0.1).astype(np.float32),
             (g.random((C, R)) * 0.9 + 0.1).astype(np.float32), (g.random((3, R)) * 0.9 + 0.1).astype(np.float32), (3, C))
    return p + (E.work_list(p[0], p[1], p[4]),)


def _solver(mode):
    return 'hals' if mode == 'zero' else 'ccd'


def _sparse(idx, vals, shape, dev):
    return torch.sparse_coo_tensor(torch.from_numpy(np.asarray(idx)), torch.from_numpy(np.asarray(vals)), shape).to(dev)


def _fold(dev, prob, mode, reg=False, max_iter=1, tol=0.0, H0=None, target=None, **kw):
    from torchnmf_amd.fold_in import fold_in_cd as fold_in
    idx, vals, W0, H00, shape = prob[:5]
    Wd = torch.from_numpy(W0).to(dev)
    Hd = torch.from_numpy(H00).to(dev) if H0 is None else H0
    V = _sparse(idx, vals, shape, dev) if target is None else target
    keepW, keepH = Wd.clone(), Hd.clone()
    H, cnt = fold_in(Wd, V, 2, max_iter, tol, ALPHA if reg else 0, L1_RATIO if reg else 0, unstored=mode, solver=_solver(mode),
                     H0=Hd, return_n_iter=True, _fill=GARBAGE, **kw)
    assert torch.equal(Wd, keepW) and torch.equal(Hd, keepH)           # W and the caller's H0 are bitwise unchanged
    assert H.dtype == torch.float32 and cnt.dtype == torch.int32 and H.shape == Hd.shape and cnt.shape == (shape[0],)
    assert not H.requires_grad
    return H, cnt


@functools.lru_cache(maxsize=None)
def _gram(which, R):
    """W^T W as the kernel reads it: ``nmfmu_gram`` on the device (what ``fold_in`` calls; a repeated call is bitwise
    identical), as a numpy fp32 matrix."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    Wd = torch.from_numpy(_problem(which, R)[2]).cuda()
    G = torch.empty(R * R, dtype=torch.float32, device='cuda')
    part = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device='cuda')
    _capi.check(lib.nmfmu_gram(Wd.data_ptr(), Wd.shape[0], R, part.data_ptr(), G.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), 'nmfmu_gram')
    return G.reshape(R, R).cpu().numpy()


def _check_one(dev, which, R, mode, reg, kw):
    prob = _problem(which, R)
    W0, H0, shape, (ptr, cols, vals) = prob[2], prob[3], prob[4], prob[5]
    omega = E.omega_of(mode)
    l1, l2 = REG if reg else (0.0, 0.0)
    H, cnt = _fold(dev, prob, mode, reg, **kw)
    err, bound = E.sweep_check(H.double().cpu().numpy(), H0, W0, None if omega == 0 else _gram(which, R), ptr, cols, vals,
                               omega, l1, l2, long_rows=kw.get('_long_rows'))
    frac = E.fraction(err, bound)
    assert frac.shape == (shape[0], R)                                  # no element left out
    worst = float(frac.max())
    info = dict(mode=mode, R=R, target=which, reg=reg, small=bool(kw))
    record('fold_in_cd_iteration', worst_fraction_of_bound=worst, **info)
    print(f'fold_in_cd_iteration {info}: worst |got - want| / bound = {worst:.3f}')
    assert bool((cnt == 1).all()) and bool(torch.isfinite(H).all())
    assert worst <= 1.0, (info, worst)
    empty = np.diff(ptr) == 0
    assert empty.any()
    if omega == 0:                                                      # nothing measured: H0 exactly
        assert torch.equal(H.cpu()[torch.from_numpy(empty)], torch.from_numpy(H0)[torch.from_numpy(empty)])
    elif not reg:                                                       # swept: the Gram term takes the row to the floor
        assert bool((H.cpu()[torch.from_numpy(empty)] == E.EPS).all())


# ---- 1. one iteration, per element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('mode', MODES)
def test_one_iteration_per_element(dev, mode, R):
    for reg in (False, True):
        for which, kw in (('a', {}), ('a', SMALL), ('b', {})):
            _check_one(dev, which, R, mode, reg, kw)


@pytest.mark.parametrize('mode', MODES)
def test_one_iteration_of_a_row_beyond_the_lds(dev, mode):
    """15 700 entries at rank 3: a share of 3 925 per wave against 2 364 floats of LDS -- no residuals kept (the same bound:
    the residual formed anew carries fewer roundings).  Three iterations in one call are three chained calls here too."""
    assert -(-15700 // E.WAVES) > E.avail(3)
    for reg in (False, True):
        _check_one(dev, 'c', 3, mode, reg, {})
    prob = _problem('c', 3)
    h = torch.from_numpy(prob[3]).to(dev)
    for _ in range(3):
        h = _fold(dev, prob, mode, H0=h)[0]
    assert torch.equal(h, _fold(dev, prob, mode, max_iter=3)[0])


# ---- 2. bitwise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [33, 256])
@pytest.mark.parametrize('mode', MODES)
def test_bitwise_properties(dev, mode, R):
    from torchnmf_amd.metrics import SparseTarget
    K = 5
    for which in ('a', 'b'):
        prob = _problem(which, R)
        idx, vals, W0, H0, shape = prob[:5]
        V = _sparse(idx, vals, shape, dev)
        for reg in (False, True):
            H, cnt = _fold(dev, prob, mode, reg, K)
            assert bool((cnt == K).all()) and bool(torch.isfinite(H).all())       # (the garbage the counts held is gone)
            H2, cnt2 = _fold(dev, prob, mode, reg, K)
            assert torch.equal(H, H2) and torch.equal(cnt, cnt2)                                   # a repeated call
            assert torch.equal(H, _fold(dev, prob, mode, reg, K, _block=8)[0])                     # staged or gathered ...
            Hs = _fold(dev, prob, mode, reg, K, **SMALL)[0]
            assert torch.equal(Hs, _fold(dev, prob, mode, reg, K, _long_rows=16)[0])               # ... at either threshold
            assert torch.equal(H, _fold(dev, prob, mode, reg, K, target=SparseTarget(V))[0])       # tensor / SparseTarget
            # K iterations in one call are K chained one-iteration calls
            for kw, full in (({}, H), (SMALL, Hs)):
                h = torch.from_numpy(H0).to(dev)
                for _ in range(K):
                    h = _fold(dev, prob, mode, reg, 1, H0=h, **kw)[0]
                assert torch.equal(h, full)
            # a shuffled subset of the rows: the same bits per row
            g = np.random.default_rng(R + shape[0])
            pick = g.permutation(shape[0])[: max(3, 2 * shape[0] // 3)]
            sub_rows = np.concatenate([np.full(int((idx[0] == r).sum()), i) for i, r in enumerate(pick)]).astype(np.int64)
            sel = np.concatenate([np.flatnonzero(idx[0] == r) for r in pick]).astype(np.int64)
            sub = (np.stack([sub_rows, idx[1][sel]]), vals[sel], W0, H0[pick], (len(pick), shape[1]))
            for kw, full in (({}, H), (SMALL, Hs)):
                assert torch.equal(_fold(dev, sub, mode, reg, K, **kw)[0], full[torch.from_numpy(pick).to(dev)])
        # max_iter = 0: H0, no iteration counted
        H, cnt = _fold(dev, prob, mode, False, 0)
        assert torch.equal(H.cpu(), torch.from_numpy(H0)) and bool((cnt == 0).all())


def test_target_without_entries(dev):
    W0, H0, shape = _problem('a', 33)[2:5]
    prob = (np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.float32), W0, H0, shape)
    H, cnt = _fold(dev, prob, 'missing', max_iter=3)
    assert torch.equal(H.cpu(), torch.from_numpy(H0)) and bool((cnt == 3).all())
    H, cnt = _fold(dev, prob, 'missing', max_iter=3, tol=1e-4)
    assert torch.equal(H.cpu(), torch.from_numpy(H0)) and bool((cnt == 1).all())       # the stop rule on the unchanged rows
    for mode in (0.3, 'zero'):
        H, cnt = _fold(dev, prob, mode, max_iter=3, tol=1e-4)
        assert bool((H == E.EPS).all()) and bool((cnt == 2).all())                     # to the floor, then no change


# ---- 3. the stop rule ------------------------------------------------------------------------------------------------------------
STOP_MAX = 30
# Cases where the float64 model (fold_in_cd_emulation.run, 30 iterations) leaves the inputs mixed -- at least a quarter of the
# rows stop early and at least one does not; its early rows of 37 or 9: 32, 12, 15, 22, 19, 27, 19, 18 and 4.  The condition
# is asserted below on the states the device returns.
STOP_CASES = [('a', 3, 0.05, 1e-3), ('a', 33, 0.3, 1e-3), ('a', 33, 0.05, 1e-2), ('a', 200, 0.05, 3e-2), ('a', 33, 'zero', 1e-3),
              ('a', 200, 'zero', 1e-2), ('a', 33, 'missing', 1e-3), ('a', 200, 'missing', 1e-2), ('b', 33, 'zero', 3e-2)]


@pytest.mark.parametrize('kw', [{}, SMALL], ids=['default', 'small'])
@pytest.mark.parametrize('which,R,mode,STOP_TOL', STOP_CASES)
def test_stop_rule(dev, which, R, mode, STOP_TOL, kw):
    prob = _problem(which, R)
    n = prob[4][0]
    sts = [torch.from_numpy(prob[3]).to(dev)]
    for _ in range(STOP_MAX):                                              # the states of tol = 0, one iteration per call
        sts.append(_fold(dev, prob, mode, max_iter=1, H0=sts[-1], **kw)[0])
    assert torch.equal(sts[-1], _fold(dev, prob, mode, max_iter=STOP_MAX, **kw)[0])
    H, cnt = _fold(dev, prob, mode, max_iter=STOP_MAX, tol=STOP_TOL, **kw)
    # the criterion, recomputed in fp32 from the states k - 1 and k
    want = torch.full((n,), STOP_MAX, dtype=torch.int32)
    tol32 = torch.tensor(STOP_TOL, dtype=torch.float32)
    for k in range(STOP_MAX, 0, -1):
        a, b = sts[k - 1].cpu(), sts[k].cpu()
        hit = (b - a).abs().amax(1) <= tol32 * b.amax(1)
        want[hit] = k
    assert np.array_equal(want.numpy(), F.stop_counts([s.cpu().numpy() for s in sts], STOP_TOL))
    early = int((want < STOP_MAX).sum())
    print(f'fold_in_cd_stop {which} R={R} {mode}: counts {sorted(want.tolist())}')
    record('fold_in_cd_stop', target=which, R=R, mode=mode, tol=STOP_TOL, small=bool(kw), early=early, rows=n)
    assert 4 * early >= n and early < n                                    # a condition on the inputs
    assert torch.equal(cnt.cpu(), want)
    for i in range(n):
        assert torch.equal(H[i], sts[int(want[i])][i]), i                  # bitwise the state its count names


# ---- 4. ten iterations: the float64 model, and the chained sweeps of the device ---------------------------------------------------
def _chained(dev, prob, mode, reg, iters):
    """``iters`` H-side sweeps of the route that existed before: ``ccd_sweep`` / ``wccd_sweep`` / ``hals_sweep``."""
    from torchnmf_amd.ccd import ccd_sweep
    from torchnmf_amd.hals import hals_sweep
    from torchnmf_amd.metrics import SparseTarget
    from torchnmf_amd.wccd import wccd_sweep
    idx, vals, W0, H0, shape = prob[:5]
    l1, l2 = REG if reg else (0.0, 0.0)
    V = _sparse(idx, vals, shape, dev)
    Wd, Hd = torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev).clone()
    if mode == 'zero':
        A, G = torch.sparse.mm(V, Wd).contiguous(), (Wd.t() @ Wd).contiguous()
        for _ in range(iters):
            hals_sweep(Hd, A, G, l1, l2)
        return Hd
    T = SparseTarget(V)
    for _ in range(iters):
        if mode == 'missing':
            ccd_sweep(Hd, Wd, T, 'h', l1, l2)
        else:
            wccd_sweep(Hd, Wd, T, 'h', mode, l1, l2)
    return Hd


@pytest.mark.parametrize('mode', MODES)
def test_ten_iterations(dev, mode):
    omega = E.omega_of(mode)
    for which, R in (('a', 33), ('b', 100), ('a', 256)):
        prob = _problem(which, R)
        W0, H0, (ptr, cols, vals) = prob[2], prob[3], prob[5]
        for reg in (False, True):
            l1, l2 = REG if reg else (0.0, 0.0)
            ref, ref_cnt = E.run(H0, W0, ptr, cols, vals, omega, 10, 0.0, l1, l2)
            H, cnt = _fold(dev, prob, mode, reg, 10)
            assert np.array_equal(cnt.cpu().numpy(), ref_cnt)
            e64 = rel_err(H.cpu(), ref)
            edev = rel_err(H.cpu(), _chained(dev, prob, mode, reg, 10).cpu())
            record('fold_in_cd_ten', mode=mode, target=which, R=R, reg=reg, rel_float64=e64, rel_chained=edev, tol=TOL)
            print(f'fold_in_cd_ten {mode} {which} R={R} reg={reg}: float64 {e64:.2e}, chained sweeps {edev:.2e}')
            assert e64 <= TOL and edev <= TOL, (e64, edev)


# ---- 5. descent: the float64 objective of the device's successive states ----------------------------------------------------------
@pytest.mark.parametrize('mode', [0.0625, 0.3, 'zero'])
def test_objective_never_rises(dev, mode):
    """Per row, ``wccd_emulation.row_objective`` on the explicit weight matrix along twelve one-iteration states of the device:
    no rise beyond 1e-5 relative (section 27's bar).  omega = 0 is left out: there the float64 model itself rises by up to
    2e-5 relative on rows whose objective is near zero."""
    omega = E.omega_of(mode)
    for which, R, kw in (('a', 33, {}), ('a', 33, SMALL), ('b', 33, {}), ('a', 256, {})):
        prob = _problem(which, R)
        W0, (ptr, cols, vals) = prob[2], prob[5]
        for reg in (False, True):
            l1, l2 = REG if reg else (0.0, 0.0)
            h = torch.from_numpy(prob[3]).to(dev)
            obj = [E.objectives(prob[3], W0, ptr, cols, vals, omega, l1, l2)]
            for _ in range(12):
                h = _fold(dev, prob, mode, reg, 1, H0=h, **kw)[0]
                obj.append(E.objectives(h.double().cpu().numpy(), W0, ptr, cols, vals, omega, l1, l2))
            obj = np.stack(obj)
            rise = float(((obj[1:] - obj[:-1]) / obj[:-1]).max())
            record('fold_in_cd_descent', mode=mode, target=which, R=R, reg=reg, small=bool(kw), worst_relative_rise=rise)
            print(f'fold_in_cd_descent {mode} {which} R={R} reg={reg} small={bool(kw)}: worst relative rise {rise:.2e}')
            assert rise <= 1e-5, rise
            assert bool((obj[-1] < obj[0]).all())


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def test_fit_transform_topk(dev):
    from torchnmf_amd.metrics import topk_scores
    from torchnmf_amd.nmf import NMF
    idx, vals, W0, H0, shape = _problem('a', 33)[:5]
    V = _sparse(idx, vals, shape, dev)
    m = NMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    m.fit(V, beta=2, max_iter=20, solver='ccd', unstored=0.05)
    keep = {k: v.detach().clone() for k, v in m.named_parameters()}
    new_rows = np.array([5, 6, 13, 20, 0])                                 # "new users": rows of the target, one without entries
    sel = np.concatenate([np.flatnonzero(idx[0] == r) for r in new_rows])
    sub_rows = np.concatenate([np.full(int((idx[0] == r).sum()), i) for i, r in enumerate(new_rows)])
    V_new = _sparse(np.stack([sub_rows, idx[1][sel]]), vals[sel], (len(new_rows), shape[1]), dev)
    g = torch.Generator(device=dev).manual_seed(3)
    H, cnt = m.transform_cd(V_new, 2, solver='ccd', unstored=0.05, generator=g, return_n_iter=True)
    assert all(torch.equal(v, keep[k]) for k, v in m.named_parameters())
    assert H.dtype == torch.float32 and H.shape == (5, 33) and not H.requires_grad and bool((H >= E.EPS).all())
    assert bool((cnt >= 1).all()) and bool((cnt <= 200).all()) and bool((H[4] == E.EPS).all())
    # the default start is |N(0, 1)| from the generator, used as it is
    start = torch.randn(5, 33, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).abs_()
    H_again, cnt_again = m.transform_cd(V_new, 2, solver='ccd', unstored=0.05, H0=start, return_n_iter=True)
    assert torch.equal(H, H_again) and torch.equal(cnt, cnt_again)
    # under the objective the model was trained on, every row ends below its start
    ptr, cols, v = E.work_list(np.stack([sub_rows, idx[1][sel]]), vals[sel], (5, shape[1]))
    Wn = m.W.data.double().cpu().numpy()
    o_new = E.objectives(H.double().cpu().numpy(), Wn, ptr, cols, v, 0.05)
    o_start = E.objectives(start.double().cpu().numpy(), Wn, ptr, cols, v, 0.05)
    assert bool((o_new < o_start).all()), (o_new, o_start)
    top = topk_scores(H, m.W.data, 5, exclude=V_new)
    stored = set(zip(sub_rows.tolist(), idx[1][sel].tolist()))
    ind = top.indices.cpu().numpy()
    assert ind.shape == (5, 5) and ind.min() >= 0
    assert not any((i, int(j)) in stored for i in range(5) for j in ind[i])
    # a double module: float64 out, the fp32 result's values
    md = NMF(W=m.W.data.cpu(), rank=33).double().to(dev)
    Hd = md.transform_cd(V_new, 2, solver='ccd', unstored=0.05, generator=torch.Generator(device=dev).manual_seed(3))
    assert Hd.dtype == torch.float64 and torch.equal(Hd, H.double())
    for kw in (dict(solver='ccd', unstored='missing'), dict(solver='hals', unstored='zero')):
        Hk = m.transform_cd(V_new, 2, max_iter=5, **kw)
        assert Hk.shape == (5, 33) and bool(torch.isfinite(Hk).all()) and bool((Hk >= 0).all())


# ---- 7. the checks of fold_in that read the data (behind the device check: they cannot run on CPU tensors) ------------------------
def test_data_checks(dev):
    from torchnmf_amd.fold_in import fold_in_cd as fold_in
    W = torch.rand(9, 4, device=dev)
    ij = torch.tensor([[0, 1, 2], [2, 3, 5]])

    def sp(*v):
        return torch.sparse_coo_tensor(ij, torch.tensor(v), (3, 9)).to(dev)
    bad_h0 = -torch.ones(3, 4, device=dev)
    for kw in (dict(solver='ccd', unstored='missing'), dict(solver='ccd', unstored=0.05), dict(solver='hals', unstored='zero')):
        with pytest.raises(AssertionError, match='Target should be non-negative'):
            fold_in(W, sp(1.0, -1.0, 0.0), 2, H0=bad_h0, **kw)                  # the target first
        with pytest.raises(AssertionError, match='Target should be non-negative'):
            fold_in(W, sp(1.0, float('nan'), 0.0), 2, **kw)
        with pytest.raises(AssertionError, match='should be non-negative'):
            fold_in(W, sp(1.0, 2.0, 0.5), 2, H0=bad_h0, **kw)
        with pytest.raises(AssertionError, match='should be non-negative'):
            fold_in(W, sp(1.0, 2.0, 0.5), 2, H0=bad_h0, max_iter=0, **kw)
        H = fold_in(W, sp(1.0, 2.0, 0.0), 2, max_iter=2, **kw)                  # a stored zero: admitted
        assert bool(torch.isfinite(H).all())
