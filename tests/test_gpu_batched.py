"""Batched NMF on the device (csrc/nmfmu_bmu.hip, batched.BatchedNMF, ``NMF.fit_restarts``): terms, step and loss of every
problem per element against the float64 model under the bounds counted in tests/batched_emulation.py (no element left out),
independence of a problem from the batch around it, the shared target, inactive problems, the stop rule on the device, the
reference's own ``NMF.fit`` runs (golden g24), agreement with the weighted exact-fp32 path, restarts and behaviour.

The kernel's tile is the weighted kernel's (128 owner rows, stages of 32 contraction steps), so the per-element shapes are
that test's: 131 x 70 (a row tile plus 3 rows, two stages plus 6 columns, rows not 16-byte aligned: the scalar loads; the W
side sees 70 owner rows over 4 stages plus 3) and 132 x 72 (the 16-byte loads, tails of 4 and 8); the split count is forced to
1, 2 and 3.  Three distinct problems per call.

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 31.
"""
import functools

import numpy as np
import pytest
import torch

import batched_emulation as BE
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(131, 70), (132, 72)]
RANKS = [3, 33, 100, 200]             # r_pad 32 / 64 / 128 / 256 (the last: two rank tiles)
BETAS = [-1, 0, 0.5, 1, 2, 3]
SPLITS = [1, 2, 3]
REG = (0.07 * 0.3, 0.07 * 0.7)
TOL = 1e-4                            # the project's bar for factors after a recorded run
NAN = float('nan')
NAN_BITS = 0x7fc00abc                 # a NaN with a payload: an untouched word keeps it


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problems(B, N, C, R):
    return BE.make_problems(B, N, C, R)


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (name, info)
    err = BE.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


def _bits(t):
    return t.contiguous().view(torch.int32)


def _v_term(V, beta, dev):
    """The float64 model's terms of v alone, and the device's (nmfmu_bmu_v_term) beside them: every term is one double
    expression of v (log or pow: 1 ulp) summed in double over n entries, so the two agree within (n + 2) 2^-53 sum |terms|."""
    from torchnmf_amd import batched
    B, N, C = V.shape
    ref = np.array([BE.v_term(V[b], beta) for b in range(B)])
    Vd = torch.from_numpy(V).to(dev)
    got = batched._v_terms(Vd, N * C, B, float(beta)).cpu().numpy()
    v = V.astype(np.float64)
    mag = {1: np.abs(v * np.log(v + BE.EPS)) + v, 0: np.abs(np.log(v + BE.EPS)) + 1.0, 2: 0 * v}.get(
        beta, np.power(v + BE.EPS if beta < 0 else v, beta)).sum(axis=(1, 2))
    assert np.all(np.abs(got - ref) <= (N * C + 2) * 2.0 ** -53 * mag), (beta, got, ref)
    one = batched._v_terms(Vd[1], 0, B, float(beta)).cpu().numpy()          # a shared target: summed once, the same bits
    assert one.tolist() == [got[1]] * B
    return torch.from_numpy(ref).to(dev)


# ---- per element against the float64 model -------------------------------------------------------------------------------------
@pytest.mark.parametrize('nsplit', SPLITS)
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('shape', SHAPES)
def test_terms_step_loss_per_element(dev, shape, beta, R, nsplit):
    from torchnmf_amd import _capi, batched
    N, C = shape
    B = 3
    lib = _capi.load()
    r_pad = lib.nmfmu_pad_rank(R)
    V, W0, H0 = _problems(B, N, C, R)
    info = dict(shape=f'{N}x{C}', beta=beta, R=R, nsplit=nsplit)
    Vd, Wd, Hd = _dev(dev, V, W0, H0)
    assert (Vd.data_ptr() % 16 == 0) and ((C % 4 == 0) == (shape == (132, 72)))      # which load path runs
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        rows, contraction = (N, C) if side == 'h' else (C, N)
        assert lib.nmfmu_bmu_ws(B, rows, contraction, r_pad, nsplit) == BE.workspace_floats(B, rows, contraction, r_pad, nsplit)
        # terms: every element of both planes is written (they and the workspace start as NaN), padded columns exactly 0
        num, den = batched._bmu_call(Vd, N * C, side, owner, panel, float(beta), nsplit=nsplit, _fill=NAN)
        assert num.shape == den.shape == (B, rows, r_pad)
        assert bool((num[:, :, R:] == 0).all()) and bool((den[:, :, R:] == 0).all())
        refs = [BE.terms(V[b], H0[b], W0[b], beta, side, nsplit) for b in range(B)]
        assert all(r['parts'] == nsplit for r in refs)
        for b in range(B):
            _check('batched_terms_num', num[b, :, :R], refs[b]['num'], refs[b]['num_bound'], side=side, problem=b, **info)
            _check('batched_terms_den', den[b, :, :R], refs[b]['den'], refs[b]['den_bound'], side=side, problem=b, **info)
        # step, without and with regularisers, on a copy of the owner; the panel is bitwise unchanged
        for l1, l2 in ((0.0, 0.0), REG):
            f = owner.clone()
            before = panel.clone()
            batched._bmu_call(Vd, N * C, side, f, panel, float(beta), step=(l1, l2, BE.gamma_of(beta)), nsplit=nsplit,
                              _fill=NAN)
            for b in range(B):
                new_ref, bound, _ = BE.step(V[b], H0[b], W0[b], beta, side, l1, l2, nsplit)
                _check('batched_step', f[b], new_ref, bound, side=side, reg=l1 > 0, problem=b, **info)
            assert torch.equal(panel, before)
    nparts = lib.nmfmu_bmu_loss_parts(N, C)
    assert nparts == BE.loss_parts(N, C)
    part = torch.full((B * nparts,), NAN, dtype=torch.float64, device=dev)
    out = torch.full((B,), NAN, dtype=torch.float64, device=dev)
    got = batched._bmu_loss(Hd, Wd, Vd, N * C, float(beta), _v_term(V, beta, dev), part=part, out=out)
    assert got.dtype == torch.float64 and got.shape == (B,)
    for b in range(B):
        ref_loss, loss_bound = BE.loss(V[b], H0[b], W0[b], beta)
        _check('batched_loss', got[b].reshape(()), ref_loss, loss_bound, problem=b, **info)


# ---- a problem does not see the batch around it ------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_a_problem_is_independent_of_its_batch(dev, beta):
    """Every problem of a B = 5 call is bitwise the same problem in a B = 1 call: terms, one step, a 30-iteration fit with its
    count; reordering the problems permutes the results.  ``tol`` is set per beta from the float64 model
    (batched_emulation.fit on these problems) so that the problems do NOT all stop together: at iteration 20 the model's
    (previous - loss) / loss_init is 0.00929 for problem 1 and 0.0095 - 0.0097 for the others at beta 0.5, 0.01267 - 0.01288
    for problems 1, 2, 3 and 0.01315 / 0.01321 for 0 and 4 at beta 1, 0.00522 for problem 2 and 0.0054 - 0.0055 for the
    others at beta 2; every chosen ``tol`` is at least 0.9 % away from the nearest of them, ten thousand times what fp32
    rounding moves the loss."""
    from torchnmf_amd import batched
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 5, 131, 70, 33
    V, W0, H0 = _problems(B, N, C, R)
    Vd, Wd, Hd = _dev(dev, V, W0, H0)
    reg = (*REG, BE.gamma_of(beta))
    num, den = batched._bmu_call(Vd, N * C, 'h', Hd, Wd, float(beta))
    stepped = Wd.clone()
    batched._bmu_call(Vd, N * C, 'w', stepped, Hd, float(beta), step=reg)

    def fit(Vx, Wx, Hx, **kw):
        m = BatchedNMF(W=Wx, H=Hx).to(dev)
        n = m.fit(Vx, beta=beta, tol=tol, max_iter=30, alpha=0.07, l1_ratio=0.3, **kw)
        return m.W.data.clone(), m.H.data.clone(), n, m.last_loss.clone()
    tol, counts = {0.5: (0.0094, [30, 20, 30, 30, 30]), 1: (0.0130, [30, 20, 20, 20, 30]),
                   2: (0.0053, [30, 30, 20, 30, 30])}[beta]
    Wf, Hf, nf, lf = fit(Vd, Wd.cpu(), Hd.cpu())
    assert nf.tolist() == counts
    assert nf.dtype == torch.int64 and nf.device.type == 'cpu' and lf.dtype == torch.float64
    print(f'independence beta {beta}: counts {nf.tolist()}')
    for b in range(B):
        one = slice(b, b + 1)
        n1, d1 = batched._bmu_call(Vd[one].contiguous(), N * C, 'h', Hd[one].contiguous(), Wd[one].contiguous(), float(beta))
        assert torch.equal(_bits(n1[0]), _bits(num[b])) and torch.equal(_bits(d1[0]), _bits(den[b]))
        s1 = Wd[one].clone()
        batched._bmu_call(Vd[one].contiguous(), N * C, 'w', s1, Hd[one].contiguous(), float(beta), step=reg)
        assert torch.equal(_bits(s1[0]), _bits(stepped[b]))
        W1, H1, n1, l1 = fit(Vd[one].contiguous(), Wd[one].cpu(), Hd[one].cpu())
        assert torch.equal(_bits(W1[0]), _bits(Wf[b])) and torch.equal(_bits(H1[0]), _bits(Hf[b]))
        assert int(n1[0]) == int(nf[b]) and torch.equal(l1[0], lf[b])
    perm = torch.tensor([3, 0, 4, 2, 1])
    Wp, Hp, npm, lp = fit(Vd[perm.to(dev)].contiguous(), Wd.cpu()[perm], Hd.cpu()[perm])
    assert torch.equal(_bits(Wp), _bits(Wf[perm.to(dev)])) and torch.equal(_bits(Hp), _bits(Hf[perm.to(dev)]))
    assert torch.equal(npm, nf[perm]) and torch.equal(lp, lf[perm.to(dev)])


@pytest.mark.parametrize('shape', SHAPES)
def test_shared_target(dev, shape):
    """fit(V2d) -- v_batch_stride 0 -- is bitwise fit of the same target repeated B times."""
    from torchnmf_amd.batched import BatchedNMF
    N, C = shape
    B, R = 4, 33
    V, W0, H0 = _problems(B, N, C, R)
    Vd, = _dev(dev, V[1])
    runs = []
    for target in (Vd, Vd.expand(B, N, C).contiguous()):
        m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
        n = m.fit(target, beta=1, tol=3e-3, max_iter=30)
        runs.append((m.W.data.clone(), m.H.data.clone(), n, m.last_loss.clone(), m.loss(target, 1)))
        assert m.last_precision == 'fp32'
    a, b = runs
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[3], a[4])
    assert not torch.equal(a[0][0], a[0][1])                    # different starts went different ways


# ---- inactive problems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nsplit', [1, 2])
def test_inactive_problems_are_not_touched(dev, nsplit):
    from torchnmf_amd import _capi, batched
    lib = _capi.load()
    B, N, C, R = 3, 131, 70, 33
    beta = 0.5
    r_pad = lib.nmfmu_pad_rank(R)
    V, W0, H0 = _problems(B, N, C, R)
    Vd, Wd, Hd = _dev(dev, V, W0, H0)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    reg = (*REG, BE.gamma_of(beta))
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        rows, contraction = (N, C) if side == 'h' else (C, N)
        n_ws = lib.nmfmu_bmu_ws(B, rows, contraction, r_pad, nsplit)
        per = n_ws // B
        full = owner.clone()
        batched._bmu_call(Vd, N * C, side, full, panel, beta, step=reg, nsplit=nsplit)
        ws = torch.full((n_ws,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        f = owner.clone()
        batched._bmu_call(Vd, N * C, side, f, panel, beta, step=reg, nsplit=nsplit, active=active, _ws=ws)
        assert torch.equal(_bits(f[1]), _bits(owner[1]))                              # its factors
        assert bool((_bits(ws[per:2 * per]) == NAN_BITS).all())                        # its slab slice
        assert not bool((_bits(ws[:per]) == NAN_BITS).any()) and not bool((_bits(ws[2 * per:]) == NAN_BITS).any())
        for b in (0, 2):
            assert torch.equal(_bits(f[b]), _bits(full[b]))
        # terms: the planes of the inactive problem keep what they held
        num, den = batched._bmu_call(Vd, N * C, side, owner, panel, beta, nsplit=nsplit, active=active, _fill=NAN)
        num_all, den_all = batched._bmu_call(Vd, N * C, side, owner, panel, beta, nsplit=nsplit)
        assert bool(torch.isnan(num[1]).all()) and bool(torch.isnan(den[1]).all())
        for b in (0, 2):
            assert torch.equal(_bits(num[b]), _bits(num_all[b])) and torch.equal(_bits(den[b]), _bits(den_all[b]))
    vt = _v_term(V, beta, dev)
    all_ = batched._bmu_loss(Hd, Wd, Vd, N * C, beta, vt)
    out = torch.tensor([7.0, -3.25, 7.0], dtype=torch.float64, device=dev)
    batched._bmu_loss(Hd, Wd, Vd, N * C, beta, vt, active=active, out=out)
    assert float(out[1]) == -3.25 and torch.equal(out[0], all_[0]) and torch.equal(out[2], all_[2])


def test_judge_on_the_device(dev):
    """bmu_judge_kernel against its Python statement: the hand-made cases (a stop, a NaN loss, an already stopped problem)
    repeated over 600 problems -- more than one trip of the workgroup's 256 threads."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    reps = 120
    div = np.tile([2.0, 0.5, -1e-9, 8.0, 0.5], reps)
    loss_init = np.tile([4.0, 2.0, 3.0, 4.0, 2.0], reps)
    previous = np.tile([2.002, 1.5, 3.0, 4.0, 1.0], reps)
    active = np.tile(np.array([1, 1, 1, 1, 0], dtype=np.int32), reps)
    n_iter = np.full(5 * reps, 80, dtype=np.int64)
    d_div, d_init, d_prev, d_act, d_n = _dev(dev, div, loss_init, previous, active, n_iter)
    d_alive = torch.full((1,), -1, dtype=torch.int32, device=dev)
    for iteration, change in ((19, None), (29, 4.5)):
        if change is not None:
            div[2::5] = change
            d_div[2::5] = change
        alive = BE.judge(div, loss_init, previous, 1e-3, iteration, active, n_iter)
        _capi.check(lib.nmfmu_bmu_judge(5 * reps, d_div.data_ptr(), d_init.data_ptr(), d_prev.data_ptr(), 1e-3, iteration,
                                        d_act.data_ptr(), d_n.data_ptr(), d_alive.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), 'nmfmu_bmu_judge')
        assert int(d_alive[0]) == alive and d_act.cpu().numpy().tolist() == active.tolist()
        assert d_n.cpu().numpy().tolist() == n_iter.tolist()
        assert np.array_equal(d_prev.cpu().numpy(), previous, equal_nan=True)
    assert alive == reps and n_iter[:5].tolist() == [20, 30, 80, 20, 80]


# ---- the reference's recorded runs ----------------------------------------------------------------------------------------------
G24 = load_golden('g24_batched_fit')


@pytest.mark.parametrize('case', [str(c) for c in G24['cases']])
def test_golden_g24(dev, case):
    """All six problems in one call: every count is the reference's, every problem's factors meet the project's bar, and a
    problem that stopped early holds bitwise what a call with max_iter = its count returns."""
    from torchnmf_amd.batched import BatchedNMF
    g = G24
    beta, alpha, l1_ratio, update_W = (float(x) for x in g[case + '_par'])
    tol, max_iter = float(g['tol']), int(g['max_iter'])
    V, = _dev(dev, g['V'])

    def run(sel, tol_, max_iter_):
        m = BatchedNMF(W=torch.from_numpy(g['W0'][sel]), H=torch.from_numpy(g['H0'][sel]), trainable_W=bool(update_W)).to(dev)
        n = m.fit(V[sel].contiguous(), beta=beta, tol=tol_, max_iter=max_iter_, alpha=alpha, l1_ratio=l1_ratio)
        return m, n
    m, n = run(slice(0, 6), tol, max_iter)
    want = g[case + '_n_iter']
    print(f'batched_g24 {case}: counts {n.tolist()} (reference {want.tolist()})')
    assert n.tolist() == want.tolist() and m.last_precision == 'fp32'
    worst = 0.0
    for b in range(6):
        ew, eh = rel_err(m.W.data[b].cpu(), g[case + '_W'][b]), rel_err(m.H.data[b].cpu(), g[case + '_H'][b])
        el = abs(float(m.last_loss[b]) - float(g[case + '_div'][b])) / abs(float(g[case + '_div'][b]))
        record('batched_g24', case=case, problem=b, W=ew, H=eh, loss=el)
        print(f'batched_g24 {case} problem {b}: W {ew:.2e} H {eh:.2e} loss {el:.2e}')
        worst = max(worst, ew, eh)
        assert ew < TOL and eh < TOL, (case, b, ew, eh)
    record('batched_g24_worst', case=case, worst=worst)
    if not update_W:
        assert torch.equal(m.W.data.cpu(), torch.from_numpy(g['W0']))
    early = [b for b in range(6) if want[b] < max_iter]
    assert early
    for b in early:
        mk, nk = run(slice(b, b + 1), -1e9, int(want[b]))
        assert nk.tolist() == [want[b]]
        assert torch.equal(_bits(mk.W.data[0]), _bits(m.W.data[b])) and torch.equal(_bits(mk.H.data[0]), _bits(m.H.data[b]))
        assert torch.equal(mk.last_loss[0], m.last_loss[b])


# ---- against the existing exact-fp32 path -------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_agrees_with_the_weighted_fit_at_unit_weights(dev, beta):
    from torchnmf_amd.batched import BatchedNMF
    from torchnmf_amd.nmf import NMF
    B, N, C, R = 3, 131, 70, 33
    V, W0, H0 = _problems(B, N, C, R)
    Vd, = _dev(dev, V)
    m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    assert m.fit(Vd, beta=beta, tol=-1e9, max_iter=20).tolist() == [20] * B
    ones = torch.ones(N, C, device=dev)
    for b in range(B):
        one = NMF(W=torch.from_numpy(W0[b]), H=torch.from_numpy(H0[b])).to(dev)
        assert one.fit(Vd[b], beta=beta, tol=-1e9, max_iter=20, weights=ones) == 20
        ew, eh = rel_err(m.W.data[b].cpu(), one.W.data.cpu()), rel_err(m.H.data[b].cpu(), one.H.data.cpu())
        record('batched_vs_weighted', beta=beta, problem=b, W=ew, H=eh)
        print(f'batched_vs_weighted beta {beta} problem {b}: W {ew:.2e} H {eh:.2e}')
        assert ew < TOL and eh < TOL, (beta, b, ew, eh)


# ---- restarts ---------------------------------------------------------------------------------------------------------------------
def test_fit_restarts(dev):
    from torchnmf_amd.batched import BatchedNMF, batched_beta_div
    from torchnmf_amd.nmf import NMF
    N, C, R = 131, 70, 5
    V, W0, H0 = _problems(1, N, C, R)
    Vd, = _dev(dev, V[0])
    kw = dict(beta=1, tol=3e-3, max_iter=40)
    runs = []
    for _ in range(2):
        m = NMF(W=torch.from_numpy(W0[0]), H=torch.from_numpy(H0[0])).to(dev)
        n, losses, best = m.fit_restarts(Vd, 6, generator=torch.Generator().manual_seed(31), **kw)
        assert n.shape == losses.shape == (6,) and n.dtype == torch.int64 and losses.dtype == torch.float64
        assert best == int(losses.argmin()) and m.last_precision == 'fp32'
        # the module holds the factors whose loss is the smallest recorded one
        now = batched_beta_div(m.H.data[None].contiguous(), m.W.data[None].contiguous(), Vd, 1)
        assert float(now[0]) == float(losses[best]) == float(losses.min())
        runs.append((m.W.data.clone(), m.H.data.clone(), n, losses, best))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert len(set(a[3].tolist())) == 6                          # six different starts
    print(f'fit_restarts: counts {a[2].tolist()} losses {a[3].tolist()} best {a[4]}')
    # n_init = 1: a BatchedNMF call on the module's own factors; the first start of the six was the same
    m = NMF(W=torch.from_numpy(W0[0]), H=torch.from_numpy(H0[0])).to(dev)
    n1, l1, best1 = m.fit_restarts(Vd, 1, **kw)
    bm = BatchedNMF(W=torch.from_numpy(W0[:1]), H=torch.from_numpy(H0[:1])).to(dev)
    nb = bm.fit(Vd, **kw)
    assert best1 == 0 and torch.equal(n1, nb) and torch.equal(l1, bm.last_loss.cpu())
    assert torch.equal(_bits(m.W.data), _bits(bm.W.data[0])) and torch.equal(_bits(m.H.data), _bits(bm.H.data[0]))
    assert int(a[2][0]) == int(n1[0]) and float(a[3][0]) == float(l1[0])
    # a frozen factor is shared by every start
    m = NMF(W=torch.from_numpy(W0[0]), H=torch.from_numpy(H0[0]), trainable_W=False).to(dev)
    m.fit_restarts(Vd, 3, generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(m.W.data.cpu(), torch.from_numpy(W0[0]))


# ---- behaviour ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_loss_is_monotone(dev, beta):
    """Five checkpoints of ten iterations, every problem: the loss does not grow; 1e-6 of the loss is the allowance for the
    rounding of the fp32 factors (as in the weighted path's test)."""
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 3, 131, 70, 33
    V, W0, H0 = _problems(B, N, C, R)
    Vd, = _dev(dev, V)
    m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    losses = [m.loss(Vd, beta).cpu()]
    for _ in range(5):
        assert m.fit(Vd, beta=beta, tol=-1e9, max_iter=10).tolist() == [10] * B
        assert torch.equal(m.last_loss, m.loss(Vd, beta))
        losses.append(m.last_loss.cpu())
    L = torch.stack(losses)
    print(f'batched monotone beta {beta}:', L.T.tolist())
    record('batched_monotone', beta=beta, first=L[0].tolist(), last=L[-1].tolist())
    assert bool((L[1:] <= L[:-1] * (1 + 1e-6)).all()), L
    assert bool((L[-1] < 0.9 * L[0]).all())


def test_target_checks_and_reproducibility(dev):
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 3, 131, 70, 33
    V, W0, H0 = _problems(B, N, C, R)
    Vd, = _dev(dev, V)

    def fresh():
        return BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    runs = []
    for _ in range(2):
        m = fresh()
        n = m.fit(Vd, beta=0.5, tol=3e-3, max_iter=30, alpha=0.07, l1_ratio=0.3)
        runs.append((m.W.data.clone(), m.H.data.clone(), n, m.last_loss.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    Vz = Vd.clone()
    Vz[1, 7, 9] = 0.0                                               # a zero in ONE problem of the batch
    for beta in (0, -1):
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            fresh().fit(Vz, beta=beta, max_iter=2)
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            fresh().loss(Vz, beta)
    assert fresh().fit(Vz, beta=1, tol=-1e9, max_iter=2).tolist() == [2] * B           # data for beta > 0
    assert fresh().fit(Vd, beta=0, tol=-1e9, max_iter=2).tolist() == [2] * B           # strictly positive: beta = 0 runs
    for bad in (-0.5, float('nan')):
        Vz[2, 0, 0] = bad
        with pytest.raises(AssertionError, match='non-negative'):
            fresh().fit(Vz, beta=1, max_iter=2)
    m = fresh()
    assert m.fit(Vd, beta=1, tol=-1e9, max_iter=0).tolist() == [0] * B                 # no iteration: the factors as they were
    assert torch.equal(m.W.data.cpu(), torch.from_numpy(W0)) and m.best(Vd, 1) == int(m.last_loss.argmin())
