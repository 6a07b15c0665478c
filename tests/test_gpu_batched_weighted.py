"""Weighted batched NMF on the device (the nmfmu_bwmu entries of csrc/nmfmu_bmu.hip, ``BatchedNMF.fit(V, weights=M)``,
``model_selection.cross_validate``): terms, step, loss and the terms of v alone of every problem per element against the
float64 model under the bounds counted in tests/weighted_emulation.py (no element left out); problem b bitwise the weighted
single-problem entries on (V_b, M_b); independence of a problem from the batch, its position, and from how its target and
weights are shared; ``M == NULL`` bitwise the unweighted entries; inactive problems; the stop rule; the reference's recorded runs
(golden g25); all-zero weights; the target checks; cross-validation on a planted target.

The shapes are the tile's edge shapes (DESIGN sections 30, 31): 131 x 70 (a row tile plus 3 rows, two stages plus 6 columns,
scalar loads; the W side sees 70 rows over 4 stages plus 3) and 132 x 72 (16-byte loads).  The problems are
weighted_emulation.make_problem's: real weights with about 30 % exact zeros, a weightless row and column, NaN / Inf / -1 /
1000 under every zero.

Measured on an MI355X (worst |got - ref| / bound over every element): see DESIGN.md section 32.
"""
import functools

import numpy as np
import pytest
import torch

import batched_weighted_emulation as BWE
import weighted_emulation as WE
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(131, 70), (132, 72)]
RANKS = [3, 33, 100, 200]             # r_pad 32 / 64 / 128 / 256 (the last: two rank tiles)
BETAS = [-1, 0, 0.5, 1, 2, 3]
SPLITS = [1, 3]
REG = (0.07 * 0.3, 0.07 * 0.7)
REGV = np.array([[0.0, 0.0], [0.07 * 0.3, 0.07 * 0.7], [0.1, 0.0]])      # a regulariser that differs per problem
TOL = 1e-4                            # the project's bar for factors after a recorded run
NAN = float('nan')
NAN_BITS = 0x7fc00abc                 # a NaN with a payload: an untouched word keeps it
DEAD_ROW, DEAD_COL = 5, 3             # weighted_emulation.make_problem


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problems(B, N, C, R):
    return BWE.make_problems(B, N, C, R)


@functools.lru_cache(maxsize=None)
def _stop_problems(B, N, C, R):
    return BWE.make_stop_problems(B, N, C, R)


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _w(M, index=None):
    """batched._Weights of a device tensor M (N, C) / (B, N, C) / (G, N, C) and an optional int32 index."""
    from torchnmf_amd import batched
    return batched._Weights(M, 0 if M.dim() == 2 else M.shape[-2] * M.shape[-1], index)


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (name, info)
    err = WE.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


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
    V, M, W0, H0 = _problems(B, N, C, R)
    info = dict(shape=f'{N}x{C}', beta=beta, R=R, nsplit=nsplit)
    Vd, Md, Wd, Hd = _dev(dev, V, M, W0, H0)
    wt = _w(Md)
    assert (Vd.data_ptr() % 16 == 0) and (Md.data_ptr() % 16 == 0) and ((C % 4 == 0) == (shape == (132, 72)))
    regd = torch.from_numpy(REGV).float().to(dev)
    for side, owner, panel, dead in (('h', Hd, Wd, DEAD_ROW), ('w', Wd, Hd, DEAD_COL)):
        rows, contraction = (N, C) if side == 'h' else (C, N)
        # terms: every element of both planes is written (they and the workspace start as NaN), padded columns exactly 0
        num, den = batched._bmu_call(Vd, N * C, side, owner, panel, float(beta), nsplit=nsplit, _fill=NAN, weights=wt)
        assert num.shape == den.shape == (B, rows, r_pad)
        assert bool((num[:, :, R:] == 0).all()) and bool((den[:, :, R:] == 0).all())
        assert bool((num[:, dead] == 0).all()) and bool((den[:, dead] == 0).all())          # a weightless row / column
        refs = BWE.terms(V, M, H0, W0, beta, side, nsplit)
        assert all(r['parts'] == nsplit for r in refs)
        for b in range(B):
            _check('bw_terms_num', num[b, :, :R], refs[b]['num'], refs[b]['num_bound'], side=side, problem=b, **info)
            _check('bw_terms_den', den[b, :, :R], refs[b]['den'], refs[b]['den_bound'], side=side, problem=b, **info)
        # step: without regularisers, with scalar ones, with a reg vector that differs per problem; the panel bitwise unchanged
        for name, scal, vec in (('none', (0.0, 0.0), None), ('scalar', REG, None), ('vector', (0.0, 0.0), REGV)):
            f = owner.clone()
            before = panel.clone()
            batched._bmu_call(Vd, N * C, side, f, panel, float(beta), step=(*scal, WE.gamma_of(beta)), nsplit=nsplit,
                              _fill=NAN, weights=wt, reg=None if vec is None else regd)
            ref = BWE.step(V, M, H0, W0, beta, side, scal if vec is None else vec, nsplit)
            for b in range(B):
                _check('bw_step', f[b], ref[b][0], ref[b][1], side=side, reg=name, problem=b, **info)
            assert torch.equal(panel, before)
            if name == 'none':
                assert _same(f[:, dead], owner[:, dead])               # nothing weighted there: bitwise unchanged
    # the terms of v alone: every term, its product with m and the sum in double, against float64 numpy
    vt_ref, vt_mag = BWE.v_term(V, M, beta, B)
    vt = batched._v_terms(Vd, N * C, B, float(beta), wt)
    assert vt.dtype == torch.float64 and vt.shape == (B,)
    assert np.all(np.abs(vt.cpu().numpy() - vt_ref) <= (N * C + 2) * 2.0 ** -53 * vt_mag), (beta, vt, vt_ref)
    nparts = lib.nmfmu_bmu_loss_parts(N, C)
    part = torch.full((B * nparts,), NAN, dtype=torch.float64, device=dev)
    out = torch.full((B,), NAN, dtype=torch.float64, device=dev)
    got = batched._bmu_loss(Hd, Wd, Vd, N * C, float(beta), torch.from_numpy(vt_ref).to(dev), part=part, out=out, weights=wt)
    assert got.dtype == torch.float64 and got.shape == (B,)
    ref = BWE.loss(V, M, H0, W0, beta)
    for b in range(B):
        _check('bw_loss', got[b].reshape(()), ref[b][0], ref[b][1], problem=b, **info)


# ---- promise 2: problem b is the weighted single-problem entry on (V_b, M_b), bit for bit -------------------------------------------
@pytest.mark.parametrize('nsplit', SPLITS)
@pytest.mark.parametrize('R', [33, 200])
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('shape', SHAPES)
def test_a_problem_is_bitwise_the_weighted_entry(dev, shape, beta, R, nsplit):
    from torchnmf_amd import batched, wmu
    from torchnmf_amd.metrics import WeightedTarget
    N, C = shape
    B = 3
    V, M, W0, H0 = _problems(B, N, C, R)
    Vd, Md, Wd, Hd = _dev(dev, V, M, W0, H0)
    wt = _w(Md)
    regd = torch.from_numpy(REGV).float().to(dev)
    gamma = WE.gamma_of(beta)
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        num, den = batched._bmu_call(Vd, N * C, side, owner, panel, float(beta), nsplit=nsplit, weights=wt)
        f = owner.clone()
        batched._bmu_call(Vd, N * C, side, f, panel, float(beta), step=(0.0, 0.0, gamma), nsplit=nsplit, weights=wt, reg=regd)
        for b in range(B):
            T = WeightedTarget(Vd[b], Md[b])
            n1, d1 = wmu._wmu_call(T, side, owner[b].contiguous(), panel[b].contiguous(), float(beta), nsplit=nsplit)
            assert _same(n1, num[b]) and _same(d1, den[b]), (side, b)
            f1 = owner[b].clone()
            l1, l2 = (float(x) for x in regd[b].cpu())
            wmu._wmu_call(T, side, f1, panel[b].contiguous(), float(beta), step=(l1, l2, gamma), nsplit=nsplit)
            assert _same(f1, f[b]), (side, b)


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_fit_is_bitwise_the_weighted_fit(dev, beta):
    from torchnmf_amd.batched import BatchedNMF
    from torchnmf_amd.nmf import NMF
    B, N, C, R = 3, 131, 70, 33
    V, M, W0, H0 = _problems(B, N, C, R)
    Vd, Md = _dev(dev, V, M)
    alphas = [0.0, 0.07, 0.2]
    m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    assert m.fit(Vd, beta=beta, tol=-1e9, max_iter=20, alpha=alphas, l1_ratio=0.3, weights=Md).tolist() == [20] * B
    assert m.last_precision == 'fp32'
    for b in range(B):
        one = NMF(W=torch.from_numpy(W0[b]), H=torch.from_numpy(H0[b])).to(dev)
        assert one.fit(Vd[b], beta=beta, tol=-1e9, max_iter=20, alpha=alphas[b], l1_ratio=0.3, weights=Md[b]) == 20
        assert _same(m.W.data[b], one.W.data) and _same(m.H.data[b], one.H.data), b


# ---- promise 3: a problem does not see the batch, its position, or how its target and weights reach it -----------------------------
P3_TOL = {0.5: 0.016, 1: 0.03, 2: 0.015}        # between the model's checkpoint ratios at iteration 20 (asserted below)
P3_ALPHA = [0.0, 0.05, 0.0, 0.1, 0.02]


@functools.lru_cache(maxsize=None)
def _p3_model(beta):
    V, M, W0, H0 = _stop_problems(5, 131, 70, 3)
    _, _, n, trace = BWE.fit(V, M, W0, H0, beta, P3_TOL[beta], 30, BWE.l1_l2(P3_ALPHA, 0.3))
    return n.tolist(), float(BWE.judged_margins(trace, P3_TOL[beta]).min())


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_a_problem_is_independent_of_batch_position_and_sharing(dev, beta):
    """B = 5 against five B = 1 calls, a permuted batch, (G, N, C) weights through weight_index [1, 0, 1, 1, 0] against their
    expanded (B, N, C) copy, a shared target against its expanded copy: terms, one step, a 30-iteration fit with stopping,
    counts and losses, all bitwise.  The problems do not all stop together: the float64 model's counts are asserted, and
    every checkpoint it judges is at least 0.05 tol from the threshold."""
    from torchnmf_amd import batched
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 5, 131, 70, 3
    V, M, W0, H0 = _stop_problems(B, N, C, R)
    Vd, Md, Wd, Hd = _dev(dev, V, M, W0, H0)
    tol = P3_TOL[beta]
    counts, margin = _p3_model(beta)
    assert margin >= 0.05 * tol and len(set(counts)) > 1, (counts, margin)
    regd = torch.from_numpy(BWE.l1_l2(P3_ALPHA, 0.3)).float().to(dev)
    gamma = WE.gamma_of(beta)

    def run(Vx, Mx, Wx, Hx, alpha, index=None):
        """(num, den, stepped W, fitted W, H, counts, last_loss, loss) of one way to pose the problems"""
        Bx = Hx.shape[0]
        vstride = 0 if Vx.dim() == 2 else N * C
        wt = _w(Mx, index)
        num, den = batched._bmu_call(Vx, vstride, 'h', Hx, Wx, float(beta), weights=wt)
        stepped = Wx.clone()
        reg = torch.from_numpy(BWE.l1_l2(alpha, 0.3)).float().to(dev)
        batched._bmu_call(Vx, vstride, 'w', stepped, Hx, float(beta), step=(0.0, 0.0, gamma), weights=wt, reg=reg)
        m = BatchedNMF(W=Wx.cpu(), H=Hx.cpu()).to(dev)
        n = m.fit(Vx, beta=beta, tol=tol, max_iter=30, alpha=alpha, l1_ratio=0.3, weights=Mx, weight_index=index)
        assert n.shape == (Bx,) and n.dtype == torch.int64
        return num, den, stepped, m.W.data.clone(), m.H.data.clone(), n.to(dev), m.last_loss.clone(), \
            m.loss(Vx, beta, weights=Mx, weight_index=index)

    def equal(a, b, sel=slice(None)):
        return all(_same(x, y[sel]) for x, y in zip(a, b))
    full = run(Vd, Md, Wd, Hd, P3_ALPHA)
    print(f'independence beta {beta}: counts {full[5].tolist()} (model {counts}, margin {margin / tol:.3f} tol)')
    assert full[5].tolist() == counts and torch.equal(full[6], full[7])
    for b in range(B):                                                   # five B = 1 calls
        one = slice(b, b + 1)
        assert equal(run(Vd[one].contiguous(), Md[one].contiguous(), Wd[one].contiguous(), Hd[one].contiguous(),
                         P3_ALPHA[b:b + 1]), full, one), b
    perm = [3, 0, 4, 2, 1]                                               # a permuted batch
    pd = torch.tensor(perm, device=dev)
    assert equal(run(Vd[pd].contiguous(), Md[pd].contiguous(), Wd[pd].contiguous(), Hd[pd].contiguous(),
                     [P3_ALPHA[p] for p in perm]), full, pd)
    index = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device=dev)   # G = 2 weight matrices through the index
    Mg = Md[:2].contiguous()
    Vi = Vd[index.long()].contiguous()            # (every problem's target is valid under the weights it reads)
    assert equal(run(Vi, Mg, Wd, Hd, P3_ALPHA, index), run(Vi, Mg[index.long()].contiguous(), Wd, Hd, P3_ALPHA))
    # ... and with a shared target as well, what cross-validation uses: problem 0's target under its weights, problem 1's
    # elsewhere -- valid under either weight matrix
    Vs = torch.where(Md[0] > 0, Vd[0], Vd[1]).contiguous()
    assert bool((Vs[(Mg > 0).any(0)] > 0).all())
    shared = run(Vs, Mg, Wd, Hd, P3_ALPHA, index)
    assert equal(shared, run(Vs.expand(B, N, C).contiguous(), Mg[index.long()].contiguous(), Wd, Hd, P3_ALPHA))
    assert equal(shared, run(Vs, Mg[index.long()].contiguous(), Wd, Hd, P3_ALPHA))
    assert equal(shared, run(Vs.expand(B, N, C).contiguous(), Mg, Wd, Hd, P3_ALPHA, index))
    # one weight matrix shared by every problem (m_batch_stride 0) against its expanded copy, the target shared or not
    V2, M2 = Vd[2].contiguous(), Md[2].contiguous()
    both = run(V2, M2, Wd, Hd, P3_ALPHA)
    assert equal(both, run(V2, M2.expand(B, N, C).contiguous(), Wd, Hd, P3_ALPHA))
    assert equal(both, run(V2.expand(B, N, C).contiguous(), M2, Wd, Hd, P3_ALPHA))


# ---- promise 1: M == NULL is the unweighted batch, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize('nsplit', SPLITS)
@pytest.mark.parametrize('beta', [0, 0.5, 1, 2])
@pytest.mark.parametrize('shape', SHAPES)
def test_null_weights_are_the_unweighted_entries(dev, shape, beta, nsplit):
    from torchnmf_amd import batched
    import batched_emulation as BE
    N, C = shape
    B, R = 3, 33
    V, W0, H0 = BE.make_problems(B, N, C, R)
    Vd, Wd, Hd = _dev(dev, V, W0, H0)
    null = batched._Weights(None, 0, None)
    gamma = WE.gamma_of(beta)
    regd = torch.from_numpy(REGV).float().to(dev)
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        old = batched._bmu_call(Vd, N * C, side, owner, panel, float(beta), nsplit=nsplit)
        new = batched._bmu_call(Vd, N * C, side, owner, panel, float(beta), nsplit=nsplit, weights=null, _fill=NAN)
        assert _same(old[0], new[0]) and _same(old[1], new[1])
        a, b = owner.clone(), owner.clone()
        batched._bmu_call(Vd, N * C, side, a, panel, float(beta), step=(*REG, gamma), nsplit=nsplit)
        batched._bmu_call(Vd, N * C, side, b, panel, float(beta), step=(*REG, gamma), nsplit=nsplit, weights=null, _fill=NAN)
        assert _same(a, b)
        # reg without weights: the old step called per problem with that problem's scalars
        f = owner.clone()
        batched._bmu_call(Vd, N * C, side, f, panel, float(beta), step=(0.0, 0.0, gamma), nsplit=nsplit, reg=regd, _fill=NAN)
        for p in range(B):
            one = owner[p:p + 1].clone()
            l1, l2 = (float(x) for x in regd[p].cpu())
            batched._bmu_call(Vd[p:p + 1].contiguous(), N * C, side, one, panel[p:p + 1].contiguous(), float(beta),
                              step=(l1, l2, gamma), nsplit=nsplit)
            assert _same(one[0], f[p]), (side, p)
    vt = batched._v_terms(Vd, N * C, B, float(beta))
    assert torch.equal(vt, batched._v_terms(Vd, N * C, B, float(beta), null))
    assert torch.equal(batched._bmu_loss(Hd, Wd, Vd, N * C, float(beta), vt),
                       batched._bmu_loss(Hd, Wd, Vd, N * C, float(beta), vt, weights=null))


def test_unit_weights_and_scalar_alpha_are_the_unweighted_fit(dev):
    """weights=None with scalar alpha calls what it always called; unit weights reach the same bits through the weighted tile
    (DESIGN section 31), and a constant alpha vector is the scalar."""
    from torchnmf_amd.batched import BatchedNMF
    import batched_emulation as BE
    B, N, C, R = 3, 131, 70, 33
    V, W0, H0 = BE.make_problems(B, N, C, R)
    Vd, = _dev(dev, V)
    runs = []
    for kw in (dict(alpha=0.07), dict(alpha=[0.07] * B), dict(alpha=0.07, weights=torch.ones(N, C, device=dev)),
               dict(alpha=torch.full((B,), 0.07, dtype=torch.float64), weights=torch.ones(B, N, C, dtype=torch.bool, device=dev))):
        m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
        n = m.fit(Vd, beta=1, tol=3e-3, max_iter=30, l1_ratio=0.3, **kw)
        runs.append((m.W.data.clone(), m.H.data.clone(), n.to(dev), m.last_loss.clone()))
    for other in runs[1:3]:
        assert all(_same(x, y) for x, y in zip(runs[0][:3], other[:3]))
    assert all(_same(x, y) for x, y in zip(runs[2], runs[3]))


# ---- promise 4: inactive problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nsplit', [1, 2])
def test_inactive_problems_are_not_touched(dev, nsplit):
    from torchnmf_amd import _capi, batched
    lib = _capi.load()
    B, N, C, R = 3, 131, 70, 33
    beta = 0.5
    r_pad = lib.nmfmu_pad_rank(R)
    V, M, W0, H0 = _problems(B, N, C, R)
    Vd, Md, Wd, Hd = _dev(dev, V, M, W0, H0)
    wt = _w(Md)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    regd = torch.from_numpy(REGV).float().to(dev)
    step = (0.0, 0.0, WE.gamma_of(beta))
    for side, owner, panel in (('h', Hd, Wd), ('w', Wd, Hd)):
        rows, contraction = (N, C) if side == 'h' else (C, N)
        n_ws = lib.nmfmu_bmu_ws(B, rows, contraction, r_pad, nsplit)
        per = n_ws // B
        full = owner.clone()
        batched._bmu_call(Vd, N * C, side, full, panel, beta, step=step, nsplit=nsplit, weights=wt, reg=regd)
        ws = torch.full((n_ws,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        f = owner.clone()
        batched._bmu_call(Vd, N * C, side, f, panel, beta, step=step, nsplit=nsplit, active=active, _ws=ws, weights=wt, reg=regd)
        assert _same(f[1], owner[1])                                                   # its factors
        assert bool((_bits(ws[per:2 * per]) == NAN_BITS).all())                        # its slab slice
        assert not bool((_bits(ws[:per]) == NAN_BITS).any()) and not bool((_bits(ws[2 * per:]) == NAN_BITS).any())
        for b in (0, 2):
            assert _same(f[b], full[b])
        # terms: the planes of the inactive problem keep what they held
        num, den = batched._bmu_call(Vd, N * C, side, owner, panel, beta, nsplit=nsplit, active=active, _fill=NAN, weights=wt)
        num_all, den_all = batched._bmu_call(Vd, N * C, side, owner, panel, beta, nsplit=nsplit, weights=wt)
        assert bool(torch.isnan(num[1]).all()) and bool(torch.isnan(den[1]).all())
        for b in (0, 2):
            assert _same(num[b], num_all[b]) and _same(den[b], den_all[b])
    vt = batched._v_terms(Vd, N * C, B, beta, wt)
    nparts = lib.nmfmu_bmu_loss_parts(N, C)
    all_ = batched._bmu_loss(Hd, Wd, Vd, N * C, beta, vt, weights=wt)
    out = torch.tensor([7.0, -3.25, 7.0], dtype=torch.float64, device=dev)
    part = torch.full((B * nparts,), NAN_BITS | (NAN_BITS << 32), dtype=torch.int64, device=dev).view(torch.float64)
    batched._bmu_loss(Hd, Wd, Vd, N * C, beta, vt, active=active, part=part, out=out, weights=wt)
    assert float(out[1]) == -3.25 and torch.equal(out[0], all_[0]) and torch.equal(out[2], all_[2])
    words = part.view(torch.int64)
    assert bool((words[nparts:2 * nparts] == (NAN_BITS | (NAN_BITS << 32))).all())     # its partials
    assert not bool((words[:nparts] == (NAN_BITS | (NAN_BITS << 32))).any())
    assert not bool((words[2 * nparts:] == (NAN_BITS | (NAN_BITS << 32))).any())


# ---- the stop rule ------------------------------------------------------------------------------------------------------------------
STOP_ALPHA = [0.0, 0.05, 0.0, 0.1]


@functools.lru_cache(maxsize=None)
def _stop_model(R, beta):
    V, M, W0, H0 = _stop_problems(4, 131, 70, R)
    return BWE.fit(V, M, W0, H0, beta, 1e-3, 100, BWE.l1_l2(STOP_ALPHA, 0.3))


@pytest.mark.parametrize('R,beta', [(3, 0.5), (3, 1), (5, 2)])
def test_stop_rule_follows_the_model(dev, R, beta):
    """tol = 1e-3 on planted targets: the counts are the float64 model's, the factors within the project's 1e-4.  The model's
    judged checkpoints are all at least 0.05 tol from the threshold (g24's screen; asserted here), five hundred times what
    fp32 rounding moves the ratio."""
    from torchnmf_amd.batched import BatchedNMF
    tol = 1e-3
    V, M, W0, H0 = _stop_problems(4, 131, 70, R)
    Wm, Hm, nm, trace = _stop_model(R, beta)
    margin = float(BWE.judged_margins(trace, tol).min())
    assert margin >= 0.05 * tol and len(set(nm.tolist())) > 1 and min(nm.tolist()) < 100, (nm, margin)
    Vd, Md = _dev(dev, V, M)
    m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    n = m.fit(Vd, beta=beta, tol=tol, max_iter=100, alpha=STOP_ALPHA, l1_ratio=0.3, weights=Md)
    print(f'bw_stop R {R} beta {beta}: counts {n.tolist()} (model {nm.tolist()}, margin {margin / tol:.3f} tol)')
    assert n.tolist() == nm.tolist()
    for b in range(4):
        ew, eh = rel_err(m.W.data[b].cpu(), Wm[b]), rel_err(m.H.data[b].cpu(), Hm[b])
        ref_loss, bound = WE.loss(V[b], M[b], m.H.data[b].cpu().numpy(), m.W.data[b].cpu().numpy(), beta)
        record('bw_stop', R=R, beta=beta, problem=b, W=ew, H=eh)
        print(f'bw_stop R {R} beta {beta} problem {b}: W {ew:.2e} H {eh:.2e}')
        assert ew < TOL and eh < TOL, (b, ew, eh)
        _check('bw_stop_last_loss', m.last_loss[b].reshape(()), ref_loss, bound, R=R, beta=beta, problem=b)


# ---- the reference's recorded runs ----------------------------------------------------------------------------------------------
G25 = load_golden('g25_batched_weighted')


@pytest.mark.parametrize('case', [str(c) for c in G25['cases']])
def test_golden_g25(dev, case):
    from torchnmf_amd.batched import BatchedNMF
    g = G25
    beta, k = float(g[case + '_beta']), int(g['iterations'])
    V, M = torch.from_numpy(g['V']).to(dev), torch.from_numpy(g['M']).to(dev)          # integer weights as they are
    index = torch.from_numpy(g['weight_index']).to(dev)
    m = BatchedNMF(W=torch.from_numpy(g['W0']), H=torch.from_numpy(g['H0'])).to(dev)
    n = m.fit(V, beta=beta, tol=-1e9, max_iter=k, alpha=g['alpha'].tolist(), l1_ratio=torch.from_numpy(g['l1_ratio']),
              weights=M, weight_index=index)
    assert n.tolist() == [k] * 4 and m.last_precision == 'fp32'
    loss = m.loss(V, beta, weights=M, weight_index=index)
    assert torch.equal(loss, m.last_loss)
    worst = 0.0
    for b in range(4):
        ew, eh = rel_err(m.W.data[b].cpu(), g[case + '_W'][b]), rel_err(m.H.data[b].cpu(), g[case + '_H'][b])
        el = abs(float(loss[b]) - float(g[case + '_loss'][b])) / abs(float(g[case + '_loss'][b]))
        record('bw_g25', case=case, problem=b, W=ew, H=eh, loss=el)
        print(f'bw_g25 {case} problem {b}: W {ew:.2e} H {eh:.2e} loss {el:.2e}')
        worst = max(worst, ew, eh)
        assert ew < TOL and eh < TOL, (case, b, ew, eh)
    record('bw_g25_worst', case=case, worst=worst)


# ---- behaviour ------------------------------------------------------------------------------------------------------------------
def test_all_zero_weights(dev):
    """A problem whose weights are all 0: loss 0, the stop ratio NaN, so it runs to max_iter; with alpha = 0 its factors are
    kept bit for bit (num = den = 0: the multiplier is eps / eps); its neighbours are what they are without it."""
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 3, 131, 70, 33
    V, M, W0, H0 = _problems(B, N, C, R)
    M = M.copy()
    M[1] = 0.0
    Vd, Md = _dev(dev, V, M)
    for beta in (0.5, 1, 2):
        m = BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
        n = m.fit(Vd, beta=beta, tol=10.0, max_iter=20, alpha=[0.1, 0.0, 0.0], l1_ratio=0.3, weights=Md)
        assert n.tolist() == [10, 20, 10]                  # tol 10 stops the others at the first checkpoint (a ratio is <= 1)
        assert float(m.last_loss[1]) == 0.0 and bool((m.last_loss[[0, 2]] > 0).all())
        assert _same(m.W.data[1].cpu(), torch.from_numpy(W0[1])) and _same(m.H.data[1].cpu(), torch.from_numpy(H0[1]))
        assert not _same(m.W.data[0].cpu(), torch.from_numpy(W0[0]))
        solo = BatchedNMF(W=torch.from_numpy(W0[[0, 2]]), H=torch.from_numpy(H0[[0, 2]])).to(dev)
        solo.fit(Vd[[0, 2]].contiguous(), beta=beta, tol=10.0, max_iter=20, alpha=[0.1, 0.0], l1_ratio=0.3,
                 weights=Md[[0, 2]].contiguous())
        assert _same(solo.W.data, m.W.data[[0, 2]]) and _same(solo.H.data, m.H.data[[0, 2]])


def test_target_checks(dev):
    """The two flags of nmf.py:329-336 over the entries that carry a positive weight in a problem that uses them."""
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R = 3, 131, 70, 3
    V, M, W0, H0 = _problems(B, N, C, R)
    Vd, Md = _dev(dev, V, M)
    assert np.isnan(V).any() and np.isinf(V).any() and (V == -1).any()

    def fresh():
        return BatchedNMF(W=torch.from_numpy(W0), H=torch.from_numpy(H0)).to(dev)
    for beta in (0, 1):                                              # NaN, Inf and -1 under weight 0 are accepted
        assert fresh().fit(Vd, beta=beta, tol=-1e9, max_iter=2, weights=Md).tolist() == [2] * B
        assert bool(torch.isfinite(fresh().loss(Vd, beta, weights=Md)).all())
    with pytest.raises(AssertionError, match='non-negative'):          # ... and refused without the weights
        fresh().fit(Vd, beta=1, max_iter=2)
    i, j = np.argwhere(M[1] > 0)[7]
    Vz = Vd.clone()
    Vz[1, i, j] = 0.0                                                # a zero under a positive weight, in ONE problem
    for beta in (0, -1):
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            fresh().fit(Vz, beta=beta, max_iter=2, weights=Md)
        with pytest.raises(ValueError, match='When beta <= 0 and V contains zeros'):
            fresh().loss(Vz, beta, weights=Md)
    assert fresh().fit(Vz, beta=1, tol=-1e9, max_iter=2, weights=Md).tolist() == [2] * B
    for bad in (-0.5, float('nan')):
        Vz[1, i, j] = bad                                            # a negative value or NaN under a positive weight
        with pytest.raises(AssertionError, match='non-negative'):
            fresh().fit(Vz, beta=1, max_iter=2, weights=Md)
        with pytest.raises(AssertionError, match='non-negative'):
            fresh().best(Vz, 1, weights=Md)
    # through an index only the slices in use are looked at: slice 1 marks (i, j) of the shared target, slice 0 does not
    Mg = Md[:2].clone()
    Mg[0, i, j] = 0.0
    Vs = torch.where(Mg[1] > 0, Vd[1], Vd[0]).contiguous()
    Vs[i, j] = -0.5
    unused = torch.zeros(B, dtype=torch.int64, device=dev)
    assert fresh().fit(Vs, beta=1, tol=-1e9, max_iter=2, weights=Mg, weight_index=unused).tolist() == [2] * B
    with pytest.raises(AssertionError, match='non-negative'):
        fresh().fit(Vs, beta=1, max_iter=2, weights=Mg, weight_index=torch.tensor([0, 1, 0], device=dev))
    with pytest.raises(ValueError, match='weight_index lives on'):
        fresh().fit(Vs, beta=1, max_iter=2, weights=Mg, weight_index=unused.cpu())
    with pytest.raises(ValueError, match='weights live on'):
        fresh().fit(Vd, beta=1, max_iter=2, weights=Md.cpu())


# ---- cross-validation -------------------------------------------------------------------------------------------------------------
CV_SEED, CV_RANKS, CV_FOLDS, CV_STARTS, CV_ITER = 0, (2, 4, 8), 4, 2, 200


@functools.lru_cache(maxsize=None)
def _cv_inputs():
    """The planted target, and the masks and starts cross_validate draws from the seed (masks first, then W and H per rank)."""
    from torchnmf_amd import model_selection as MS
    V = BWE.planted(131, 70, 4, seed=CV_SEED)
    g = torch.Generator().manual_seed(CV_SEED)
    train, test = MS.holdout_masks(V.shape, CV_FOLDS, g)
    starts = [MS.draw_starts(CV_FOLDS * CV_STARTS, 131, 70, R, g) for R in CV_RANKS]
    return V, train, test, starts


@functools.lru_cache(maxsize=None)
def _cv_model(beta):
    V, train, test, starts = _cv_inputs()
    return BWE.cross_validate(V, train.numpy(), test.numpy(), [(w.numpy(), h.numpy()) for w, h in starts], CV_RANKS, (0.0,),
                              beta, 0.0, CV_ITER)


@pytest.mark.parametrize('beta', [1, 2])
def test_cross_validate_finds_the_planted_rank(dev, beta):
    """131 x 70, true rank 4, |H W^T (1 + 0.1 randn)| + 1e-3; ranks (2, 4, 8), 4 folds, 2 starts, 200 iterations without
    stopping.  (a) every train / test loss is the float64 loss of the factors the fit returns, under weighted_emulation.loss's
    bound; (b) mean_test and best follow from the returned arrays; (c) the best rank is 4 -- resting on the float64 model alone
    putting its runner-up at least 5 % above its best (asserted on the model)."""
    from torchnmf_amd.batched import BatchedNMF
    from torchnmf_amd.model_selection import cross_validate, problem_layout
    V, train, test, starts = _cv_inputs()
    Vd, = _dev(dev, V)
    res = cross_validate(Vd, CV_RANKS, beta=beta, folds=CV_FOLDS, n_init=CV_STARTS, tol=-1e9, max_iter=CV_ITER,
                         generator=torch.Generator().manual_seed(CV_SEED))
    shape = (len(CV_RANKS), 1, CV_FOLDS, CV_STARTS)
    assert res.ranks == CV_RANKS and res.alphas == (0.0,)
    assert res.n_iter.dtype == torch.int64 and bool((res.n_iter == CV_ITER).all())
    for t in (res.n_iter, res.train_loss, res.test_loss):
        assert tuple(t.shape) == shape and t.device.type == 'cpu'
    assert res.train_loss.dtype == res.test_loss.dtype == torch.float64
    assert torch.equal(res.masks[0].cpu(), train) and torch.equal(res.masks[1].cpu(), test)
    assert torch.equal(res.n_test, test.double().sum(dim=(1, 2))) and tuple(res.mean_test.shape) == (3, 1)
    # (a) the same fits posed directly: the losses are cross_validate's bit for bit, and the float64 loss of those factors
    _, k_of, _ = problem_layout(1, CV_FOLDS, CV_STARTS)
    index = k_of.to(dev)
    for i, R in enumerate(CV_RANKS):
        m = BatchedNMF(W=starts[i][0], H=starts[i][1]).to(dev)
        m.fit(Vd, beta=beta, tol=-1e9, max_iter=CV_ITER, weights=train.to(dev), weight_index=index)
        assert torch.equal(m.last_loss.cpu().reshape(shape[1:]), res.train_loss[i])
        assert torch.equal(m.loss(Vd, beta, weights=test.to(dev), weight_index=index).cpu().reshape(shape[1:]), res.test_loss[i])
        Hn, Wn = m.H.data.cpu().numpy(), m.W.data.cpu().numpy()
        for b in range(len(k_of)):
            k = int(k_of[b])
            for name, mask, got in (('train', train, res.train_loss), ('test', test, res.test_loss)):
                ref, bound = WE.loss(V, mask[k].numpy(), Hn[b], Wn[b], beta)
                _check('cv_loss', got[i].reshape(-1)[b].reshape(()), ref, bound, which=name, beta=beta, R=R, problem=b)
    # (b) consistency of the summary with the arrays
    mean = (res.test_loss / res.n_test.reshape(1, 1, -1, 1)).mean(dim=(2, 3))
    assert torch.equal(mean, res.mean_test)
    at = int(res.mean_test.reshape(-1).argmin())
    assert res.best == (CV_RANKS[at], 0.0)
    # (c) the planted rank, on the float64 model's margin
    model = _cv_model(beta)
    ordered = np.sort(model['mean_test'][:, 0])
    assert model['best'][0] == 4 and ordered[1] >= 1.05 * ordered[0], model['mean_test']
    diff = float((res.mean_test[:, 0] - torch.from_numpy(model['mean_test'][:, 0])).abs().div(
        torch.from_numpy(model['mean_test'][:, 0])).max())
    record('cv_mean_test', beta=beta, device=res.mean_test[:, 0].tolist(), model=model['mean_test'][:, 0].tolist(),
           worst_relative_difference=diff)
    print(f'cv beta {beta}: mean_test {res.mean_test[:, 0].tolist()} model {model["mean_test"][:, 0].tolist()} '
          f'(runner-up / best {ordered[1] / ordered[0]:.3f}); device vs model {diff:.2e}; best {res.best}')
    assert res.best[0] == 4


def test_cross_validate_sweeps_alpha_and_respects_base_weights(dev):
    """Two alphas in one launch sequence per rank, on the masks a single alpha gets from the same seed; base weights with zeros
    hide junk from the masks, the fits and the scores."""
    from torchnmf_amd.model_selection import cross_validate
    V = BWE.planted(131, 70, 4, seed=CV_SEED)
    Vd, = _dev(dev, V)
    kw = dict(beta=1, folds=3, n_init=2, tol=-1e9, max_iter=20)
    one = cross_validate(Vd, (3,), alpha=0.0, generator=torch.Generator().manual_seed(5), **kw)
    assert tuple(one.test_loss.shape) == (1, 1, 3, 2)
    two = cross_validate(Vd, (3,), alpha=(0.0, 0.3), l1_ratio=0.5, generator=torch.Generator().manual_seed(5), **kw)
    assert two.alphas == (0.0, 0.3) and tuple(two.test_loss.shape) == (1, 2, 3, 2)
    assert torch.equal(two.masks[1], one.masks[1])
    assert bool((two.train_loss[0, 1] > 0).all()) and bool(torch.isfinite(two.mean_test).all())
    assert two.best[0] == 3 and two.best[1] in two.alphas
    base = torch.from_numpy(WE.make_problem(131, 70, 3)[1]).to(dev)
    junk = torch.where(base > 0, Vd, torch.full_like(Vd, float('nan')))
    res = cross_validate(junk, (3,), weights=base, generator=torch.Generator().manual_seed(5), **kw)
    assert bool(torch.isfinite(res.test_loss).all()) and bool(torch.isfinite(res.train_loss).all())
    assert torch.equal(res.masks[0] + res.masks[1], base.expand(3, 131, 70))
    assert abs(float(res.n_test.sum()) - float(base.double().sum())) <= 1e-9 * float(base.double().sum())
