"""``trainer.BetaMu``'s kernels and host composition per element against float64 (tests/trainer_emulation.py).

Every kernel is checked from the inputs the device gave it, so no bound absorbs an upstream product's rounding:

* ``nmfmu_trainer_update``, ``nmfmu_mu_terms``, ``nmfmu_reconstruct`` through the C entries: outputs prefilled with NaN, guard
  elements behind every buffer, every element checked, every launch run twice with bit-identical results;
* the fused one-layer path (``DenseMU.trainer_step`` -> ``nmfmu_trainer_apply``): the slabs the partial launch left are summed
  over the splits in fp32 in the kernel's order and handed to ``update`` / ``update_bound`` together with the old master and
  the other factor's column sums; master per element, ``grad`` bit-exact, operand images bit-exact roundings of the new
  master, column sums, status word -- for one parameter, then for the other from the state the first step left;
* a chain of three layers and one convolutive layer end to end, one optimiser per parameter from the same start state.

The worst error / bound ratio of every test goes to ``conftest.record('trainer_parity', ...)``.
"""
import numpy as np
import pytest
import torch

from conftest import record
import trainer_emulation as T
from test_gpu_emulated_parity import _check_images

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD, SENTINEL = 64, -12345.75
PEN = T.PENALTIES


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dev, data=None):
    """n floats (``data`` or NaN) followed by GUARD sentinels."""
    buf = torch.full((n + GUARD,), NAN, device=dev)
    buf[n:] = SENTINEL
    if data is not None:
        buf[:n] = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).reshape(-1).to(dev)
    return buf


def _guards_ok(n, *bufs):
    return all(bool((b[n_:] == SENTINEL).all()) for b, n_ in zip(bufs, n))


def _host(buf, n, shape):
    return buf[:n].cpu().numpy().reshape(shape)


# ---- nmfmu_trainer_update ------------------------------------------------------------------------------------------------
def _trainer_update(dev, theta, neg, pos, gamma, pen, with_grad):
    from torchnmf_amd import _capi
    lib = _capi.load()
    rows, cols = theta.shape
    n = rows * cols
    f, ng, ps = _guarded(n, dev, theta), _guarded(n, dev, neg), _guarded(n, dev, pos)
    gr = _guarded(n, dev)
    _capi.check(lib.nmfmu_trainer_update(f.data_ptr(), rows, cols, ng.data_ptr(), ps.data_ptr(), *pen, gamma,
                                         gr.data_ptr() if with_grad else None, _stream()), 'nmfmu_trainer_update')
    torch.cuda.synchronize()
    assert _guards_ok([n] * 4, f, ng, ps, gr)
    assert np.array_equal(_host(ng, n, theta.shape), neg) and np.array_equal(_host(ps, n, theta.shape), pos)   # inputs untouched
    return _host(f, n, theta.shape), _host(gr, n, theta.shape)


@pytest.mark.parametrize('shape', T.UPDATE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_trainer_update_per_element(dev, shape):
    theta, neg, pos = T.update_problem(*shape)
    assert bool((neg < 0).any() or shape == (1, 1)) and (shape == (1, 1) or bool(((neg == 0) & (pos == 0)).any()))
    want_grad = T.grad_f32(neg, pos)
    worst = 0.0
    for beta in T.UPDATE_BETAS:
        gamma = T.mu_gamma(beta)
        for name, pen in PEN.items():
            ref, _ = T.update(theta, neg, pos, gamma, *pen)
            bound = T.update_bound(theta, neg, pos, gamma, *pen, c_rs=T.rowsum_ops_update(shape[1]))
            new, grad = _trainer_update(dev, theta, neg, pos, gamma, pen, True)
            ratio = T.worst_ratio(new, ref, bound)
            print(f'trainer_update {shape} beta {beta:g} {name}: worst error / bound = {ratio:.3f}')
            worst = max(worst, ratio)
            assert ratio <= 1.0, (beta, name, ratio)
            assert np.array_equal(grad.view(np.uint32), want_grad.view(np.uint32)), (beta, name)
            new2, grad2 = _trainer_update(dev, theta, neg, pos, gamma, pen, True)
            assert np.array_equal(new.view(np.uint32), new2.view(np.uint32)) and np.array_equal(grad.view(np.uint32), grad2.view(np.uint32))
            new3, grad3 = _trainer_update(dev, theta, neg, pos, gamma, pen, False)         # grad == NULL
            assert np.array_equal(new.view(np.uint32), new3.view(np.uint32)) and bool(np.isnan(grad3).all())
    record('trainer_parity', kernel='trainer_update', shape=list(shape), worst_ratio=worst)


# ---- nmfmu_mu_terms ------------------------------------------------------------------------------------------------------
def _mu_terms(dev, s_d, v_d, n, beta):
    from torchnmf_amd import _capi
    gn, gp = _guarded(n, dev), _guarded(n, dev)
    _capi.check(_capi.load().nmfmu_mu_terms(s_d.data_ptr(), v_d.data_ptr(), n, float(beta), gn.data_ptr(), gp.data_ptr(),
                                            _stream()), 'nmfmu_mu_terms')
    torch.cuda.synchronize()
    assert _guards_ok([n] * 4, s_d, v_d, gn, gp)
    return _host(gn, n, (n,)), _host(gp, n, (n,))


@pytest.mark.parametrize('n', T.TERMS_SIZES)
def test_mu_terms_per_element(dev, n):
    s, v = T.terms_problem(n)
    s_d, v_d = _guarded(n, dev, s), _guarded(n, dev, v)
    worst = 0.0
    for beta in T.TERMS_BETAS:
        gn, gp = _mu_terms(dev, s_d, v_d, n, beta)
        rn, rp = T.terms(s, v, beta)
        bn, bp = T.terms_bound(s, v, beta)
        ratio = max(T.worst_ratio(gn, rn, bn), T.worst_ratio(gp, rp, bp))
        print(f'mu_terms n {n} beta {beta:g}: worst error / bound = {ratio:.3f}')
        worst = max(worst, ratio)
        assert ratio <= 1.0, (beta, ratio)
        if beta == 2:
            assert np.array_equal(gn.view(np.uint32), v.view(np.uint32)) and np.array_equal(gp.view(np.uint32), s.view(np.uint32))
        if beta == 1:
            assert bool((gp == np.float32(1.0)).all())
        gn2, gp2 = _mu_terms(dev, s_d, v_d, n, beta)
        assert np.array_equal(gn.view(np.uint32), gn2.view(np.uint32)) and np.array_equal(gp.view(np.uint32), gp2.view(np.uint32))
    record('trainer_parity', kernel='mu_terms', n=n, worst_ratio=worst)


# ---- nmfmu_reconstruct ---------------------------------------------------------------------------------------------------
def _reconstruct(dev, A, B, ld):
    from torchnmf_amd import _capi
    (M, R), K = A.shape, B.shape[0]
    a, b = _guarded(M * R, dev, A), _guarded(K * R, dev, B)
    out = _guarded(M * ld, dev)
    _capi.check(_capi.load().nmfmu_reconstruct(a.data_ptr(), M, b.data_ptr(), K, R, out.data_ptr(), ld, _stream()),
                'nmfmu_reconstruct')
    torch.cuda.synchronize()
    assert _guards_ok([M * R, K * R, M * ld], a, b, out)
    full = _host(out, M * ld, (M, ld))
    assert bool(np.isnan(full[:, K:]).all())                  # the columns between K and ld
    return full[:, :K]


@pytest.mark.parametrize('mk', T.RECON_MK, ids=lambda s: f'{s[0]}x{s[1]}')
def test_reconstruct_per_element(dev, mk):
    M, K = mk
    worst = 0.0
    for R in T.RECON_R:
        A, B = T.recon_problem(M, K, R)
        ref, bound = T.matmul(A, B), T.matmul_bound(A, B)
        Ah, Bh = T.recon_problem(M, K, R, one_hot=True)
        want_h = np.ascontiguousarray(Bh[:, T.one_hot_rank(M, K, R)].T)
        for ld in (K, K + 3):
            got = _reconstruct(dev, A, B, ld)
            ratio = T.worst_ratio(got, ref, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (R, ld, ratio)
            assert np.array_equal(got.view(np.uint32), _reconstruct(dev, A, B, ld).view(np.uint32)), (R, ld)
            # one-hot A: out[m][k] is B[k][r(m)] itself -- the MFMA output lane map and the wave / tile offsets
            got_h = _reconstruct(dev, Ah, Bh, ld)
            assert np.array_equal(got_h.view(np.uint32), want_h.view(np.uint32)), (R, ld)
        print(f'reconstruct {M}x{K} rank {R}: worst error / bound so far = {worst:.3f}')
    record('trainer_parity', kernel='reconstruct', shape=[M, K], worst_ratio=worst)


# ---- the fused one-layer path ----------------------------------------------------------------------------------------------
def _slab_sum(slab, nsplit, rows_pad, r_pad, rows, R, from_zero):
    """fp32 sum over the splits in apply_kernel's order: the numerator starts from 0.f and adds the slabs in order (its
    rounds of 16 and 8 add in that order too), the denominator starts from slab 0."""
    s = slab.view(nsplit, rows_pad, r_pad)[:, :rows, :R].cpu()
    acc = torch.zeros(rows, R) if from_zero else s[0].clone()
    for i in range(0 if from_zero else 1, nsplit):
        acc = acc + s[i]
    return acc.numpy()


def _fused_param_step(eng, which, case, ortho):
    """One parameter: partial launch -> slab sums -> reference; trainer_step from the same state -> checks."""
    from torchnmf_amd import _capi
    st = eng.step_w if which == 'W' else eng.step_h
    owner, other = st.owner, st.panel
    rows, R, r_pad = owner.rows, case['R'], st.r_pad
    kl = case['beta'] == 1.0
    dev = owner.f.device
    assert st.struct.stage == _capi.STAGE_DMA          # both operand images are live and refreshed by the apply
    theta = owner.f.cpu().numpy().copy()
    other_cs = other.colsum.cpu().numpy()[:R].copy()
    st.slab_num.fill_(NAN)
    if st.slab_den is not None:
        st.slab_den.fill_(NAN)
    eng._partial(st, which.lower())
    torch.cuda.synchronize()
    slabs = (st.slab_num.clone(), None if kl else st.slab_den.clone())
    num = _slab_sum(st.slab_num, st.nsplit, owner.rows_pad, r_pad, rows, R, True)
    pos = np.broadcast_to(other_cs, theta.shape) if kl else _slab_sum(st.slab_den, st.nsplit, owner.rows_pad, r_pad, rows, R, False)
    assert bool(np.isfinite(num).all() and np.isfinite(pos).all())
    gamma, l1, l2 = float(st.struct.gamma), float(st.struct.l1), float(st.struct.l2)
    assert gamma == T.mu_gamma(case['beta'])
    ref, _ = T.update(theta, num, pos, gamma, l1, l2, ortho)
    bound = T.update_bound(theta, num, pos, gamma, l1, l2, ortho, c_rs=T.rowsum_ops_apply(R))
    want_grad = T.grad_f32(num, pos)

    n = rows * R
    gbuf = _guarded(n, dev)
    eng.status.zero_()
    eng.trainer_step(which, ortho, gbuf[:n].view(rows, R))
    torch.cuda.synchronize()
    out = {'nsplit': st.nsplit}
    assert _guards_ok([n], gbuf)
    # trainer_step ran the partial launch again: the same slabs, bit for bit
    assert torch.equal(st.slab_num.view(torch.int32), slabs[0].view(torch.int32))
    assert kl or torch.equal(st.slab_den.view(torch.int32), slabs[1].view(torch.int32))
    new = owner.f.cpu().numpy().copy()
    grad = _host(gbuf, n, (rows, R)).copy()
    out['ratio'] = T.worst_ratio(new, ref, bound)
    out['grad_mismatch'] = int((grad.view(np.uint32) != want_grad.view(np.uint32)).sum())
    out['image_mismatch'] = _check_images(owner, r_pad, case['prec'], False)
    full = owner.f.cpu().double()
    cs = owner.colsum.cpu().double()
    out['colsum'] = float(((cs[:R] - full.sum(0)).abs() / full.sum(0).abs().clamp_min(1e-30)).max())
    out['colsum_pad'] = float(cs[R:].abs().max()) if R < r_pad else 0.0
    out['status'] = int(eng.status.item())
    # the apply alone, again, from the restored master and the slabs still in place: bit-identical
    owner.f.copy_(torch.from_numpy(theta))
    gbuf[:n] = NAN
    eng.be.trainer_apply(st, other.colsum if kl else None, ortho, gbuf[:n].view(rows, R))
    torch.cuda.synchronize()
    out['rerun_equal'] = bool(np.array_equal(owner.f.cpu().numpy().view(np.uint32), new.view(np.uint32))
                              and np.array_equal(_host(gbuf, n, (rows, R)).view(np.uint32), grad.view(np.uint32)))
    return out


@pytest.mark.parametrize('case', T.FUSED_CASES, ids=lambda c: c['id'])
def test_fused_trainer_step_per_element(dev, monkeypatch, case):
    from torchnmf_amd.engine import DenseMU
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    V, W0, H0 = (torch.from_numpy(a) for a in T.fused_problem(case))
    l1, l2, ortho = PEN[case['pen']]
    W, H = W0.to(dev), H0.to(dev)
    eng = DenseMU(V.to(dev), W, H, case['beta'], l1, l2, precision=case['prec'], allow_f16=True)   # as BetaMu._engine does
    assert eng.precision_name == case['prec'] and not eng.gram_path
    torch.cuda.synchronize()
    if case['id'] == 'r5-b1-ns25':
        assert eng.step_h.nsplit == 25                    # 16 + 8 + 1: all three slab-summing loops
    if case['id'] == 'r5-b1-pen-tall':
        assert eng.fH.rows_pad // 64 >= 512 and eng.fW.rows_pad // 64 < 512      # the 64-row and the 16-row instance
    for fac in (eng.fW, eng.fH):
        assert not any(_check_images(fac, eng.r_pad, case['prec'], False).values())
    res = {}
    for which in ('W', 'H'):                               # H's step reads the images and column sums W's step left
        res[which] = r = _fused_param_step(eng, which, case, ortho)
        print(f"fused {case['id']} {which} (nsplit {r['nsplit']}): worst error / bound = {r['ratio']:.3f}")
    record('trainer_parity', kernel='fused', case=case['id'], **{k: v['ratio'] for k, v in res.items()},
           nsplit=[res['W']['nsplit'], res['H']['nsplit']])
    for which, r in res.items():
        assert r['ratio'] <= 1.0, (which, r)
        assert r['grad_mismatch'] == 0 and not any(r['image_mismatch'].values()), (which, r)
        assert r['colsum'] <= 1e-6 and r['colsum_pad'] == 0.0 and r['status'] & 1 == 0 and r['rerun_equal'], (which, r)


# ---- a chain of three layers, end to end -----------------------------------------------------------------------------------
_chain_refs = {}


def _chain_ref(which, beta, pen):
    key = (which, beta, pen)
    if key not in _chain_refs:
        V, X0, Ws = T.chain_problem()
        _chain_refs[key] = T.chain_step(V, X0, Ws, which, beta, *PEN[pen])
    return _chain_refs[key]


@pytest.mark.parametrize('pen', T.CHAIN_PENS)
@pytest.mark.parametrize('beta', T.CHAIN_BETAS)
def test_chain_step_per_element(dev, beta, pen):
    from torch import nn
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import BetaMu
    V, X0, Ws = T.chain_problem()
    V, X0, Ws = torch.from_numpy(V), torch.from_numpy(X0), [torch.from_numpy(w) for w in Ws]
    Vd = V.to(dev)
    worst, worst_g = 0.0, 0.0
    for which in range(4):                                 # one optimiser per parameter, each from the start state
        m = nn.Sequential(NMF(W=Ws[0].clone(), H=X0.clone()), NMF(W=Ws[1].clone()), NMF(W=Ws[2].clone())).to(dev)
        p = [m[0].H, m[0].W, m[1].W, m[2].W][which]
        trainer = BetaMu([p], beta, *PEN[pen])

        def closure():
            trainer.zero_grad()
            return Vd, m(None)
        trainer.step(closure)
        torch.cuda.synchronize()
        assert trainer.last_precision is None              # the chain path, not a fused binding
        ref = _chain_ref(which, beta, pen)
        ratio = T.worst_ratio(p.data.cpu().numpy(), ref['new'], ref['bound'])
        rg = T.worst_ratio(p.grad.cpu().numpy(), ref['grad'], ref['grad_bound'])
        print(f'chain beta {beta:g} {pen} parameter {which}: worst error / bound = {ratio:.3f} (new), {rg:.3f} (grad)')
        worst, worst_g = max(worst, ratio), max(worst_g, rg)
        assert ratio <= 1.0 and rg <= 1.0, (which, ratio, rg)
        for q, src in zip((m[0].H, m[0].W, m[1].W, m[2].W), (X0, Ws[0], Ws[1], Ws[2])):   # nobody else moved
            assert q is p or torch.equal(q.data.cpu(), src)
    record('trainer_parity', kernel='chain', beta=beta, pen=pen, worst_ratio=worst, worst_ratio_grad=worst_g)


# ---- one convolutive layer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', T.CONV_BETAS)
def test_conv_step_per_element(dev, beta):
    from torchnmf_amd.nmf import NMFD
    from torchnmf_amd.trainer import BetaMu, _ConvBinding
    V, W0, H0 = (torch.from_numpy(a) for a in T.conv_problem())
    Vd = V.to(dev)
    ortho, gamma = T.CONV_ORTHO, T.mu_gamma(beta)
    b = _ConvBinding(Vd, W0.to(dev), H0.to(dev), beta, 'auto')
    res = {}
    for name, fn, theta in (('W', b.grads_w, W0), ('H', b.grads_h, H0)):
        neg, pos = (x.cpu().numpy().copy() for x in fn())
        neg2, pos2 = (x.cpu().numpy().copy() for x in fn())
        assert np.array_equal(neg.view(np.uint32), neg2.view(np.uint32)) and np.array_equal(pos.view(np.uint32), pos2.view(np.uint32))
        assert neg.shape == tuple(theta.shape) == pos.shape
        m = NMFD(W=W0.clone(), H=H0.clone()).to(dev)
        p = getattr(m, name)
        trainer = BetaMu([p], beta, 0, 0, ortho)

        def closure():
            trainer.zero_grad()
            return Vd, m()
        trainer.step(closure)
        torch.cuda.synchronize()
        th = theta.numpy()
        # trainer.py:105-106 of the reference: p.sum(1, keepdims=True) - p over the parameter's own layout (dim 1 = rank);
        # five fp32 additions form the device's sum in whatever order: c_rs = R - 1
        rowsum = th.astype(np.float64).sum(1, keepdims=True)
        ref, _ = T.update(th, neg, pos, gamma, 0.0, 0.0, ortho, rowsum=rowsum)
        bound = T.update_bound(th, neg, pos, gamma, 0.0, 0.0, ortho, c_rs=th.shape[1] - 1, rowsum=rowsum)
        res[name] = ratio = T.worst_ratio(p.data.cpu().numpy(), ref, bound)
        print(f'conv beta {beta:g} {name}: worst error / bound = {ratio:.3f}')
        assert ratio <= 1.0, (name, ratio)
        assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), T.grad_f32(neg, pos).view(np.uint32)), name
        other = m.H if name == 'W' else m.W
        assert torch.equal(other.data.cpu(), H0 if name == 'W' else W0)
    record('trainer_parity', kernel='conv', beta=beta, **res)
