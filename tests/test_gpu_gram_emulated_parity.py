"""The beta == 2 path that fit() runs (DenseMU(allow_gram=True)) per element against the rounding-exact emulation.

test_gpu_emulated_parity.py builds its engines without ``allow_gram``, so its beta == 2 cases run the reconstruction
kernels; fit() never does.  Here, stage by stage and each stage emulated from what the GPU holds at that point
(tests/mu_emulation.py, section "beta == 2 without the reconstruction"):

* nmfmu_gram_panel: every element of the fp32 Gram matrix against the float64 product of the read-back image under a bound
  derived from the summation chain, the hi / lo images and row scales bit for bit, padding, determinism;
* the kModeXB instance of fused_kernel: every numerator element (summed over the splits) and every element of the ONE
  denominator slab, slabs poisoned with NaN first; then the apply (fused epilogue, or the apply kernel with den_nslab = 1):
  every element of the fp32 master, the images bit-exact with zero padding, no range-clamp status;
* nmfmu_xb_partial (a public entry without a caller in the engine): the same numerator bits, the denominator slab untouched;
* one whole iteration on the Gram path against one on the reconstruction path from the same state.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import record
import mu_emulation as E
from test_gpu_emulated_parity import _check_images, _image_bits, _img_dtype, _ncu, _offsets, _read_images

pytestmark = pytest.mark.gpu

POISON = 0x7fc00abc     # a quiet NaN with a payload: "nobody wrote here"


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _read_p2(fac, r_pad, prec):
    """The transposed image P2 (what gram_partial_kernel and the XB stream read) as float64 [rows_pad, r_pad]."""
    bits = _image_bits(fac.p2_hi, _offsets(fac.rows_pad, r_pad, 2))
    return torch.from_numpy(bits).view(_img_dtype(prec)).double().numpy()


def _gram_readback(gm, r_pad):
    _, gram, hi, lo, scale = gm
    words = lambda t: t[:r_pad * r_pad * 2].view(torch.int16).cpu().numpy().view(np.uint16).reshape(r_pad, r_pad)
    return gram.view(r_pad, r_pad).cpu().numpy(), words(hi), words(lo), scale.cpu().numpy()


def _poison_gram(gm):
    ws, gram, hi, lo, scale = gm
    ws.fill_(0xff)                       # fp32 0xffffffff: NaN
    gram.fill_(float('nan'))
    hi.fill_(0xff)
    lo.fill_(0xff)
    scale.fill_(float('nan'))


# ---- the Gram matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', E.gram_cases(), ids=lambda c: c['id'])
def test_gram_panel_per_element(dev, case):
    """nmfmu_gram_panel on a poisoned workspace / outputs.

    Bound on the fp32 matrix: an element is a sum of non-negative products of 16-bit values, each exact in fp32, so the
    error of ANY summation order is at most depth * 2^-24 * (the element) to first order, depth = the longest chain of
    sequential fp32 additions a product passes through (mu_emulation.gram_plan, counted from nmfmu_gram.hip): 16 inside its
    MFMA (K = 16, order undocumented) + 4 MFMA accumulations per tile * tiles per chunk + ceil(nchunk / ngrp) chunk
    partials per finalize group + (ngrp - 1) groups.  ``n_seq`` is written out per case (25 .. 79) and checked against the
    mirror.  Symmetry: bit for bit, or else within twice the bound (two elements, each within the bound of the same exact
    value).  Measured on the MI355X over the 20 cases: largest relative error 2.6e-7 (66000 x 40, f16), largest fraction of
    the bound 0.11 (300 x 200, f16: 1.6e-7 against 25 * 2^-24); the matrix is symmetric bit for bit in every case; hi never
    exceeds 900 (entries x 200: Gram maximum 1.9e9)."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import FactorBuf, HipBackend
    be = HipBackend()
    rows, rank, prec = case['rows'], case['rank'], case['precision']
    f16 = prec == 'f16'
    r_pad, P = be.pad_rank(rank), _capi.PRECISIONS[prec]
    plan = E.gram_plan(rows, r_pad)
    assert plan['n_seq'] == case['n_seq'], plan
    F = E.gram_problem(case).to(dev)
    fb = FactorBuf(F, r_pad, P, be)
    be.pack_factor(fb, rank, r_pad, P)
    gm = be.gram_alloc(r_pad, dev)
    _poison_gram(gm)
    be.gram_panel(fb, r_pad, P, gm)
    torch.cuda.synchronize()
    G, hi, lo, scale = _gram_readback(gm, r_pad)
    img = _read_p2(fb, r_pad, prec)
    assert not img[rows:].any() and not img[:, rank:].any()            # the image's own padding
    ref = E.gram_matrix(img)
    excess = E.gram_excess(G, ref, case['n_seq'])
    sym_bits = bool(np.array_equal(G, G.T))
    sym = 0.0 if sym_bits else E.gram_excess(G, G.T.astype(np.float64), 2 * case['n_seq'])
    pad_zero = not G[rank:].any() and not G[:, rank:].any()
    w_hi, w_lo, w_scale = E.gram_images(G, r_pad, f16)
    bad = dict(hi=int((hi != w_hi).sum()), lo=int((lo != w_lo).sum()), scale=int((scale.view(np.uint32) != w_scale.view(np.uint32)).sum()))
    first = [t.clone() for t in gm[1:]]
    be.gram_panel(fb, r_pad, P, gm)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, gm[1:]))
    hi_v = E.image_values(hi, f16)
    record('gram_per_element', case=case['id'], n_seq=case['n_seq'], bound_rel=case['n_seq'] * 2.0 ** -24,
           max_rel=float((np.abs(G[:rank, :rank] - ref[:rank, :rank]) / ref[:rank, :rank]).max()), fraction_of_bound=excess,
           symmetric_bitwise=sym_bits, symmetry_excess=sym, image_mismatch=bad, reproducible=same,
           max_hi=float(np.abs(hi_v).max()), max_gram=float(G.max()))
    assert excess <= 1.0, excess
    assert sym_bits or sym <= 1.0, sym
    assert pad_zero
    assert not any(bad.values()), bad
    assert np.all(scale[rank:] == 1.0) and np.isfinite(hi_v).all() and float(np.abs(hi_v).max()) <= 1024.0   # (a maximum just below 2^10 rounds up to it)
    if case['scale'] > 1:
        assert G.max() > E.F16_MAX                                     # the case is what it says: only the scale keeps hi finite
    assert same


# ---- the XB half-steps ----------------------------------------------------------------------------------------------
def _engine(dev, case, monkeypatch, allow_gram=True):
    from torchnmf_amd.engine import DenseMU
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    V, W0, H0 = E.make_problem(case)
    W, H = W0.clone().to(dev), H0.clone().to(dev)
    eng = DenseMU(V.to(dev), W, H, 2.0, *case['regs'], precision=case['precision'], allow_gram=allow_gram)
    return eng, V


def _gram_values(gm, r_pad, f16):
    _, hi, lo, scale = _gram_readback(gm, r_pad)
    return E.image_values(hi, f16), E.image_values(lo, f16), scale.astype(np.float64)


def _poison_slabs(st):
    st.slab_num.view(torch.int32).fill_(POISON)
    st.slab_den.view(torch.int32).fill_(POISON)


def _xb_half_step(eng, st, which, case, V):
    """One half-step in stages; returns the recorded maxima."""
    prec, R = case['precision'], case['R']
    f16 = prec in E.F16_OPS
    be, gm = eng.be, eng.gm
    owner, panel = st.owner, st.panel
    M, K, r_pad = owner.rows, panel.rows, st.r_pad
    l1, l2, gamma = st.struct.l1, st.struct.l2, st.struct.gamma
    X = (V.t() if which == 'w' else V).numpy()
    # 1. the Gram matrix of the panel
    _poison_gram(gm)
    be.gram_panel(panel, r_pad, eng.precision, gm)
    torch.cuda.synchronize()
    g_hi, g_lo, g_scale = _gram_values(gm, r_pad, f16)
    assert R < 3 or len({g_scale[0], g_scale[1], g_scale[2]}) > 1       # (make_problem: neighbouring rows, unlike scales)
    A = _read_images(owner, r_pad, prec)[0]
    B = _read_images(panel, r_pad, prec)[0]
    em = E.xb_half_step(X, A[:M], B[:K], g_hi, g_lo, g_scale, prec)
    theta = owner.f.cpu().numpy().astype(np.float64)
    fused = st.nsplit == 1 and r_pad <= 128
    out = {'fused': fused}
    eng.status.zero_()
    if not fused:
        # 2. the kernel alone: nsplit numerator slabs and ONE denominator slab, every element of both written
        _poison_slabs(st)
        be.xb_step(st, gm, 1)
        torch.cuda.synchronize()
        num = st.slab_num.view(st.nsplit, owner.rows_pad, r_pad).double().sum(0).cpu().numpy()
        den = st.slab_den.view(owner.rows_pad, r_pad).double().cpu().numpy()
        out['num'] = float(E.elem_err(num[:M, :R], em['num'][:, :R], em['num_amb']).max())
        out['den'] = float(E.elem_err(den[:M, :R], em['den'][:, :R]).max())
        pad = np.ones(num.shape, dtype=bool)
        pad[:M, :R] = False
        out['pad_nonzero'] = int((num[pad] != 0).sum() + (den[pad] != 0).sum())     # (NaN poison counts as non-zero)
        if case['target'] == 'zero_row':
            row = min(3, M - 1) if which == 'h' else min(5, M - 1)
            out['zero_row_num'] = float(np.abs(num[row]).max())
        # 3. the apply kernel on those slabs
        be.xb_step(st, gm, 2)
    else:
        be.xb_step(st, gm, 0)          # 2 + 3 in the kernel's epilogue
    torch.cuda.synchronize()
    new = owner.f.cpu().numpy().astype(np.float64)
    ref = E.apply(theta, em['num'][:, :R], em['den'][:, :R], 2.0, gamma, l1, l2)
    allow = E.apply_allowance(ref, em['num'][:, :R], em['den'][:, :R], em['num_amb'], 0.0, 2.0, gamma, l1=l1, l2=l2, theta=theta)
    out['master'] = float(E.elem_err(new, ref, allow).max())
    out['image_mismatch'] = _check_images(owner, r_pad, prec, False)
    out['status'] = int(eng.status.item())
    return out


def _xb_plan(case):
    return E.half_step_plan(case['N'], case['C'], case['R'], case['precision'], 2.0, _ncu(), case['nsplit'], None, gram=True)


@pytest.mark.parametrize('case', E.xb_cases(_ncu()), ids=lambda c: c['id'])
def test_xb_half_steps_per_element(dev, monkeypatch, case):
    """W and H half-step of the Gram path in stages (Gram images -> kernel -> apply), each emulated from the GPU's own state.

    Tolerance: E.TOL[precision] per element for numerator, denominator slab and master -- the project's bar for "fp32
    accumulation order only", which is all that is left once the emulation takes the images, the Gram image pair and the
    row scales as the GPU holds them.  The owner's column sums are NOT asserted: this path skips their finalize on purpose
    (nmfmu_capi.hip:441 -- beta == 2 reads neither the closed-form denominators nor the fp16 scale).
    Largest per-element errors measured on the MI355X over the 57 cases (numerator / denominator slab / master): bf16
    5.8e-7 / 5.4e-7 / 7.9e-7, f16 5.4e-7 / 5.3e-7 / 7.6e-7 (both against 2.5e-6), f16x 5.7e-7 / 4.0e-7 / 7.6e-7 (against
    2e-6); no poison left, padding exactly zero, the zero rows' numerators exactly zero."""
    plan = _xb_plan(case)
    prec, R = case['precision'], case['R']
    assert {plan['w']['family'], plan['h']['family']} == {'xb'}
    for cl in case['claims']:
        assert any(E.claim_holds(cl, plan[w], R) for w in ('w', 'h')), (cl, plan)
    eng, V = _engine(dev, case, monkeypatch)
    assert eng.gram_path
    for w, st in (('w', eng.step_w), ('h', eng.step_h)):
        assert (st.block_rows, st.nsplit) == (plan[w]['block_rows'], plan[w]['nsplit']), (w, plan[w])
    torch.cuda.synchronize()
    for fac in (eng.fW, eng.fH):
        assert not any(_check_images(fac, eng.r_pad, prec, False).values())
    res = {w: _xb_half_step(eng, st, w, case, V) for w, st in (('w', eng.step_w), ('h', eng.step_h))}
    tol = E.TOL[prec]
    record('xb_per_element', case=case['id'], tol=tol, nsplit=(eng.step_w.nsplit, eng.step_h.nsplit),
           tiles=(plan['w']['tiles'], plan['h']['tiles']), **res)
    for w in ('w', 'h'):
        r = res[w]
        assert r.get('num', 0.0) <= tol and r.get('den', 0.0) <= tol and r['master'] <= tol, (w, r)
        assert r.get('pad_nonzero', 0) == 0 and r.get('zero_row_num', 0.0) == 0.0, (w, r)
        assert not any(r['image_mismatch'].values()), (w, r['image_mismatch'])
        assert r['status'] & 1 == 0, (w, r)


def test_f16x_leaves_the_gram_path_above_rank_128(dev):
    """'f16x' has no kModeXB instance at padded rank 256 (nmfmu_xb_supported): the engine must say so, not run one."""
    from torchnmf_amd.engine import DenseMU
    g = torch.Generator().manual_seed(2)
    V, W, H = torch.rand(130, 260, generator=g), torch.rand(260, 200, generator=g), torch.rand(130, 200, generator=g)
    assert not DenseMU(V.to(dev), W.to(dev), H.to(dev), 2.0, precision='f16x', allow_gram=True).gram_path
    assert DenseMU(V.to(dev), W.to(dev), H.to(dev), 2.0, precision='f16', allow_gram=True).gram_path


def test_xb_partial_numerator_only(dev, monkeypatch):
    """nmfmu_xb_partial (numerator slabs only, for callers that reduce across ranks before the apply): the numerator slabs
    of nmfmu_xb_step's kernel bit for bit -- empty split's zeros included -- and not one word of the denominator slab."""
    case = next(c for c in E.xb_cases(_ncu()) if c['id'].startswith('xb-f16-130x2304r128-ns7'))
    eng, _ = _engine(dev, case, monkeypatch)
    st, be = eng.step_h, eng.be
    assert st.nsplit == 7 and 0 in _xb_plan(case)['h']['tiles']
    be.gram_panel(st.panel, st.r_pad, eng.precision, eng.gm)
    _poison_slabs(st)
    be.xb_step(st, eng.gm, 1)
    torch.cuda.synchronize()
    want = st.slab_num.clone()
    assert torch.isfinite(want).all() and torch.isfinite(st.slab_den).all()
    _poison_slabs(st)
    from torchnmf_amd import _capi
    _capi.check(be.lib.nmfmu_xb_partial(C.byref(st.struct), be.stream()), 'nmfmu_xb_partial')
    torch.cuda.synchronize()
    assert torch.equal(st.slab_num.view(torch.int32), want.view(torch.int32))
    assert bool((st.slab_den.view(torch.int32) == POISON).all())


def test_gram_path_against_reconstruction_path(dev, monkeypatch):
    """One whole iteration with allow_gram=True and one with allow_gram=False from the same state, (384, 1100, 64) in f16:
    the only check that ties the path fit() runs to the path test_gpu_emulated_parity.py covers.

    Bound per element of W and H: |emulation of the Gram path - emulation of the reconstruction path| + TOL (|one| + |other|)
    -- each GPU path is within TOL of its own emulation (the two per-element suites), so the GPU paths differ by no more.
    Both emulations run on the CPU from what each engine holds: its images, and on the Gram path the Gram image pair of the
    same iteration (left in eng.gm by each half-step, whose panel the half-step does not change).  The reconstruction
    path rounds S to fp16 per element; the roundings its emulation cannot predict are allowed for as in its own suite
    (apply_allowance), and that allowance's largest share of an element's bound is recorded next to the result.
    Measured: the paths differ by up to 5.4e-5 (W) / 3.3e-5 (H) relative, which IS the emulations' own difference (the
    fp16 rounding of S); largest fraction of the bound 0.91 / 0.85, the allowance at most 0.81 / 0.70 of a bound."""
    case = dict(N=384, C=1100, R=64, precision='f16', beta=2.0, nsplit=None, regs=(0.0, 0.0), target='rand')
    eg, V = _engine(dev, case, monkeypatch, allow_gram=True)
    er, _ = _engine(dev, case, monkeypatch, allow_gram=False)
    assert eg.gram_path and not er.gram_path
    r_pad, R, tol = eg.r_pad, 64, E.TOL['f16']
    worst = {}
    for w in ('w', 'h'):
        X = (V.t() if w == 'w' else V).numpy()
        em, new, allow = {}, {}, {}
        for name, eng in (('gram', eg), ('recon', er)):
            st = eng.step_w if w == 'w' else eng.step_h
            M, K = st.owner.rows, st.panel.rows
            A = _read_images(st.owner, r_pad, 'f16')[0][:M]
            B = _read_images(st.panel, r_pad, 'f16')[0][:K]
            theta = st.owner.f.cpu().numpy().astype(np.float64)
            (eng.w_step if w == 'w' else eng.h_step)()
            torch.cuda.synchronize()
            if name == 'gram':
                hs = E.xb_half_step(X, A, B, *_gram_values(eng.gm, r_pad, True), 'f16')
            else:
                hs = E.half_step(X, None, None, 2.0, 'f16', A_img=(A, None), B_img=(B, None))
            em[name] = E.apply(theta, hs['num'][:, :R], hs['den'][:, :R], 2.0, 1.0)
            amb = hs['den_amb'] if np.ndim(hs['den_amb']) == 0 else hs['den_amb'][:, :R]
            allow[name] = E.apply_allowance(em[name], hs['num'][:, :R], hs['den'][:, :R], 0.0, amb, 2.0, 1.0)
            new[name] = st.owner.f.cpu().numpy().astype(np.float64)
        # (the reconstruction path rounds S to fp16: the roundings it cannot predict are allowed for as in its own suite)
        bound = np.abs(em['gram'] - em['recon']) + tol * (np.abs(em['gram']) + np.abs(em['recon'])) + allow['gram'] + allow['recon']
        diff = np.abs(new['gram'] - new['recon'])
        worst[w] = dict(max_rel_diff=float((diff / np.abs(new['recon'])).max()), fraction_of_bound=float((diff / bound).max()),
                        emulations_rel_diff=float((np.abs(em['gram'] - em['recon']) / np.abs(em['recon'])).max()),
                        allowance_share_of_bound=float(((allow['gram'] + allow['recon']) / bound).max()))
    record('gram_vs_reconstruction', **worst)
    assert worst['w']['fraction_of_bound'] <= 1.0 and worst['h']['fraction_of_bound'] <= 1.0, worst
