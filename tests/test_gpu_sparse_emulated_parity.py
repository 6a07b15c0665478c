"""The sparse-COO MU path per element against a float64 reference (tests/sparse_emulation.py).

For every case of ``sparse_emulation.parity_cases`` (every RL instantiation and pad_rank class, beta in {1, 2, 0.5, 1.5, 3},
with and without regularisation, split-bf16 and bf16 images of the generic denominator pass, forced contraction splits,
owner-row counts off the 4-row workgroups and below the 64 Gram chunks on both axes, rows of 0 .. 5 and C entries, an empty
column, duplicates, a stored 0.0, an owner row of zeros, no entry at all, a larger skewed target on sampled rows) the
``SparseMU`` engine runs one W and one H half-step, each emulated from the state read back from the device:

* control flow: the precision, padded rank and contraction splits the engine chose, against the host mirror;
* CSR: ``csr_h`` / ``csr_w`` bit-equal to ``sparse_emulation.csr``; ``target_flags()``;
* numerator (nmfmu_sp_partial alone, buffers poisoned with NaN): every element of rows < owner.rows, columns < rank within
  ``numerator_bound`` -- k u sum |g panel|, k from the operations of the kernel; padded rank columns exactly 0; no NaN left;
* denominator: beta == 2 the Gram matrix and ``den1`` per element within their bounds; generic beta ``den1`` against
  ``mu_emulation.half_step`` on the image planes read back, at ``mu_emulation.TOL``; beta == 1 the column sums at 1e-6;
* step: every element of the new fp32 master (``mu_emulation.elem_err``, the numerator / denominator bounds propagated
  through ``apply_allowance``) within APPLY_OPS u (generic beta: ``mu_emulation.TOL``), P1 / P2 images bit-exact and zero in
  the padding, column sums;
* loss: nmfmu_sp_loss_neg's output, the workgroup partials summing to it, ``pos`` and ``divergence()`` against float64.

No element is excluded on the fp32 paths (beta in {1, 2}); every bound is derived in sparse_emulation's docstring, none from
a run.  Measured on the MI355X, the largest fraction of the bound used over all 42 cases (also in DESIGN.md section 4):
numerator 0.62 (beta in {1, 2}) / 0.35 (generic), Gram matrix 0.13, beta == 2 den1 0.07, master 0.34 of APPLY_OPS u (generic:
0.50 of TOL), neg 0.14, pos 0.03, divergence 0.10; generic den1 <= 2.9e-6 after the allowance (9.7e-5 before it, bf16);
column sums <= 2.9e-7; images, padded columns and CSR arrays exact.  The file takes 5 s.
"""
import numpy as np
import pytest
import torch

from conftest import record
import mu_emulation as E
import sparse_emulation as S
from test_gpu_emulated_parity import _check_images, _read_images

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _np(t):
    return t.detach().cpu().numpy()


def _half_step(eng, st, csr_dev, csr_ref, which, case, pl, rows):
    """One half-step in its three stages against the reference; returns the measured maxima (bounds: 1.0 = the bound)."""
    beta, R = case['beta'], case['R']
    own, pan = st.owner, st.panel
    r_pad, prec = st.r_pad, pl['precision']
    kind = E.beta_kind(beta)
    l1, l2, gamma = st.struct.l1, st.struct.l2, st.struct.gamma
    sel = np.arange(own.rows) if rows is None else rows
    theta_all = _np(own.f).astype(np.float64)
    theta, P = theta_all[sel], _np(pan.f).astype(np.float64)
    em = S.numerator(csr_ref, theta_all, P, beta, rows=sel)
    nb = S.numerator_bound(em)
    out = {'rows': int(len(sel)), 'excluded': 0}
    # ---- numerator
    st.num1.fill_(float('nan'))
    if st.den1 is not None:
        st.den1.fill_(float('nan'))
    eng._numerator(st, csr_dev)
    torch.cuda.synchronize()
    num = _np(st.num1).reshape(own.rows_pad, r_pad)
    out['num_nan'] = int(np.isnan(num[:own.rows]).sum())
    out['num_pad'] = float(np.abs(num[:own.rows, R:]).max()) if R < r_pad else 0.0
    out['num'] = float(S.bound_err(num[sel, :R], em['num'], nb).max())
    # ---- denominator
    den_ref, db, den_amb, kl_den, tol = None, 0.0, 0.0, None, S.APPLY_OPS * S.U
    if pl['generic']:
        st.slab_num.fill_(float('nan'))       # (an empty contraction split must still write its zeros)
    eng._denominator(st)
    torch.cuda.synchronize()
    if kind == 'kl':
        kl_den = _np(pan.colsum).astype(np.float64)
        cs = P.sum(0)
        out['colsum_panel'] = float((np.abs(kl_den[:R] - cs) / np.maximum(np.abs(cs), 1e-30)).max())
    elif kind == 'euc':
        g, gb = S.gram(P)
        out['gram'] = float(S.bound_err(_np(eng.gram).reshape(R, R), g, gb).max())
        den_ref, db = S.rowmat(theta, g, pan.rows)
        den = _np(st.den1).reshape(own.rows_pad, r_pad)
        out['den_nan'] = int(np.isnan(den[:own.rows]).sum())
        out['den_pad'] = float(np.abs(den[:own.rows, R:]).max()) if R < r_pad else 0.0
        out['den'] = float(S.bound_err(den[sel, :R], den_ref, db).max())
    else:
        A_hi, A_lo = _read_images(own, r_pad, prec)
        B_hi, B_lo = _read_images(pan, r_pad, prec)
        pick = lambda im, r: None if im is None else im[r][:, :R]
        ed = S.generic_den((pick(A_hi, sel), pick(A_lo, sel)), (pick(B_hi, slice(0, pan.rows)), pick(B_lo, slice(0, pan.rows))),
                           beta, prec, own.rows, pan.rows)
        den_ref, den_amb = ed['den'], ed['den_amb']
        den = _np(st.den1).reshape(own.rows_pad, r_pad)
        out['den_nan'] = int(np.isnan(den[:own.rows]).sum())
        out['den_pad'] = float(np.abs(den[:own.rows, R:]).max()) if R < r_pad else 0.0
        out['den'] = float(E.elem_err(den[sel, :R], den_ref, den_amb).max())
        out['den_raw'] = float(E.elem_err(den[sel, :R], den_ref).max())
        db, tol = den_amb, E.TOL[prec]
    # ---- apply
    eng._apply(st)
    torch.cuda.synchronize()
    new = _np(own.f).astype(np.float64)
    ref = E.apply(theta, em['num'], den_ref, beta, gamma, l1, l2, kl_den=kl_den)
    allow = E.apply_allowance(ref, em['num'], den_ref, nb, db, beta, gamma, l1=l1, l2=l2, theta=theta)
    out['master'] = float(E.elem_err(new[sel], ref, allow).max() / tol)
    out['master_raw'] = float(E.elem_err(new[sel], ref).max())
    out['image_mismatch'] = _check_images(own, r_pad, prec, False)
    cs, full = _np(own.colsum).astype(np.float64), new.sum(0)
    out['colsum'] = float((np.abs(cs[:R] - full) / np.maximum(np.abs(full), 1e-30)).max())
    out['colsum_pad'] = float(np.abs(cs[R:]).max()) if R < r_pad else 0.0
    return out


def _loss(eng, case, pl, csr_ref, cvals):
    beta, R = case['beta'], case['R']
    H, W = _np(eng.fH.f).astype(np.float64), _np(eng.fW.f).astype(np.float64)
    neg_ref, neg_b = S.loss_neg(csr_ref, H, W, beta)
    eng._launch_neg()
    torch.cuda.synchronize()
    neg = float(eng.loss_out.item())
    part = _np(eng.loss_part)
    out = {'neg': abs(neg - neg_ref) / neg_b if neg_b > 0 else (0.0 if neg == neg_ref else float('inf')),
           'neg_rel': abs(neg - neg_ref) / max(abs(neg_ref), 1e-300),
           'neg_partials': abs(float(part.sum()) - neg) / max(float(np.abs(part).sum()) * len(part) * 2.0 ** -53, 1e-300)}
    imgs = {}
    if pl['generic']:
        A_hi, A_lo = _read_images(eng.fH, eng.r_pad, pl['precision'])
        B_hi, B_lo = _read_images(eng.fW, eng.r_pad, pl['precision'])
        pick = lambda im, n: None if im is None else im[:n, :R]
        tiles = -(-(eng.fW.rows_pad // E.KBK) // eng.step_h.nsplit)
        imgs = dict(A_img=(pick(A_hi, eng.fH.rows), pick(A_lo, eng.fH.rows)), B_img=(pick(B_hi, eng.fW.rows), pick(B_lo, eng.fW.rows)),
                    r_pad=eng.r_pad, tiles=tiles)
    pos_ref, pos_b = S.loss_pos(H, W, beta, **imgs)
    pos = eng._pos()
    out['pos'] = abs(pos - pos_ref) / pos_b
    out['pos_rel'] = abs(pos - pos_ref) / max(abs(pos_ref), 1e-300)
    vn = S.v_norm(cvals, beta)
    vb = S.v_norm_bound(cvals, beta)
    out['v_norm'] = 0.0 if (np.isnan(vn) and np.isnan(eng.v_norm)) else abs(eng.v_norm - vn) / vb
    div, div_ref = eng.divergence(), vn + pos_ref - neg_ref
    out['div_nan'] = (bool(np.isnan(div)), bool(np.isnan(div_ref)))
    scale = abs(pos_ref) + abs(neg_ref) + (0.0 if np.isnan(vn) else abs(vn))
    out['div'] = 0.0 if np.isnan(div_ref) else abs(div - div_ref) / (neg_b + pos_b + vb + 4 * 2.0 ** -53 * scale)
    return out


@pytest.mark.parametrize('case', S.parity_cases(), ids=lambda c: c['id'])
def test_sparse_half_steps_per_element(dev, monkeypatch, case):
    from torchnmf_amd import _capi
    from torchnmf_amd.sparse_engine import SparseMU
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    prob = S.make_problem(case)
    for cl in case['claims']:
        assert S.claim_holds(cl, case, prob), cl
    idx, vals, (N, C), W0, H0 = prob
    beta, R = case['beta'], case['R']
    a1, a2 = case['regs']
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    V = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), (N, C)).to(dev)
    assert 'duplicates' not in case['claims'] or not V.is_coalesced()
    W, H = W0.clone().to(dev), H0.clone().to(dev)
    eng = SparseMU(V, W, H, beta, a1 * a2, a1 * (1 - a2))
    # ---- control flow
    pl = S.plan(case, ncu)
    assert eng.prec == {'bf16': _capi.PREC_BF16, 'bf16x3': _capi.PREC_BF16X3}[pl['precision']]
    assert eng.r_pad == pl['r_pad']
    assert (eng.step_h.nsplit, eng.step_w.nsplit) == (pl['nsplit']['h'], pl['nsplit']['w']), pl
    if 'split' in case['claims']:
        assert max(eng.step_h.nsplit, eng.step_w.nsplit) > 1
    # ---- CSR and flags
    cidx, cvals = S.coalesce(idx, vals, (N, C))
    csr_h, csr_w = S.csr(cidx[0], cidx[1], cvals, N), S.csr(cidx[1], cidx[0], cvals, C)
    for got, want in ((eng.csr_h, csr_h), (eng.csr_w, csr_w)):
        for g_, w_ in zip(got, want):
            assert _np(g_).dtype == w_.dtype and np.array_equal(_np(g_).view(np.int32), w_.view(np.int32))
    assert eng.target_flags() == (False, bool(len(cvals) < N * C or (cvals == 0).any()))
    torch.cuda.synchronize()
    for fac in (eng.fW, eng.fH):
        assert not any(_check_images(fac, eng.r_pad, pl['precision'], False).values())
    # ---- the two half-steps, then the loss of the state they leave
    gs = np.random.default_rng(7)
    res = {}
    for w, st, cd, cr in (('w', eng.step_w, eng.csr_w, csr_w), ('h', eng.step_h, eng.csr_h, csr_h)):
        rows = None
        if case['sample']:
            rows = np.sort(gs.choice(st.owner.rows, size=case['sample'], replace=False))
        res[w] = _half_step(eng, st, cd, cr, w, case, pl, rows)
    res['loss'] = _loss(eng, case, pl, csr_h, cvals)
    record('sparse_emulated_parity', case=case['id'], precision=pl['precision'],
           nsplit=(eng.step_w.nsplit, eng.step_h.nsplit), **res)
    for w in ('w', 'h'):
        r = res[w]
        assert r['num_nan'] == 0 and r['num_pad'] == 0.0 and r['num'] <= 1.0, (w, r)
        assert r.get('den_nan', 0) == 0 and r.get('den_pad', 0.0) == 0.0, (w, r)
        assert r.get('gram', 0.0) <= 1.0 and r.get('colsum_panel', 0.0) <= 1e-6, (w, r)
        assert r.get('den', 0.0) <= (E.TOL[pl['precision']] if pl['generic'] else 1.0), (w, r)
        assert r['master'] <= 1.0, (w, r)
        assert not any(r['image_mismatch'].values()), (w, r['image_mismatch'])
        assert r['colsum'] <= 1e-6 and r['colsum_pad'] == 0.0, (w, r)
        assert r['excluded'] == 0
    r = res['loss']
    assert r['neg'] <= 1.0 and r['neg_partials'] <= 1.0 and r['pos'] <= 1.0 and r['v_norm'] <= 1.0, r
    assert r['div_nan'][0] == r['div_nan'][1] and r['div'] <= 1.0, r
