"""Dense MU kernels per element against a rounding-exact emulation (tests/mu_emulation.py).

For every case of ``mu_emulation.parity_cases`` (ping-pong, software-pipelined, two-accumulator and four-wave kernels, all
operand modes, every beta branch, ragged shapes, split and unsplit contractions, empty splits) and for each half-step,
starting from the state the GPU holds:

* the case is what it says: kernel family, tile height and split as the host mirror predicts, and the control flow it is
  named for (empty split, short last split, odd tiles per split, fused apply, ragged M / K / R) in the mirrored tile list;
* partials: every numerator / denominator element of the slabs (poisoned with NaN first), summed over the splits;
* step: every element of the updated fp32 master (fused-apply epilogue where nsplit == 1, slabs + apply kernel otherwise);
* images: P1 / P2 (hi and lo) bit-exact the rounding of the new master, zero on padded rows and rank columns (P2 not
  checked where NMFMU_STAGE_DMA_NOP2 drops it); column sums against float64 sums; no range-clamp status.

Each half-step is emulated from the images read back from the GPU, so errors do not compound from one to the next.
"""
import numpy as np
import pytest
import torch

from conftest import record
import mu_emulation as E
from test_layout_emulation import p1_offset, p2_offset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _cases():
    return E.parity_cases(_ncu())


def _img_dtype(prec):
    return torch.float16 if prec in E.F16_OPS else torch.bfloat16


def _image_bits(buf, offs):
    return buf.view(torch.int16)[torch.from_numpy(offs).to(buf.device)].cpu().numpy()


def _offsets(rows_pad, r_pad, which):
    rr, cc = np.meshgrid(np.arange(rows_pad, dtype=np.int64), np.arange(r_pad, dtype=np.int64), indexing='ij')
    return (p1_offset if which == 1 else p2_offset)(rr, cc, r_pad)


def _bits_of(vals, prec):
    """16-bit words of the image planes of fp32 values (hi, lo) as the kernels write them (pack_img / bf16 lo plane)."""
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32))
    if prec == 'bf16x3':
        hi = t.to(torch.bfloat16)
        lo = (t - hi.float()).to(torch.bfloat16)
        return hi.view(torch.int16).numpy(), lo.view(torch.int16).numpy()
    if prec in E.F16_OPS:
        return t.clamp(max=E.F16_MAX).to(torch.float16).view(torch.int16).numpy(), None
    return t.to(torch.bfloat16).view(torch.int16).numpy(), None


def _read_images(fac, r_pad, prec):
    """(hi, lo or None) of P1 as float64 [rows_pad, r_pad]."""
    offs = _offsets(fac.rows_pad, r_pad, 1)
    dt = _img_dtype(prec) if prec != 'bf16x3' else torch.bfloat16

    def dec(buf):
        return torch.from_numpy(_image_bits(buf, offs)).view(dt).double().numpy()
    return dec(fac.p1_hi), (dec(fac.p1_lo) if fac.p1_lo is not None else None)


def _check_images(fac, r_pad, prec, nop2):
    """Mismatching 16-bit words of P1 / P2 (hi, lo) against the rounding of the fp32 master, padding included."""
    full = np.zeros((fac.rows_pad, r_pad), dtype=np.float32)
    full[:fac.rows, :fac.rank] = fac.f.cpu().numpy()
    want_hi, want_lo = _bits_of(full, prec)
    bad = {}
    for which in ((1,) if nop2 else (1, 2)):
        offs = _offsets(fac.rows_pad, r_pad, which)
        planes = [(f'p{which}_hi', getattr(fac, f'p{which}_hi'), want_hi)]
        if want_lo is not None:
            planes.append((f'p{which}_lo', getattr(fac, f'p{which}_lo'), want_lo))
        for name, buf, want in planes:
            bad[name] = int((_image_bits(buf, offs) != want).sum())
    return bad


def _half_step(eng, st, which, case, V, rows):
    """Partials and step of one half-step against the emulation; returns the recorded maxima."""
    from torchnmf_amd import _capi
    prec, beta, R = case['precision'], case['beta'], case['R']
    owner, panel = st.owner, st.panel
    M, K, r_pad = owner.rows, panel.rows, st.r_pad
    l1, l2 = st.struct.l1, st.struct.l2
    gamma = st.struct.gamma
    X = (V.t() if which == 'w' else V).numpy()
    sel = np.arange(M) if rows is None else rows
    A_hi, A_lo = _read_images(owner, r_pad, prec)
    B_hi, B_lo = _read_images(panel, r_pad, prec)
    pick = lambda im, r: None if im is None else im[r][:, :R]
    cs_o, cs_p = owner.colsum.cpu().numpy(), panel.colsum.cpu().numpy()
    theta = owner.f.cpu().numpy().astype(np.float64)[sel]
    em = E.half_step(X[sel], None, None, beta, prec, M=M, K=K, cs_owner=cs_o, cs_panel=cs_p,
                     A_img=(pick(A_hi, sel), pick(A_lo, sel)), B_img=(pick(B_hi, slice(0, K)), pick(B_lo, slice(0, K))))
    kl = E.beta_kind(beta) == 'kl'
    # ---- partials (slabs poisoned first: an empty workgroup must still write its zeros)
    st.slab_num.fill_(float('nan'))
    if st.slab_den is not None:
        st.slab_den.fill_(float('nan'))
    eng._partial(st, which)
    torch.cuda.synchronize()
    shape = (st.nsplit, owner.rows_pad, r_pad)
    num = st.slab_num.view(shape).double().sum(0).cpu().numpy()[sel, :R]
    e_num = E.elem_err(num, em['num'], em['num_amb'])
    out = {'num': float(e_num.max()), 'num_raw': float(E.elem_err(num, em['num']).max())}
    if not kl:
        den = st.slab_den.view(shape).double().sum(0).cpu().numpy()[sel, :R]
        e_den = E.elem_err(den, em['den'], em['den_amb'])
        out['den'] = float(e_den.max())
        out['den_raw'] = float(E.elem_err(den, em['den']).max())
    # ---- the whole half-step from the same state
    eng.status.zero_()
    if which == 'w':
        eng.w_step()
    else:
        eng.h_step()
    torch.cuda.synchronize()
    new = owner.f.cpu().numpy().astype(np.float64)[sel]
    ref = E.apply(theta, em['num'], em['den'], beta, gamma, l1, l2, kl_den=cs_p)
    allow = E.apply_allowance(ref, em['num'], em['den'], em['num_amb'], em['den_amb'], beta, gamma, l1=l1, l2=l2, theta=theta)
    out['master'] = float(E.elem_err(new, ref, allow).max())
    out['master_raw'] = float(E.elem_err(new, ref).max())
    nop2 = st.struct.stage == _capi.STAGE_DMA_NOP2 and case['family'] == 'sp'
    out['image_mismatch'] = _check_images(owner, r_pad, prec, nop2)
    full = owner.f.cpu().double()
    cs = owner.colsum.cpu().double()
    out['colsum'] = float(((cs[:R] - full.sum(0)).abs() / full.sum(0).abs().clamp_min(1e-30)).max())
    out['colsum_pad'] = float(cs[R:].abs().max()) if R < r_pad else 0.0
    out['status'] = int(eng.status.item())
    return out


@pytest.mark.parametrize('case', _cases(), ids=lambda c: c['id'])
def test_half_steps_per_element(dev, monkeypatch, case):
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    ncu = _ncu()
    N, C, R, prec, beta = case['N'], case['C'], case['R'], case['precision'], case['beta']
    plan = E.half_step_plan(N, C, R, prec, beta, ncu, case['nsplit'], case['block_rows'])
    # the case is what it says (host mirror of the split arithmetic)
    assert {plan['w']['family'], plan['h']['family']} == {case['family']}
    for cl in case['claims']:
        assert any(E.claim_holds(cl, plan[w], R) for w in ('w', 'h')), (cl, plan)
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    V, W0, H0 = E.make_problem(case)
    alpha_l1, alpha_l2 = case['regs']
    stage = _capi.STAGE_DMA_NOP2 if case['stage'] == 'nop2' else _capi.STAGE_DMA
    W, H = W0.clone().to(dev), H0.clone().to(dev)
    eng = DenseMU(V.to(dev), W, H, beta, alpha_l1, alpha_l2, precision=prec, stage=stage, block_rows=case['block_rows'])
    fam = {'pp': _capi.KERNEL_PP, 'sp': _capi.KERNEL_SP, 'sp2': _capi.KERNEL_SP, 'fused': _capi.KERNEL_FUSED}[case['family']]
    if case['block_rows'] is None:
        assert eng.be.kernel_family(eng.r_pad, eng.precision, beta) == fam
    for w, st in (('w', eng.step_w), ('h', eng.step_h)):
        assert (st.block_rows, st.nsplit) == (plan[w]['block_rows'], plan[w]['nsplit']), (w, plan[w])
    torch.cuda.synchronize()
    # the images the first half-step reads (nmfmu_pack_factor)
    for fac in (eng.fW, eng.fH):
        assert not any(_check_images(fac, eng.r_pad, prec, False).values())
    gs = np.random.default_rng(7)
    res = {}
    for w, st in (('w', eng.step_w), ('h', eng.step_h)):
        rows = None
        if case['sample']:
            rows = np.sort(gs.choice(st.owner.rows, size=case['sample'], replace=False))
        res[w] = _half_step(eng, st, w, case, V, rows)
    record('emulated_parity', case=case['id'], tol=E.TOL[prec],
           nsplit=(eng.step_w.nsplit, eng.step_h.nsplit), tiles=(plan['w']['tiles'], plan['h']['tiles']), **res)
    tol = E.TOL[prec]
    for w in ('w', 'h'):
        r = res[w]
        assert r['num'] <= tol and r.get('den', 0.0) <= tol and r['master'] <= tol, (w, r)
        assert not any(r['image_mismatch'].values()), (w, r['image_mismatch'])
        assert r['colsum'] <= 1e-6 and r['colsum_pad'] == 0.0, (w, r)
        assert r['status'] & 1 == 0, (w, r)
