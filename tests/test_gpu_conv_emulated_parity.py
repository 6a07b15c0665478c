"""Convolutive MU kernels (nmfd_engine.ConvMU) per element against a rounding-exact emulation (tests/conv_emulation.py).

For every case of ``conv_emulation.conv_cases`` the test first asserts that the engine took the control flow the case is
there for (operand form, H-numerator path, fused sums / tables, tap fold, contraction splits, tail-round split, ragged
channels, 64-row channel tile, window staging), then runs two full iterations -- the second is the first to use the
partial sums of the fused kernels, the shadow-H table rewrite and the second form of rows_fused.  Before each half-step
the GPU's own fp32 W and H are read as the emulation's start state, so errors do not compound.  Per half-step:

1. ratio planes (gn / gp, gnt / gpt), filled with a NaN pattern first, after the reconstruction launch alone: every valid
   element equals the emulated rounding bit for bit or is ambiguous and equals the other neighbour (at most 2 % of a
   plane may be ambiguous); zero-initialised padding is still zero, other padding finite (zero at beta == 1);
2. numerators / denominators where they exist as buffers, NaN-poisoned first: num_w / den_w (summed over the split-K
   slabs), hnum / hden of the window-operand path (gathered over the folded taps), y / y_den of the store-then-fold path;
   on the fold-parts path the tile diagonal sums are checked through the H update only;
3. the fp32 masters after the step;
4. the operand images after the step: wm, wmt, wk and the explicit hu / hut planes bit-exact against the rounding of the
   new master, zero padding included.  The implicit window tables are not decoded here: check 1 of the following
   half-step reads the reconstruction they produce, and one more ratio check after the last H half-step covers the
   tables it wrote;
5. eng.divergence() after the two iterations against the emulated loss;
6. exact zeros (a silent channel of W, a silent rank segment of H) stay exact zeros.

The numerators and the master are emulated from the ratio words the device wrote (checked one by one in 1.), not from the
emulation's own choice among ambiguous neighbours, so they carry no allowance (conv_emulation.with_device_planes).  The
silent channel's rows of num_w / den_w (1e7 times the others) are judged apart from the live rows.

The case list holds a case for every plan signature (conv_emulation.signature) that the default switches reach on the
grid of tests/test_conv_emulation.py::test_every_default_plan_on_the_grid_has_a_case.

Measured on the MI355X (121 cases, 9 s): every ratio plane, operand image and zero exact; ambiguous share at most 0.18 %
(bf16 / bf16x3) and 0.70 % (f16); numerators, denominators and masters at most 1.6e-6 per element (ragged-in-grid; 1.2e-6
elsewhere, rows-3d-fold1 in split bf16) against mu_emulation.TOL of 2.5e-6 / 4e-6; loss at most 3.2e-7 relative.  No
tolerance is raised.  One finding on the reference side: at rank 40 with 48 taps (3 x 1920 products per element of S) the
fp32 sum of S alone differs from float64 by 1.2e-6, which beta == 0 doubles in Gn -- past the 2e-6 band of the lo-word
check in 10 of 17 280 words; that case runs beta == 1.5 (the note beside it in conv_cases).
"""
import numpy as np
import pytest
import torch

from conftest import record
import conv_emulation as CE
import mu_emulation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _bits(vals, prec):
    """(hi, lo or None) int16 words of fp32 values as pack_img writes them."""
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32))
    if prec == 'bf16x3':
        hi = t.to(torch.bfloat16)
        return hi.view(torch.int16).numpy(), (t - hi.float()).to(torch.bfloat16).view(torch.int16).numpy()
    if prec == 'f16':
        return t.clamp(max=E.F16_MAX).to(torch.float16).view(torch.int16).numpy(), None
    return t.to(torch.bfloat16).view(torch.int16).numpy(), None


def _plane(pl, which='hi'):
    buf = getattr(pl, which)
    return None if buf is None else buf.view(torch.int16).view(pl.rows_pad, pl.cols_pad)


def _poison(eng, names, rows, cols, prec, rz):
    """NaN words into the ratio planes: everywhere, or the valid region alone where the padding is zero-initialised once
    and the GEMM leaves it alone (a NaN there would reach the numerator GEMMs)."""
    for name in names:
        pl = getattr(eng, name)
        if pl is None:
            continue
        for which in ('hi', 'lo'):
            p = _plane(pl, which)
            if p is None:
                continue
            word = CE.nan_word('bf16' if which == 'lo' else prec)
            if rz:
                p[:rows, :cols] = word
            else:
                p.fill_(word)


def _read_planes(eng, names):
    out = {}
    for key, name in names.items():
        pl = getattr(eng, name)
        if pl is not None:
            lo = _plane(pl, 'lo')
            out[key] = (_plane(pl, 'hi').cpu().numpy(), None if lo is None else lo.cpu().numpy())
    return out


def _image_mismatch(pl, full, prec):
    """Mismatching words of a row-major plane set against the rounding of ``full`` [rows_pad][cols_pad] fp32."""
    hi, lo = _bits(full, prec)
    bad = int((_plane(pl, 'hi').cpu().numpy() != hi).sum())
    if lo is not None:
        bad += int((_plane(pl, 'lo').cpu().numpy() != lo).sum())
    return bad


def _padded(mat, rows_pad, cols_pad):
    full = np.zeros((rows_pad, cols_pad), dtype=np.float32)
    full[:mat.shape[0], :mat.shape[1]] = mat
    return full


def _wk_matrix(W, eng):
    """Wk[r F + d][((to TQ + q) CK + ck) 64 + c'] = W[64 ck + c'][r][to T_last + F q + d] (conv_pack_wk_kernel)."""
    C, R = W.shape[:2]
    T, tl, F = eng.T, eng.ts[-1], eng.wk_fold
    ck = -(-C // 64)
    Wp = np.zeros((ck * 64, R, T), dtype=np.float32)
    Wp[:C] = W.reshape(C, R, T)
    x = Wp.reshape(ck, 64, R, T // tl, tl // F, F)                 # (ck, c', r, to, q, d)
    x = x.transpose(2, 5, 3, 4, 0, 1).reshape(R * F, (T // F) * ck * 64)
    return _padded(x, eng.wk.rows_pad, eng.wk.cols_pad)


def _w_images(eng, prec):
    W = eng.W.cpu().numpy()
    wm = W.reshape(W.shape[0], -1)
    bad = {'wm': _image_mismatch(eng.wm, _padded(wm, eng.c_pad, eng.rp_pad), prec),
           'wmt': _image_mismatch(eng.wmt, _padded(wm.T, eng.rp_pad, eng.c_pad), prec)}
    if eng.h_rows:
        bad['wk'] = _image_mismatch(eng.wk, _wk_matrix(W, eng), prec)
    return bad


def _h_images(eng, prec):
    if eng.implicit:
        return {}
    hu = CE.unfold(eng.H.cpu().numpy(), eng.ts).astype(np.float32)
    return {'hu': _image_mismatch(eng.hu, _padded(hu, eng.bl_pad, eng.rp_pad), prec),
            'hut': _image_mismatch(eng.hut, _padded(hu.T, eng.rp_pad, eng.bl_pad), prec)}


def _slabs(buf, nslab, rows, cols, summed):
    a = buf[:nslab * rows * cols].view(nslab, rows, cols).double()
    return (a[0] if summed else a.sum(0)).cpu().numpy()


def _gemm_rows(eng):
    """Channels the reconstruction GEMMs cover (they write their own padding); beyond them the planes are zero-initialised."""
    return eng.c_main if eng.ragged else eng.c_rows


def _exact_channels(eng, prec):
    return tuple(range(eng.c_main, eng.C)) if (eng.ragged and not eng.ragged_in_grid and prec == 'bf16x3') else ()


def _w_half(eng, V, case):
    prec, beta = case['precision'], case['beta']
    l1, l2 = eng.l1, eng.l2
    C, BL, RT = eng.C, eng.B * eng.L, eng.R * eng.T
    rz = eng.ragged or bool(eng.c_rows)
    W0, H0 = eng.W.cpu().numpy(), eng.H.cpu().numpy()
    _poison(eng, ('gn', 'gp'), C, BL, prec, rz)
    eng.recon_ratio_w()
    torch.cuda.synchronize()
    got = {'planes': _read_planes(eng, {'gn': 'gn', 'gp': 'gp'})}
    em = CE.w_half_step(V, W0, H0, beta, prec, l1, l2, exact_channels=_exact_channels(eng, prec), planes=got['planes'])
    eng.num_w.fill_(float('nan'))
    if eng.den_w is not None:
        eng.den_w.fill_(float('nan'))
    eng.w_step()
    torch.cuda.synchronize()
    rows = eng.c_rows or eng.c_pad
    summed = eng.w_ksplit > 2 or (eng.w_ksplit > 1 and bool(eng.c_rows))
    got['num'] = _slabs(eng.num_w, eng.w_ksplit, rows, eng.rp_pad, summed)[:C, :RT]
    got['den'] = None if eng.den_w is None else _slabs(eng.den_w, eng.w_ksplit, rows, eng.rp_pad, summed)[:C, :RT]
    got['new'] = eng.W.cpu().numpy().astype(np.float64)
    ok, fig = CE.check_half_step(got, em, prec, beta, 'w', gemm_rows=_gemm_rows(eng), tol=E.TOL[prec] * case['tol_x'])
    fig['images'] = _w_images(eng, prec)
    return ok and not any(fig['images'].values()), fig


def _gather_rows(buf, eng):
    """num[b][r][jo][j] = sum_d out[(b, jo, j + d)][r F + d] of the window-operand GEMM's output (slab 0 holds the sum)."""
    F, R, B = eng.wk_fold, eng.R, eng.B
    ll = eng.lhs[-1]
    lo = eng.Lh // ll
    out = buf[:eng.hj_pad * eng.wk_rows].view(eng.hj_pad, eng.wk_rows).double().cpu().numpy()
    out = out[:B * lo * (ll + F - 1), :R * F].reshape(B, lo, ll + F - 1, R, F)
    num = sum(out[:, :, d:d + ll, :, d] for d in range(F))          # (B, lo, ll, R)
    return np.moveaxis(num, -1, 1).reshape((B, R) + tuple(eng.lhs))


def _h_half(eng, V, case):
    prec, beta = case['precision'], case['beta']
    C, BL, RT = eng.C, eng.B * eng.L, eng.R * eng.T
    rz = eng.ragged or bool(eng.c_rows)
    W0, H0 = eng.W.cpu().numpy(), eng.H.cpu().numpy()
    _poison(eng, ('gnt', 'gpt'), BL, C, prec, rz)
    eng.recon_ratio_h()
    torch.cuda.synchronize()
    got = {'planes': _read_planes(eng, {'gn': 'gnt', 'gp': 'gpt'})}
    em = CE.h_half_step(V, W0, H0, beta, prec, eng.l1, eng.l2, exact_channels=_exact_channels(eng, prec), planes=got['planes'])
    store_fold = not eng.h_rows and not eng.fold_parts
    for buf in ((eng.hnum, eng.hden) if eng.h_rows else (eng.y, eng.y_den) if store_fold else ()):
        if buf is not None:
            buf.fill_(float('nan'))
    eng.h_step()
    torch.cuda.synchronize()
    if eng.h_rows:
        got['num'] = _gather_rows(eng.hnum, eng)
        got['den'] = None if eng.hden is None else _gather_rows(eng.hden, eng)
    elif store_fold:
        rd = lambda b: b.view(eng.rp_pad, eng.bl_pad)[:RT, :BL].t().double().cpu().numpy()
        got['y'] = rd(eng.y)
        got['yd'] = None if eng.y_den is None else rd(eng.y_den)
    got['new'] = eng.H.cpu().numpy().astype(np.float64)
    ok, fig = CE.check_half_step(got, em, prec, beta, 'h', gemm_rows=_gemm_rows(eng), tol=E.TOL[prec] * case['tol_x'])
    fig['images'] = _h_images(eng, prec)
    return ok and not any(fig['images'].values()), fig


def _flags(eng):
    return dict(implicit=bool(eng.implicit), fold_parts=bool(eng.fold_parts), fused_sums=bool(eng.fused_sums),
                fused_tables=bool(eng.fused_tables), h_rows=bool(eng.h_rows), rows_fused=bool(eng.rows_fused),
                wk_fold=eng.wk_fold if eng.h_rows else None, h_ksplit=eng.h_ksplit if eng.h_rows else None,
                w_ksplit=eng.w_ksplit, h_tail=(eng.h_tail_rows, eng.h_tail_split), ragged=bool(eng.ragged),
                ragged_in_grid=bool(eng.ragged_in_grid), c_rows=eng.c_rows)


@pytest.mark.parametrize('case', CE.conv_cases(), ids=lambda c: c['id'])
def test_conv_half_steps_per_element(dev, monkeypatch, case):
    from torchnmf_amd.nmfd_engine import ConvMU, WideRankMU
    for k in ('WINSTAGE', 'EXPLICIT', 'FOLD_PARTS', 'FUSED_SUMS', 'FUSED_TABLES', 'H_ROWS', 'H_FOLD', 'KSPLIT', 'ROWS_FUSED',
              'TAIL_SPLIT', 'RAGGED', 'RAGGED_IN_GRID', 'NARROW'):
        monkeypatch.delenv('TORCHNMF_AMD_NMFD_' + k, raising=False)
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    prec, beta = case['precision'], case['beta']
    V, W0, H0 = CE.make_problem(case)
    l1, l2 = case['regs']
    if case['wide']:      # NMF.fit above rank 256: V (N, C), W (C, R), H (N, R) through the T = 1 member of the family
        Hu = H0[0].t().contiguous().to(dev)
        wide = WideRankMU(V[0].t().contiguous().to(dev), W0[:, :, 0].contiguous().to(dev), Hu, beta, l1, l2, precision=prec)
        eng = wide.eng
    else:
        eng = ConvMU(V.to(dev), W0.clone().to(dev), H0.clone().to(dev), beta, l1, l2, precision=prec)
    assert eng.precision_name == prec
    # the case is what it says: the plan from the sizes alone, then the engine itself
    flags = _flags(eng)
    p = CE.plan(case, _ncu())
    assert {k: p[k] for k in flags} == flags, (p, flags)
    for cl in case['claims']:
        assert CE.claim_holds(cl, dict(p, **flags), case), (cl, flags)
    torch.cuda.synchronize()
    assert not any(_w_images(eng, prec).values()) and not any(_h_images(eng, prec).values())   # what the first step reads
    Vn = V.numpy()
    res, oks = {}, []
    for it in range(2):
        ok, res[f'w{it}'] = _w_half(eng, Vn, case)
        oks.append(ok)
        ok, res[f'h{it}'] = _h_half(eng, Vn, case)
        oks.append(ok)
    for tag, want in case['staged'].items():
        assert eng.staged.get(tag) == want, (tag, eng.staged)
    # the tables / planes the last H half-step wrote, through one more reconstruction
    Wn, Hn = eng.W.cpu().numpy(), eng.H.cpu().numpy()
    ex = _exact_channels(eng, prec)
    rz = eng.ragged or bool(eng.c_rows)
    rt = CE.ratio(CE.target_w(Vn), CE.operands(Wn, Hn, prec), beta, prec, ex)
    _poison(eng, ('gn', 'gp'), eng.C, eng.B * eng.L, prec, rz)
    eng.recon_ratio_w()
    torch.cuda.synchronize()
    res['last'] = CE.check_ratio(_read_planes(eng, {'gn': 'gn', 'gp': 'gp'}), rt, prec, beta, _gemm_rows(eng))
    oks.append(CE.ratio_ok(res['last']))
    # loss
    got = eng.divergence()
    want, addends = CE.loss(Vn, Wn, Hn, beta, prec, ex)
    loss_tol = CE.LOSS_ULPS * addends / abs(want)
    res['loss'] = dict(got=got, want=want, rel=abs(got - want) / abs(want), tol=loss_tol)
    record('conv_emulated_parity', case=case['id'], tol=E.TOL[prec] * case['tol_x'], flags={k: str(v) for k, v in flags.items()},
           staged={k: v for k, v in eng.staged.items()}, **res)
    print(case['id'], res)
    assert all(oks), res
    assert res['loss']['rel'] <= loss_tol, res['loss']
    if case['zeros']:
        assert float(eng.W[3].abs().max()) == 0.0
        nz = max(1, H0[0, -1].numel() // 3)
        assert float(eng.H[0, -1].reshape(-1)[:nz].abs().max()) == 0.0
