"""CPU tests of tests/mu_emulation.py: the emulation is the algorithm of the oracle once rounding is switched off, its
rounding helpers are bit-exact, and the per-element check of test_gpu_emulated_parity.py fails on seeded kernel faults
that the relative-norm checks of the older tests let through."""
import numpy as np
import pytest
import torch

import mu_emulation as E
from oracle import mu_oracle as O


def _problem(N, C, R, seed, beta):
    g = torch.Generator().manual_seed(seed)
    V = torch.rand(N, C, generator=g, dtype=torch.float64) + (2.0 ** -7 if beta <= 0 else 0.0)
    W = torch.rand(C, R, generator=g, dtype=torch.float64) + 0.05
    H = torch.rand(N, R, generator=g, dtype=torch.float64) + 0.05
    return V, W, H


@pytest.mark.parametrize('beta', [-1.0, 0.0, 0.3, 0.5, 1.0, 1.5, 2.0, 3.0])
@pytest.mark.parametrize('regs', [(0.0, 0.0), (0.1, 0.2)])
def test_unrounded_emulation_is_the_oracle(beta, regs):
    """rounding=False: the emulated W and H half-steps equal mu_oracle's in float64."""
    l1, l2 = regs
    V, W, H = _problem(70, 90, 13, 5, beta)
    gam = O.gamma_of(beta)
    em = E.half_step(V.t().numpy(), W.numpy(), H.numpy(), beta, 'f16x', rounding=False)
    Wn = E.apply(W.numpy(), em['num'], em['den'], beta, gam, l1, l2, kl_den=H.sum(0).numpy())
    Wr = O.nmf_w_step(V, W, H, beta, gam, l1, l2).numpy()
    assert np.abs(Wn - Wr).max() <= 1e-12 * np.abs(Wr).max()
    em = E.half_step(V.numpy(), H.numpy(), Wn, beta, 'f16x', rounding=False)
    Hn = E.apply(H.numpy(), em['num'], em['den'], beta, gam, l1, l2, kl_den=Wn.sum(0))
    Hr = O.nmf_h_step(V, torch.from_numpy(Wr), H, beta, gam, l1, l2).numpy()
    assert np.abs(Hn - Hr).max() <= 1e-12 * np.abs(Hr).max()


def _special_f32():
    g = np.random.default_rng(3)
    rnd = (g.random(4000) * 10.0 ** g.integers(-45, 39, 4000)).astype(np.float32)
    spec = np.array([0.0, 1.0, 65504.0, 65519.0, 65520.0, 7e4, 6e-8, 3e-8, 1e-40, 1.4e-45, 2049.0, 0.333333343,
                     np.float32(2.0 ** -14), np.float32(2.0 ** -24), np.float32(2.0 ** -126)], dtype=np.float32)
    fmax = np.array([0x7f7fffff], dtype=np.uint32).view(np.float32)
    return np.concatenate([spec, fmax, rnd, np.nextafter(rnd, np.float32(np.inf))])


def test_rounding_helpers_are_bit_exact():
    """bf16 RNE and saturating fp16 against torch's conversions and an independent bit formula, f16r against round24."""
    x = _special_f32()
    bits = x.view(np.uint32).astype(np.uint64)
    # bf16: torch, and round-to-nearest-even of the top 16 bits (no NaN among the inputs)
    want = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    got = torch.from_numpy(E.round_bf16(x).astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert np.array_equal(E.round_bf16(x), torch.from_numpy(x).bfloat16().double().numpy())
    # fp16, clamped at 65504 (pack_img)
    h = E.round_f16_sat(x)
    assert np.array_equal(h, torch.from_numpy(x).clamp(max=65504.0).half().double().numpy())
    assert h.max() == 65504.0 and E.round_f16_sat(np.float32(7e4)) == 65504.0 and E.round_f16_sat(-7e4) == -65504.0
    assert E.round_f16_sat(np.float32(2.0 ** -24)) == 2.0 ** -24 and E.round_f16_sat(np.float32(2.0 ** -26)) == 0.0
    # f16r: nearest-even at bit 8, FLT_MAX truncated instead of carried into infinity
    r = E.round_f16r(x)
    assert np.array_equal(r.astype(np.float32).view(np.uint32) & 0xff, np.zeros(len(x), np.uint32))
    assert np.all(np.abs(r - x) <= np.maximum(np.abs(x.astype(np.float64)) * 2.0 ** -16, 2.0 ** -142))
    assert r[15] == float(np.array([0x7f7fff00], np.uint32).view(np.float32)[0])
    assert np.array_equal(E.round24_bits(bits),
                          np.where(((bits + 0x7f + ((bits >> 8) & 1)) & 0x7f800000) == 0x7f800000, bits,
                                   bits + 0x7f + ((bits >> 8) & 1)) & 0xffffff00)
    # the bf16x3 split: hi + lo carries x to 2^-16 (where the lo plane stays a normal number)
    xx = x[(x >= 2.0 ** -100) & (x < 1e38)].astype(np.float64)
    hi, lo = E.split_op(xx, 'bf16')
    assert np.all(np.abs(hi + lo - xx) <= np.abs(xx) * 2.0 ** -16)


def test_every_case_reaches_its_control_flow_on_256_cus():
    """The host mirror places every case of the GPU matrix on its kernel family with the control flow it is named for; at
    least one sp and one sp2 case run a split with zero tiles, the product-heuristic one among them."""
    cases = E.parity_cases(256)
    empty = set()
    for c in cases:
        plan = E.half_step_plan(c['N'], c['C'], c['R'], c['precision'], c['beta'], 256, c['nsplit'], c['block_rows'])
        assert {plan['w']['family'], plan['h']['family']} == {c['family']}, c['id']
        for cl in c['claims']:
            assert any(E.claim_holds(cl, plan[w], c['R']) for w in plan), (c['id'], cl)
        if any(0 in plan[w]['tiles'] for w in plan):
            empty.add(c['family'])
    assert {'sp', 'sp2'} <= empty
    assert E.heuristic_empty_split_cols(256) == 9000
    assert E.half_step_plan(2200, 9000, 256, 'f16', 1.0, 256)['w']['tiles'] == [12, 12, 12, 0]
    assert E.split_tiles(1280, 4, 'sp') == [8, 8, 4, 0] and E.split_tiles(1280, 4, 'pp') == [6, 6, 6, 2]
    for ncu in (80, 104, 228, 304):
        C = E.heuristic_empty_split_cols(ncu)
        assert 0 in E.half_step_plan(2200, C, 256, 'f16', 1.0, ncu)['w']['tiles']


# ---- seeded faults --------------------------------------------------------------------------------------------------
def _case(prefix):
    return next(c for c in E.parity_cases(256) if c['id'].startswith(prefix))


def _h_step(case, **kw):
    """Emulated H half-step of a case from its initial factors (owner H, panel W), fp32 column sums for ki."""
    V, W, H = E.make_problem(case)
    X, A, B = V.numpy(), H.numpy(), W.numpy()
    args = dict(M=A.shape[0], K=B.shape[0], cs_owner=A.sum(0), cs_panel=B.sum(0))
    args.update(kw)
    return X, A, B, args


def _trunc(G, precision):
    """Round toward zero to the operand type (the fault: truncation instead of nearest-even)."""
    if precision in E.F16_OPS:
        h = np.clip(np.asarray(G, np.float32), -E.F16_MAX, E.F16_MAX).astype(np.float16)
        over = np.abs(h.astype(np.float64)) > np.abs(G)
        return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)
    b = np.asarray(G, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return b.view(np.float32).astype(np.float64)


@pytest.mark.parametrize('prefix', ['pp-bf16-b1-257x1100', 'pp-f16-b1-257x1100', 'sp2-f16-b0.5-300x1200', 'fused-f16-b3-300x640'])
def test_seeded_fault_ratio_truncated(prefix):
    c = _case(prefix)
    prec, beta = c['precision'], c['beta']
    X, A, B, args = _h_step(c)
    ok = E.half_step(X, A, B, beta, prec, **args)
    bad = E.half_step(X, A, B, beta, prec, ratio_round=lambda G, split: [_trunc(G, prec)], **args)
    tol = E.TOL[prec]
    assert E.elem_err(bad['num'], ok['num'], ok['num_amb']).max() > tol
    gam = O.gamma_of(beta)
    kl = B.sum(0)
    ref = E.apply(A, ok['num'], ok['den'], beta, gam, kl_den=kl)
    got = E.apply(A, bad['num'], bad['den'], beta, gam, kl_den=kl)
    allow = E.apply_allowance(ref, ok['num'], ok['den'], ok['num_amb'], ok['den_amb'], beta, gam)
    assert E.elem_err(got, ref, allow).max() > tol


def test_seeded_fault_one_owner_row_of_the_ragged_block():
    """One owner row of the ragged last row block off by 1e-3: below the old 6e-4 norm bar, far above the element bar."""
    c = _case('pp-f16-b1-257x1100')
    X, A, B, args = _h_step(c)
    ok = E.half_step(X, A, B, 1.0, 'f16', **args)
    ref = E.apply(A, ok['num'], None, 1.0, 1.0, kl_den=B.sum(0))
    got = ref.copy()
    got[-1] *= 1 + 1e-3
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 6e-4
    assert E.elem_err(got, ref).max() > E.TOL['f16']


def test_seeded_fault_short_last_split_dropped():
    """The short last split of [8, 8, 4, 0] contributes nothing (a wrong ``nt`` for the last non-empty workgroup)."""
    c = _case('sp2-f16-b0.5-300x1200')
    X, A, B, args = _h_step(c)
    plan = E.half_step_plan(c['N'], c['C'], c['R'], 'f16', 0.5, 256, c['nsplit'])['h']
    assert plan['tiles'] == [8, 8, 4, 0]
    k_cut = 16 * E.KBK
    ok = E.half_step(X, A, B, 0.5, 'f16', **args)
    bad = E.half_step(X[:, :k_cut], A, B[:k_cut], 0.5, 'f16', **args)
    assert E.elem_err(bad['num'], ok['num'], ok['num_amb']).max() > E.TOL['f16']
    assert E.elem_err(bad['den'], ok['den'], ok['den_amb']).max() > E.TOL['f16']


@pytest.mark.parametrize('prefix', ['sp2-f16-b0.5-300x1200', 'fused-bf16x3-b0.5-200x330', 'fused-f16-b0.5-384x1100'])
def test_seeded_fault_padded_panel_row_leaks_into_den(prefix):
    """A padded panel row of 1e-3 (instead of 0) at beta = 0.5: its Gp = S^-0.5 is large where S ~ eps."""
    c = _case(prefix)
    X, A, B, args = _h_step(c)
    ok = E.half_step(X, A, B, 0.5, c['precision'], **args)
    Xp = np.concatenate([X, np.zeros((X.shape[0], 1))], axis=1)
    Bp = np.concatenate([B, np.full((1, B.shape[1]), 1e-3)], axis=0)
    bad = E.half_step(Xp, A, Bp, 0.5, c['precision'], **args)
    assert E.elem_err(bad['den'], ok['den'], ok['den_amb']).max() > E.TOL[c['precision']]


@pytest.mark.parametrize('prefix', ['pp-f16-b1-257x1100', 'sp-f16-b1-300x1200', 'sp2-f16-b0-300x1200', 'fused-f16x-b1.5'])
def test_seeded_fault_one_rank_column(prefix):
    """One rank column of the numerator off by 1e-4 relative."""
    c = _case(prefix)
    X, A, B, args = _h_step(c)
    ok = E.half_step(X, A, B, c['beta'], c['precision'], **args)
    bad = ok['num'].copy()
    bad[:, 7] *= 1 + 1e-4
    assert E.elem_err(bad, ok['num'], ok['num_amb']).max() > E.TOL[c['precision']]


# ---- beta == 2 without the reconstruction (family 'xb', tests/test_gpu_gram_emulated_parity.py) ---------------------
@pytest.mark.parametrize('regs', [(0.0, 0.0), (0.1, 0.2)])
def test_unrounded_xb_emulation_is_the_oracle(regs):
    """rounding=False: owner @ (panel^T panel) and X @ panel followed by the apply are the reference's beta == 2 half-steps
    (reconstruction + two backward products) in float64."""
    l1, l2 = regs
    V, W, H = _problem(70, 90, 13, 5, 2.0)
    one = np.ones(13)
    em = E.xb_half_step(V.t().numpy(), W.numpy(), H.numpy(), E.gram_matrix(H.numpy()), 0.0, one, 'f16x', rounding=False)
    Wn = E.apply(W.numpy(), em['num'], em['den'], 2.0, 1.0, l1, l2)
    Wr = O.nmf_w_step(V, W, H, 2.0, 1.0, l1, l2).numpy()
    assert np.abs(Wn - Wr).max() <= 1e-12 * np.abs(Wr).max()
    em = E.xb_half_step(V.numpy(), H.numpy(), Wn, E.gram_matrix(Wn), 0.0, one, 'f16x', rounding=False)
    Hn = E.apply(H.numpy(), em['num'], em['den'], 2.0, 1.0, l1, l2)
    Hr = O.nmf_h_step(V, torch.from_numpy(Wr), H, 2.0, 1.0, l1, l2).numpy()
    assert np.abs(Hn - Hr).max() <= 1e-12 * np.abs(Hr).max()


def test_gram_images_are_bit_exact():
    """gram_images against an independent formulation of gram_finalize_kernel's tail: the exponent from the fp32 bit
    pattern of the row maximum, bf16 by the integer round-to-nearest-even formula, fp16 by numpy's conversion."""
    g = np.random.default_rng(11)
    r_pad = 64
    G = (g.random((r_pad, r_pad)) * 10.0 ** g.integers(-6, 9, (r_pad, 1))).astype(np.float32)
    G[3] = 0.0                                   # zero row (padding): scale 1
    G[4, :] = 1024.0                             # maximum an exact power of two: 0.5 * 2^11 -> scaled maximum 512
    G[5, 7] = np.inf                             # the ``m < 3e38`` guard: ex = 0
    G[6] = np.float32(3.2e38) * g.random(r_pad).astype(np.float32)
    G[6, 0] = np.float32(3.2e38)             # finite, but not below 3e38: ex = 0 as well
    G[7] *= np.float32(1e-30)
    G[8, 1:] = 0.0                               # one entry carries the row
    G[9] = np.float32(65504.0 * 37)
    for f16 in (True, False):
        hi, lo, scale = E.gram_images(G, r_pad, f16)
        m = np.nanmax(np.where(np.isfinite(G), G, np.inf), axis=1).astype(np.float32)
        expo = ((m.view(np.uint32) >> 23) & 0xff).astype(np.int64) - 127        # m = 1.f * 2^expo (normal numbers)
        ok = (m > 0) & (m < np.float32(3.0e38))
        ex = np.where(ok, expo + 1 - 10, 0)
        assert np.array_equal(scale.astype(np.float64), 2.0 ** ex.astype(np.float64))
        assert scale[3] == 1.0 and scale[5] == 1.0 and scale[6] == 1.0 and scale[4] == 2.0
        with np.errstate(over='ignore', invalid='ignore'):
            v = (G.astype(np.float64) * 2.0 ** -ex.astype(np.float64)[:, None]).astype(np.float32)   # exact: a power of two
            fin = np.isfinite(v).all(axis=1) & (np.abs(v) < 6e4).all(axis=1)
            assert fin.sum() >= r_pad - 2
            if f16:
                h = v.astype(np.float16)
                l = (v - h.astype(np.float32)).astype(np.float16)
                want_hi, want_lo = h.view(np.uint16), l.view(np.uint16)
            else:
                def bf(x):
                    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
                    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
                want_hi = bf(v)
                hv = (want_hi.astype(np.uint32) << 16).view(np.float32)
                want_lo = bf(v - hv)
        assert np.array_equal(hi[fin], want_hi[fin]) and np.array_equal(lo[fin], want_lo[fin])
        hv, lv = E.image_values(hi, f16), E.image_values(lo, f16)
        assert 512.0 <= hv[4].max() < 1024.0 and all(512.0 <= hv[r].max() <= 1024.0 for r in (0, 1, 2, 7, 8, 9))
        with np.errstate(invalid='ignore'):
            rec = (hv + lv) * scale.astype(np.float64)[:, None]
        sel = fin & ok
        rel = 2.0 ** (-21 if f16 else -15)       # hi + lo: 22 (16) significant bits, less one where lo is subnormal / tiny
        assert np.all(np.abs(rec[sel] - G[sel]) <= rel * m[sel, None].astype(np.float64))
        assert not hv[3].any() and not lv[3].any()


def test_every_xb_case_reaches_its_control_flow_on_256_cus():
    """The Gram-path matrix: every case runs family 'xb' with the control flow it is named for, and every claim of the family
    is reached at NSTAGE 4 (bf16, f16) and at NSTAGE 3 (f16x) wherever that instance can reach it."""
    assert E.xb_nstage('f16x') == 3 and E.xb_nstage('f16') == E.xb_nstage('bf16') == 4
    reached = {cl: set() for cl in E.XB_CLAIMS}
    ids = set()
    for c in E.xb_cases(256):
        assert c['id'] not in ids and max(c['N'], c['C']) <= 2400
        ids.add(c['id'])
        assert c['precision'] != 'f16x' or E.pad_rank(c['R']) <= 128
        plan = E.half_step_plan(c['N'], c['C'], c['R'], c['precision'], 2.0, 256, c['nsplit'], None, gram=True)
        assert {plan['w']['family'], plan['h']['family']} == {'xb'}, c['id']
        for cl in c['claims']:
            assert any(E.claim_holds(cl, plan[w], c['R']) for w in plan), (c['id'], cl)
        for cl in reached:
            if any(E.claim_holds(cl, plan[w], c['R']) for w in plan):
                reached[cl].add(E.xb_nstage(c['precision']))
    for cl, want in E.XB_CLAIMS.items():
        assert reached[cl] >= set(want), (cl, reached[cl])
    assert sum(1 for c in E.xb_cases(256) if c['regs'][0] > 0) * 3 >= len(E.xb_cases(256)) - 2
    # the split arithmetic of the shapes the matrix is built on
    assert E.split_tiles(2304, 8, 'xb') == [5] * 7 + [1] and E.split_tiles(2048, 7, 'xb') == [5] * 6 + [2]
    assert E.split_tiles(1792, 6, 'xb') == [5] * 5 + [3] and E.split_tiles(2304, 7, 'xb') == [6] * 6 + [0]
    assert E.split_tiles(1280, 3, 'xb') == [7, 7, 6] and E.split_tiles(2304, 9, 'xb') == [4] * 9
    # the Gram launches: chunks, tiles per chunk, and the chain length written into every case
    for c in E.gram_cases():
        assert E.gram_plan(c['rows'], E.pad_rank(c['rank']))['n_seq'] == c['n_seq'], c['id']
    p = E.gram_plan(16500, 128)
    assert (p['ktiles'], p['nchunk'], p['per']) == (260, 65, 4)
    p = E.gram_plan(66000, 64)
    assert (p['ktiles'], p['nchunk'], p['per']) == (1032, 256, 5) and sorted(set(p['tiles'])) == [0, 2, 5] and p['tiles'].count(0) == 49
    p = E.gram_plan(82000, 128)
    assert (p['ktiles'], p['nchunk'], p['per']) == (1284, 256, 6)


# Seeded faults of the Gram path.  Each is applied to the emulation's output and must fail the check the GPU test asserts
# (E.elem_err against E.TOL for numerator / denominator / master, E.gram_excess <= 1 for the fp32 matrix); ``old`` says
# whether the bars of the older tests would have let it through (whole-factor relative norm < 1e-4, 5e-3 in bf16:
# test_half_steps_beta2_without_reconstruction; Gram matrix norm < 2e-6: test_gram_panel_matches_fp32).
OLD_BAR = {'f16': 1e-4, 'f16x': 1e-4, 'bf16': 5e-3}


def _xb_state(N, C, R, prec, seed=3):
    """H half-step (owner H [N, R], panel W [C, R]) as the GPU would hold it: images, Gram matrix in fp32, its images."""
    g = torch.Generator().manual_seed(seed)
    V = torch.rand(N, C, generator=g)
    W = (torch.randn(C, R, generator=g).abs() + 0.05) * E.xb_column_scales(R)
    H = (torch.randn(N, R, generator=g).abs() + 0.05) * E.xb_column_scales(R)
    r_pad = E.pad_rank(R)
    A = np.zeros((N, r_pad))
    A[:, :R] = E.round_op(H.numpy(), prec)
    B = np.zeros((E.pad_rows(C), r_pad))
    B[:C, :R] = E.round_op(W.numpy(), prec)
    G32 = E.gram_matrix(B).astype(np.float32)
    f16 = prec in E.F16_OPS
    hi, lo, scale = E.gram_images(G32, r_pad, f16)
    return dict(X=V.numpy(), A=A, B=B, W=W.numpy(), H=H.numpy(), G32=G32, hi=E.image_values(hi, f16), lo=E.image_values(lo, f16),
                scale=scale.astype(np.float64), prec=prec, R=R, C=C, r_pad=r_pad)


def _xb_em(s, **kw):
    a = dict(X=s['X'], A=s['A'], B=s['B'][:s['C']], hi=s['hi'], lo=s['lo'], scale=s['scale'])
    a.update(kw)
    return E.xb_half_step(a['X'], a['A'], a['B'], a['hi'], a['lo'], a['scale'], s['prec'])


def _xb_verdict(s, ok, bad, name, expect_old_pass):
    """new check: per element, numerator / denominator / master against E.TOL; old bar: relative norm of the new factor."""
    R, tol = s['R'], E.TOL[s['prec']]
    theta = s['H'].astype(np.float64)
    ref = E.apply(theta, ok['num'][:, :R], ok['den'][:, :R], 2.0, 1.0)
    got = E.apply(theta, bad['num'][:, :R], bad['den'][:, :R], 2.0, 1.0)
    new = max(E.elem_err(bad['num'][:, :R], ok['num'][:, :R]).max(), E.elem_err(bad['den'][:, :R], ok['den'][:, :R]).max())
    master = E.elem_err(got, ref).max()
    finite = np.isfinite(got).all()
    old = float(np.linalg.norm(got - ref) / np.linalg.norm(ref)) if finite else float('inf')
    old_pass = old < OLD_BAR[s['prec']]
    print(f'fault {name}: fails the new check (slab {new:.2e}, master {master:.2e} > {tol:.1e}); '
          f'{"passes" if old_pass else "fails"} the old norm bar ({old:.2e} vs {OLD_BAR[s["prec"]]:.0e})')
    assert new > tol and master > tol, (name, new, master)
    assert old_pass == expect_old_pass, (name, old)


@pytest.mark.parametrize('prec', ['f16', 'bf16'])
def test_seeded_fault_gram_lo_plane_dropped(prec):
    """(a) the lo plane of the Gram image lost: a 2^-12 (fp16) / 2^-9 (bf16) effect on the matrix, below the old norm bar."""
    s = _xb_state(300, 1100, 100, prec)
    _xb_verdict(s, _xb_em(s), _xb_em(s, lo=np.zeros_like(s['lo'])), f'(a) lo plane dropped, {prec}', True)


@pytest.mark.parametrize('kind', ['not multiplied back', 'neighbouring row'])
def test_seeded_fault_gram_row_scale(kind):
    """(b) one row's scale not multiplied back / taken from the neighbouring row: one denominator column."""
    s = _xb_state(300, 1100, 100, 'f16')
    scale = s['scale'].copy()
    r = next(i for i in range(s['R'] - 1) if scale[i] != scale[i + 1]) if kind == 'neighbouring row' else 17
    scale[r] = scale[r + 1] if kind == 'neighbouring row' else 1.0
    assert scale[r] != s['scale'][r]
    _xb_verdict(s, _xb_em(s), _xb_em(s, scale=scale), f'(b) scale of row {r} {kind}', False)


def _gram_verdict(name, G32, ref, n_seq, expect_old_pass):
    ex = E.gram_excess(G32, ref, n_seq)
    old = float(np.linalg.norm(G32.astype(np.float64) - ref) / np.linalg.norm(ref))
    print(f'fault {name}: fails the new check ({ex:.2e} x the n_seq = {n_seq} bound); '
          f'{"passes" if old < 2e-6 else "fails"} the old Gram norm bar ({old:.2e} vs 2e-06)')
    assert ex > 1.0, (name, ex)
    assert (old < 2e-6) == expect_old_pass, (name, old)


def _gram_case(cid):
    c = next(c for c in E.gram_cases() if c['id'] == cid)
    rows, rank = c['rows'], c['rank']
    r_pad = E.pad_rank(rank)
    B = np.zeros((E.pad_rows(rows), r_pad))
    B[:rows, :rank] = E.round_op(E.gram_problem(c).numpy(), c['precision'])
    return c, B, E.gram_plan(rows, r_pad)


def test_seeded_fault_last_short_gram_chunk_dropped():
    """(c) the 2-tile chunk behind 206 chunks of 5 contributes nothing: 80 of 66000 rows."""
    c, B, plan = _gram_case('66000x40-f16')
    ref = E.gram_matrix(B)
    assert E.gram_excess(ref.astype(np.float32), ref, c['n_seq']) <= 1.0      # the correctly rounded matrix passes
    last = max(i for i, t in enumerate(plan['tiles']) if t)
    assert plan['tiles'][last] == 2
    cut = last * plan['per'] * E.KBK
    _gram_verdict('(c) last, short Gram chunk dropped', E.gram_matrix(B[:cut]).astype(np.float32), ref, c['n_seq'], False)


def test_seeded_fault_padded_panel_row_in_the_gram():
    """(d) one padded row of the image holds a stale copy of a live row: in the Gram matrix, and in the denominator."""
    c, B, plan = _gram_case('300x24-f16')
    ref = E.gram_matrix(B)
    Bp = B.copy()
    Bp[c['rows'] + 5] = B[0]
    _gram_verdict('(d) padded panel row non-zero (Gram matrix)', E.gram_matrix(Bp).astype(np.float32), ref, c['n_seq'], False)
    s = _xb_state(300, 1100, 100, 'f16')
    Bp = s['B'].copy()
    Bp[s['C'] + 5] = s['B'][0]
    hi, lo, scale = E.gram_images(E.gram_matrix(Bp).astype(np.float32), s['r_pad'], True)
    bad = _xb_em(s, hi=E.image_values(hi, True), lo=E.image_values(lo, True), scale=scale.astype(np.float64))
    _xb_verdict(s, _xb_em(s), bad, '(d) padded panel row non-zero (denominator)', False)


def test_seeded_fault_denominator_tile_unwritten():
    """(e) one 32-column rank tile of the ONE denominator slab left unwritten: the slab's NaN poison stays.  (The variant
    "the same tile written by two workgroups" is left out: both compute the same product from the same operands in the
    same order, so the slab holds the right bits either way -- a waste of time, not a wrong value, and invisible in one slab.)"""
    s = _xb_state(300, 1100, 100, 'f16')
    ok = _xb_em(s)
    bad = dict(ok, den=ok['den'].copy())
    bad['den'][128:256, 64:96] = np.nan
    _xb_verdict(s, ok, bad, '(e) rank tile 2 of row block 1 unwritten', False)


def test_seeded_fault_last_tile_of_a_rem1_split_dropped():
    """(f) the last tile of a split with nt % NSTAGE == 1 (the ring's one-tile remainder) missing from the numerator."""
    c = next(c for c in E.xb_cases(256) if c['id'].startswith('xb-f16-130x2300r64-ns8'))
    tiles = E.half_step_plan(c['N'], c['C'], c['R'], 'f16', 2.0, 256, c['nsplit'], None, gram=True)['h']['tiles']
    assert tiles == [5] * 7 + [1] and tiles[0] % E.xb_nstage('f16') == 1
    s = _xb_state(130, 2300, 64, 'f16')
    X = s['X'].copy()
    X[:, 4 * E.KBK:5 * E.KBK] = 0.0               # the fifth tile of split 0
    _xb_verdict(s, _xb_em(s), dict(_xb_em(s), num=_xb_em(s, X=X)['num']), '(f) tile 4 of split 0 dropped', False)


@pytest.mark.parametrize('prec', ['f16', 'bf16'])
def test_seeded_fault_gram_from_the_fp32_master(prec):
    """(g) the Gram matrix formed from the fp32 master instead of the 16-bit image: caught in the fp32 matrix itself (where
    the old 2e-6 norm bar is blind to it only for very long panels) and in the denominator; far below the old factor bar."""
    c, B, plan = _gram_case('700x64-' + prec)
    F = np.zeros_like(B)
    F[:c['rows'], :c['rank']] = E.gram_problem(c).numpy()
    _gram_verdict(f'(g) Gram from the fp32 master, {prec} (Gram matrix)', E.gram_matrix(F).astype(np.float32), E.gram_matrix(B),
                  c['n_seq'], False)
    s = _xb_state(1100, 130, 64, prec)
    F = np.zeros_like(s['B'])
    F[:s['C'], :s['R']] = s['W']
    f16 = prec == 'f16'
    hi, lo, scale = E.gram_images(E.gram_matrix(F).astype(np.float32), s['r_pad'], f16)
    bad = _xb_em(s, hi=E.image_values(hi, f16), lo=E.image_values(lo, f16), scale=scale.astype(np.float64))
    _xb_verdict(s, _xb_em(s), bad, f'(g) Gram from the fp32 master, {prec} (denominator)', True)


def test_seeded_fault_owner_fragments_of_the_neighbouring_wave():
    """(h) the denominator of one wave's 32 rows formed from the owner fragments of the wave next to it."""
    s = _xb_state(300, 1100, 100, 'f16')
    ok = _xb_em(s)
    bad = dict(ok, den=ok['den'].copy())
    bad['den'][32:64] = ok['den'][0:32]
    _xb_verdict(s, ok, bad, '(h) owner fragments of wave 0 in wave 1', False)


# ---- the dense loss pass: float64 model per partial, its bound, seeded faults ------------------------------------------
def _loss_case(prefix):
    return next(c for c in E.loss_cases(256) if c['id'].startswith(prefix))


_LOSS_MEMO = {}


def _loss_model(case, **kw):
    """(plan, partials) of a loss case from its initial factors, images rounded on the host (memoised: the cap test and the
    seeded-fault tests share the unfaulted models)."""
    key = (case['id'], tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _LOSS_MEMO:
        prec, beta = case['precision'], case['beta']
        plan = E.loss_plan(case['N'], case['C'], case['R'], prec, beta, 256, case['nsplit'], case['block_rows'], case['gram'])
        V, W0, H0 = E.loss_problem(case)
        lp = E.loss_partials(V.numpy(), E.host_images(H0.numpy(), prec), E.host_images(W0.numpy(), prec), beta, prec, plan, **kw)
        _LOSS_MEMO[key] = (plan, lp)
    return _LOSS_MEMO[key]


@pytest.mark.parametrize('block_rows', [None, 128])
@pytest.mark.parametrize('beta', [-1.0, 0.0, 0.3, 0.5, 1.0, 1.5, 2.0, 3.0])
def test_unrounded_loss_partials_sum_to_the_oracle(beta, block_rows):
    """rounding=False: the partials are a partition of beta_div(H W^T, V) -- every valid element once, no padded one -- on a
    ragged shape (rows, columns and rank off every tile) with 30 % exact zeros in the target, for every beta branch, on the
    ping-pong kernel's 256-row blocks (beta == 1) and on 128-row blocks."""
    N, C, R = 150, 330, 7
    g = torch.Generator().manual_seed(11)
    V = torch.rand(N, C, generator=g, dtype=torch.float64)
    V = torch.where(torch.rand(N, C, generator=g) < 0.3, torch.zeros((), dtype=torch.float64), V)
    W = torch.rand(C, R, generator=g, dtype=torch.float64) + 0.05
    H = torch.rand(N, R, generator=g, dtype=torch.float64) + 0.05
    plan = E.loss_plan(N, C, R, 'f16', beta, 256, 2, block_rows)
    assert plan['family'] == ('pp' if beta == 1.0 and block_rows is None else 'fused') and plan['nsplit'] == 2
    lp = E.loss_partials(V.numpy(), (H.numpy(), None), (W.numpy(), None), beta, 'f16', plan, rounding=False)
    want = float(O.beta_div(O.nmf_reconstruct(H, W), V, float(np.float32(beta))))     # (the library takes beta as a float: 0.3f)
    assert lp['ref'].shape == (plan['nparts'],)
    assert float(lp['ref'].sum()) == pytest.approx(want, rel=1e-10)


def test_loss_plan_walks_the_loss_modes_tile_list():
    """The loss runs on step_h's nsplit with ITS OWN tiles per split: rounded to even on the ping-pong kernel, not rounded on the
    four-wave kernel -- whatever the MU family rounds to."""
    sp = E.loss_plan(300, 1200, 256, 'f16', 1.0, 256, 4)
    assert (sp['mu_family'], sp['family'], sp['mu_tiles'], sp['tiles']) == ('sp', 'fused', [8, 8, 4, 0], [5, 5, 5, 5])
    sp2 = E.loss_plan(300, 1200, 100, 'f16', 0.5, 256, 4)
    assert (sp2['mu_family'], sp2['family'], sp2['mu_tiles'], sp2['tiles']) == ('sp2', 'fused', [8, 8, 4, 0], [5, 5, 5, 5])
    one = E.loss_plan(300, 200, 200, 'f16', 1.0, 256)
    assert (one['mu_family'], one['family'], one['mu_tiles'], one['tiles']) == ('sp', 'fused', [4], [4])
    xb = E.loss_plan(384, 700, 64, 'f16', 2.0, 256, 3, gram=True)
    assert (xb['mu_family'], xb['family'], xb['mu_tiles'], xb['tiles']) == ('xb', 'fused', [4, 4, 4], [4, 4, 4])
    pp = E.loss_plan(257, 1100, 33, 'f16', 1.0, 256, 4)
    assert (pp['family'], pp['block_rows'], pp['tiles'], pp['nparts'], pp['tree']) == ('pp', 256, [6, 6, 6, 2], 8, 9)
    assert E.loss_plan(257, 1700, 33, 'f16', 1.0, 256, 6)['tiles'] == [6, 6, 6, 6, 4, 0]
    four = E.loss_plan(100, 2304, 24, 'bf16', 0.5, 256, 7)
    assert (four['family'], four['tiles'], four['nparts'], four['tree']) == ('fused', [6] * 6 + [0], 14, 8)
    assert E.s_chain(32, 'f16') == 19 and E.s_chain(128, 'bf16x3') == 41 and E.s_chain(256, 'f16') == 33
    ids = [c['id'] for c in E.loss_cases(256)]
    assert len(ids) == len(set(ids))


def test_every_loss_case_bound_is_at_most_1e5_of_its_terms():
    """Non-vacuity of the bound: for every case of the GPU matrix and every partial that owns a valid element, the derived bound
    is at most LOSS_CAP = 1e-5 of the partial's sum |terms| (images rounded on the host).  A cap, not a measurement: a case
    that exceeds it gets a shorter contraction (mu_emulation.LOSS_SHAPES), the cap stays."""
    assert E.LOSS_CAP == 1e-5
    for c in E.loss_cases(256):
        plan, lp = _loss_model(c)
        live = lp['abs_terms'] > 0
        assert live.any(), c['id']
        frac = lp['bound'][live] / lp['abs_terms'][live]
        assert frac.max() <= E.LOSS_CAP, (c['id'], float(frac.max()))
        assert (lp['bound'][~live] == 0).all() and (lp['ref'][~live] == 0).all(), c['id']
        assert lp['n_chain'].max() == 32 * max(plan['tiles'])


def _fp32_loss_partials(case):
    """The loss pass executed in numpy fp32 in the kernel's order: loss_elem as written (np.log2 / np.exp2 on float32 are
    within an ulp), one accumulator per lane over (tile, tt, d, half), six butterfly levels, the waves' tree.  S is the
    float64 reconstruction rounded to fp32 once."""
    prec, beta = case['precision'], case['beta']
    plan = E.loss_plan(case['N'], case['C'], case['R'], prec, beta, 256, case['nsplit'], case['block_rows'], case['gram'])
    V, W0, H0 = E.loss_problem(case)
    f = np.float32
    kind = E.beta_kind(beta)
    S = E._recon(E.host_images(H0.numpy(), prec), E.host_images(W0.numpy(), prec), plan['m_pad'], plan['k_pad'],
                 0.0 if kind == 'euc' else E.EPS).astype(f)
    x = E._padded(E.stored_target(V.numpy(), prec), plan['m_pad'], plan['k_pad']).astype(f)
    eps, ln2, b = f(E.EPS), f(0.6931471805599453), f(beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == 'euc':
            d = S - x
            l = f(0.5) * d * d
        elif kind == 'kl':
            l = x * ((np.log2(x + eps) - np.log2(S)) * ln2) - x + (S - eps)
        elif kind == 'is':
            xe = x + eps
            l = xe * (f(1.0) / S) - (np.log2(xe) - np.log2(S)) * ln2 - f(1.0)
        else:
            xb = x + eps if beta < 0 else x
            t1 = np.where(xb > 0, np.exp2(b * np.log2(np.where(xb > 0, xb, f(1.0)))), f(0.0)).astype(f)
            sb1 = np.exp2((b - f(1.0)) * np.log2(S)).astype(f)
            l = (t1 + (b - f(1.0)) * (sb1 * S) - b * xb * sb1) / (b * (b - f(1.0)))
    assert l.dtype == np.float32
    ok = (np.arange(plan['m_pad'])[:, None] < plan['M']) & (np.arange(plan['k_pad'])[None, :] < plan['K'])
    l = np.where(ok, l, f(0.0))
    br, ns, tps = plan['block_rows'], plan['nsplit'], plan['tps']
    out = np.zeros(plan['nparts'], dtype=f)
    for mb in range(plan['m_pad'] // br):
        for ks in range(ns):
            nt = plan['tiles'][ks]
            if nt == 0:
                continue
            blk = l[mb * br:(mb + 1) * br, ks * tps * 64:(ks * tps + nt) * 64].reshape(br // 32, 32, nt, 2, 32)   # wave, j, tile, hl, slot
            acc = np.zeros((br // 32, 32, 2), dtype=f)
            for t in range(nt):
                for sl in range(32):
                    acc = acc + blk[:, :, t, :, sl]
            lanes = acc.transpose(0, 2, 1).reshape(br // 32, 64)          # lane = 32 hl + j
            for o in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[:, np.arange(64) ^ o]
            red = lanes[:, 0]
            while len(red) > 1:
                red = red[0::2] + red[1::2]
            out[mb * ns + ks] = red[0]
    return plan, out


@pytest.mark.parametrize('prefix', ['pp-f16-b1-257x1100', 'fused-bf16x3-b0.5-200x330', 'fused-f16-b2-300x500', 'fused-bf16-b0-384x1100',
                                    'fused-f16-b3-', 'fused-bf16-b-1-200x330', 'pp-f16r-b1-257x1100r33-ns4-fitted'])
def test_fp32_execution_of_the_loss_stays_inside_the_bound(prefix):
    """The bound holds for an fp32 execution in the kernel's order (so it is not too tight to be met), and that execution is
    not the float64 value (so the comparison is not trivially zero)."""
    c = _loss_case(prefix)
    plan, got = _fp32_loss_partials(c)
    _, lp = _loss_model(c)
    ex = E.partial_excess(got, lp['ref'], lp['bound'])
    assert ex.max() <= 1.0, (c['id'], float(ex.max()))
    assert ex.max() > 0.0


@pytest.mark.parametrize('beta', [0.5, 3.0, -1.0])
def test_seeded_fault_loss_column_mask_dropped(beta):
    """(a) ``k0 < a.K`` dropped on C % 64 != 0: every padded column of a valid row adds loss_elem(s = eps, x = 0).  At beta = 0.5
    that is eps^0.5 / 0.5 = 6.9e-4 per element and the checker flags it by more than 10x where the padding is a sizeable share of
    the tiles (200 x 330: 182 padded columns per row in split 1; the six of 520 x 250 move a partial by 0.19 of its bound).  At beta = 3 it is eps^3 / 3 =
    5.6e-22 per element, below 1e-15 of a partial; at beta = -1 the padded element becomes x = eps against s = eps, a
    divergence of EXACTLY zero (all three terms are powers of two).  At those two betas a kernel without the mask returns the
    same fp32 words as one with it: no check of the output can tell them apart, and the sum is right either way.  The test pins
    both halves: caught where the fault changes the value, provably harmless where it does not."""
    c = _loss_case({0.5: 'fused-bf16x3-b0.5-200x330r24', 3.0: 'fused-bf16-b3-200x250r24', -1.0: 'fused-bf16-b-1-200x330r24'}[beta])
    plan, ok = _loss_model(c)
    _, bad = _loss_model(c, col_mask=False)
    shift = np.abs(bad['ref'] - ok['ref'])
    pad_cols = plan['k_pad'] - plan['K']
    assert pad_cols > 0
    if beta == 0.5:
        ex = E.partial_excess(bad['ref'], ok['ref'], ok['bound'])
        assert plan['tiles'] == [4, 4] and (shift[0::2] == 0).all()             # split 0 holds no padded column, split 1 holds 182
        assert (ex[1::2] >= 10.0).all(), ex
        assert shift.sum() == pytest.approx(plan['M'] * pad_cols * np.sqrt(E.EPS) / 0.5, rel=1e-9)
    elif beta == 3.0:
        assert shift.sum() == pytest.approx(plan['M'] * pad_cols * E.EPS ** 3 / 3.0, rel=1e-6)
        live = ok['abs_terms'] > 0
        assert (shift[live] <= 2.0 ** -40 * np.abs(ok['ref'][live])).all()          # far below half an ulp of the fp32 partial
    else:
        assert (shift == 0).all()


def test_seeded_fault_loss_last_valid_row_dropped():
    """(b) ``m0 < a.M`` off by one: row M - 1 is missing from the last row block's partials."""
    for prefix in ('pp-f16-b1-257x1100r33-ns4', 'fused-bf16x3-b0.5-200x330'):
        c = _loss_case(prefix)
        plan, ok = _loss_model(c)
        _, bad = _loss_model(c, m_valid=plan['M'] - 1)
        ex = E.partial_excess(bad['ref'], ok['ref'], ok['bound'])
        mb = (plan['M'] - 1) // plan['block_rows']
        own = [mb * plan['nsplit'] + ks for ks in range(plan['nsplit']) if ok['abs_terms'][mb * plan['nsplit'] + ks] > 0]
        assert own and (ex[own] >= 10.0).all(), (prefix, ex)


def test_seeded_faults_loss_partials_swapped_or_a_tile_skipped_pass_the_total():
    """(c) two partials swapped and (d) the last tile of one split skipped: the per-partial check flags both by more than 10x,
    the total at rel = 2e-4 -- what test_gpu_parity.py holds the loss to -- sees neither.  257 x 1100 on 256-row blocks,
    tiles [6, 6, 6, 2]: the second row block holds one row, the last tile of split 2 twelve valid columns."""
    c = _loss_case('pp-f16-b1-257x1100r33-ns4')
    plan, ok = _loss_model(c)
    assert plan['tiles'] == [6, 6, 6, 2]
    total = ok['ref'].sum()
    # (c)
    got = ok['ref'].copy()
    got[[0, 1]] = got[[1, 0]]
    ex = E.partial_excess(got, ok['ref'], ok['bound'])
    assert ex[0] >= 10.0 and ex[1] >= 10.0
    assert got.sum() == pytest.approx(total, rel=2e-4)
    # (d): workgroup (row block 1, split 2) walks five of its six tiles
    _, bad = _loss_model(c, tiles=[6, 6, 5, 2])
    ex = E.partial_excess(bad['ref'], ok['ref'], ok['bound'])
    assert ex[4 + 2] >= 10.0 and ex[2] >= 10.0
    got = ok['ref'].copy()
    got[4 + 2] = bad['ref'][4 + 2]                      # the fault in ONE workgroup
    assert E.partial_excess(got, ok['ref'], ok['bound'])[4 + 2] >= 10.0
    assert got.sum() == pytest.approx(total, rel=2e-4)


def test_seeded_fault_loss_empty_split_keeps_its_poison():
    """(e) an empty split (or one of padding only) that does not write its slot: the slot must hold exactly 0.0."""
    for prefix, empty in (('pp-f16-b1-257x1700r33-ns6', 5), ('fused-bf16-b0.5-100x2304r24-ns7', 6)):
        c = _loss_case(prefix)
        plan, ok = _loss_model(c)
        assert plan['tiles'][empty] == 0 and ok['bound'][empty] == 0
        for poison in (float('nan'), 1e-30, -0.0 + 1e-45):
            got = ok['ref'].copy()
            got[empty] = poison
            assert E.partial_excess(got, ok['ref'], ok['bound'])[empty] >= 10.0
        assert E.partial_excess(ok['ref'], ok['ref'], ok['bound']).max() == 0.0
    # a split of padding only ([6, 6, 6, 2]: tiles 18, 19 lie beyond column 1100) and a row block of padding only
    plan, ok = _loss_model(_loss_case('pp-f16-b1-257x1100r33-ns4'))
    assert ok['bound'][3] == 0 and ok['bound'][7] == 0 and ok['n_chain'][3] == 64
    plan, ok = _loss_model(_loss_case('fused-bf16-b0.5-100x2304r24-ns7'))
    assert (ok['bound'][7:] == 0).all() and (ok['bound'][:6] > 0).all()


def test_seeded_fault_loss_eps_dropped_from_the_log():
    """(f) log(x) for log(x + eps): 0 * log2(0) is NaN in every partial that owns a zero of the target."""
    c = _loss_case('pp-f16-b1-300x1000r64-ns2-zeros')
    plan, ok = _loss_model(c)
    _, bad = _loss_model(c, eps_in_log=False)
    ex = E.partial_excess(bad['ref'], ok['ref'], ok['bound'])
    live = ok['abs_terms'] > 0
    assert live.sum() == 4 and (ex[live] >= 10.0).all()
    # ... and on a target without zeros the dropped eps is still seen: x ln(x + eps) - x ln x ~ eps per element
    c = _loss_case('pp-f16-b1-257x1100r33-ns4')
    _, ok = _loss_model(c)
    _, bad = _loss_model(c, eps_in_log=False)
    assert np.isfinite(bad['ref']).all()


def _riding_model(case, **kw):
    prec = case['precision']
    plan = E.riding_plan(case['N'], case['C'], case['R'], prec, 256, case['nsplit'])
    V, W0, H0 = E.riding_problem(case)
    return plan, V, E.riding_total(V.numpy(), E.host_images(W0.numpy(), prec), E.host_images(H0.numpy(), prec), prec, plan, **kw)


@pytest.mark.parametrize('case', E.RIDING_CASES, ids=lambda c: c['id'])
def test_riding_model_is_the_kl_divergence(case):
    """The value assembled from the pairs the way riding_finish_kernel does is the float64 KL divergence of the fp32 target
    within the bound (the stored target's rounding is the only difference in exact arithmetic), and the bound is small
    against the terms."""
    plan, V, rt = _riding_model(case)
    assert abs(rt['kernel_value'] - rt['ref']) <= rt['bound']
    H0, W0 = E.riding_problem(case)[2], E.riding_problem(case)[1]
    want = float(O.beta_div(O.nmf_reconstruct(torch.from_numpy(E.host_images(H0.numpy(), case['precision'])[0]),
                                              torch.from_numpy(E.host_images(W0.numpy(), case['precision'])[0])), V.double(), 1.0))
    assert rt['ref'] == pytest.approx(want, rel=1e-10)
    S = E._recon((E.host_images(W0.numpy(), case['precision'])[0], None), (E.host_images(H0.numpy(), case['precision'])[0], None),
                 plan['m_pad'], plan['k_pad'], E.EPS)[:plan['M'], :plan['K']]
    x = V.double().numpy().T
    terms = (np.abs(x * np.log(x + E.EPS)) + np.abs(x * np.log(S)) + np.abs(x) + np.abs(S)).sum()
    assert rt['bound'] <= 2 * E.LOSS_CAP * terms, (rt['bound'] / terms)


def test_seeded_fault_riding_n_all_counts_valid_elements_only():
    """(g) the device subtracts n_all * eps for EVERY processed element (each padded one contributed exactly eps to sum s); with
    the valid count instead the loss is too large by (n_all - M K) eps.  1 x 300 rank 1: 131 072 processed, 300 valid."""
    case = next(c for c in E.RIDING_CASES if c['id'].startswith('f16-1x300'))
    plan, V, ok = _riding_model(case)
    assert plan['n_all'] == 512 * 256 and plan['tiles'] == [4]
    _, _, bad = _riding_model(case, n_all=300)
    assert abs(ok['kernel_value'] - ok['ref']) <= ok['bound']
    assert abs(bad['kernel_value'] - ok['ref']) >= 10.0 * ok['bound']
    assert bad['kernel_value'] - ok['kernel_value'] == pytest.approx((plan['n_all'] - 300) * E.EPS, rel=1e-6)


def test_beta_div_bound_is_the_oracle_value():
    g = torch.Generator().manual_seed(5)
    x, y = torch.rand(700, generator=g), torch.rand(700, generator=g)
    y = torch.where(torch.rand(700, generator=g) < 0.3, torch.zeros(()), y)
    for beta in (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0):
        ref, bound = E.beta_div_bound(x.numpy(), y.numpy(), beta)
        assert ref == pytest.approx(float(O.beta_div(x.double(), y.double(), beta)), rel=1e-9)
        assert 0 < bound <= 1e-5 * float(E.loss_abs_terms(x.double().numpy() + (0 if beta == 2 else E.EPS), y.double().numpy(), beta).sum())
