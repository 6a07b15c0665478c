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
