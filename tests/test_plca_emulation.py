"""tests/plca_emulation.py on the CPU: agreement with the float64 oracle, seeded faults, host mirrors.

1. With rounding off (the prior constant kept in double, u = 2^-53) ``plca_emulation.em_step`` fed with the oracle's own
   products equals ``oracle.mu_oracle.plca_em_step`` in float64, on dense and 1-D / 2-D / 3-D shift-invariant problems, for
   all seven trainable combinations, with and without priors.  Both sides run the same float64 operations -- two multiplies,
   a divide, an add, sums of n terms in some order -- so each is within the emulation's own propagated bound at u = 2^-53
   with chain length n (any order) of the exact result: the allowed difference is twice that bound, element by element.
2. Seeded faults: eight wrong kernels written in numpy.  Each must leave the derived bound of a named case of the GPU
   test (same shapes, same chain lengths) by a factor of at least ``CLEAR``.
3. The host mirrors against the library's static queries and the launch arithmetic of the kernels.
"""
import numpy as np
import pytest
import torch

import plca_emulation as P
from oracle import mu_oracle as O

CLEAR = 4.0


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


PROBLEMS = [  # W shape, H shape
    ((13, 4), (9, 4)),
    ((6, 3, 4), (2, 3, 11)),
    ((3, 2, 2, 3), (2, 2, 5, 4)),
    ((2, 2, 2, 2, 2), (1, 2, 3, 2, 4)),
]


@pytest.mark.parametrize('wshape,hshape', PROBLEMS, ids=['dense', 'siplca', 'siplca2', 'siplca3'])
@pytest.mark.parametrize('alphas', P.PRIORS + [(0.99, 1.0, 1.03)], ids=str)
def test_em_step_without_rounding_is_the_oracle(wshape, hshape, alphas):
    g = np.random.default_rng(len(wshape) * 100 + int(alphas[0] * 1000))
    W, H = g.random(wshape) + 0.01, g.random(hshape) + 0.01
    W[0] = 0.0                                                        # a silent channel
    Z = g.random(wshape[1]) + 0.1
    W, H, Z = W / W.sum(P._axes(W), keepdims=True), H / H.sum(P._axes(H), keepdims=True), Z / Z.sum()
    if len(wshape) == 2:
        vshape = (hshape[0], wshape[0])
    else:
        vshape = (hshape[0], wshape[0]) + tuple(a + t - 1 for a, t in zip(hshape[2:], wshape[2:]))
    V = g.random(vshape)
    Vn = V / V.sum()
    GtH, GW = O._plca_products(_t(Vn), _t(W), _t(H), _t(Z))
    for train in P.TRAINS:
        aW, aH, aZ = alphas
        Wr, Hr, Zr = O.plca_em_step(_t(Vn), _t(W), _t(H), _t(Z), aW, aH, aZ, train=train)
        em = P.em_step(W, H, Z, GtH.numpy(), GW.numpy(), train, alphas, u=2.0 ** -53, rounding=False)
        for key, ref in (('W', Wr), ('H', Hr), ('Z', Zr)):
            v = em[key]
            ex = P.excess(ref.numpy(), P.Val(v.v, 2 * v.e))
            assert ex <= 1.0, (train, key, ex)


def _em_case(i):
    c = P.EM_CASES[i]
    r_pad = P.pad_rank(c['rank'])
    f, num, z = P.synthetic((c['rows'], c['rank']), 11 + i, c['nslab'])
    g = np.random.default_rng(5)
    flat = g.standard_normal(c['nslab'] * c['rows_pad'] * r_pad).astype(np.float32)        # padding holds other numbers
    full = flat.reshape(c['nslab'], c['rows_pad'], r_pad)
    full[:, :c['rows'], :c['rank']] = num
    return c, r_pad, f, flat, z


def test_seeded_faults_of_the_em_kernel():
    # the last ragged row left out of a column sum: 33 rows = one full block and one row
    c, r_pad, f, flat, z = _em_case(3)
    assert (c['rows'], c['rank']) == (33, 5) and c['rows'] % P.PLCA_ROWS == 1
    k = P.chain_rows(c['rows'], r_pad)
    slabs = P.read_slabs(flat, c['nslab'], c['rows'], c['rows_pad'], r_pad, c['rank'])
    good = P.stage_em(f, slabs, z, k)
    bad = P.stage_em(f, slabs, z, k, fault='ragged_row')
    assert P.excess(bad['cs'].v, good['cs']) > CLEAR
    # no relu on the numerator; the plane stride taken as rows * r_pad: 31 rows, three slabs, rows_pad 256
    c, r_pad, f, flat, z = _em_case(1)
    assert c['nslab'] == 3 and c['rows_pad'] > c['rows']
    k = P.chain_rows(c['rows'], r_pad)
    slabs = P.read_slabs(flat, c['nslab'], c['rows'], c['rows_pad'], r_pad, c['rank'])
    good = P.stage_em(f, slabs, z, k)
    assert (good['n'] < 0).any() and (good['n'] == 0).any()
    bad = P.stage_em(f, slabs, z, k, fault='no_relu')
    assert P.excess(bad['x'].v, good['x']) > CLEAR
    bad = P.stage_em(f, P.read_slabs(flat, c['nslab'], c['rows'], c['rows_pad'], r_pad, c['rank'], fault='stride'), z, k)
    assert P.excess(bad['x'].v, good['x']) > CLEAR and P.excess(bad['zg'].v, good['zg']) > CLEAR


def test_seeded_faults_of_the_normalize_kernel():
    by = {(c['rows'], c['rank'], c['alpha']): c for c in P.NORM_CASES}
    # clamp at 0 instead of eps: alpha = 0.99 sends the entries below 0.01 to the clamp -- some at 32 rows, most at 300
    big = by[(300, 256, 0.99)]
    assert (P.stage_normalize(*P.norm_problem(big), big['alpha'], 62)['y'].v == P.EPS).mean() > 0.5
    c = by[(32, 33, 0.99)]
    f, d = P.norm_problem(c)
    k = P.chain_rows(c['rows'], P.pad_rank(c['rank']))
    good = P.stage_normalize(f, d, c['alpha'], k)
    assert 0.1 < (good['y'].v == P.EPS).mean() < 0.9
    bad = P.stage_normalize(f, d, c['alpha'], k, fault='clamp0')
    assert P.excess(bad['y'].v, good['y']) > CLEAR
    # alpha - 1.f from an fp32 alpha: the 520-row column at alpha = 1.001, through the renormalisation as well
    c = by[(520, 5, 1.001)]
    f, d = P.norm_problem(c)
    k = P.chain_rows(c['rows'], P.pad_rank(c['rank']))
    good = P.stage_normalize(f, d, c['alpha'], k)
    bad = P.stage_normalize(f, d, c['alpha'], k, fault='alpha_f32')
    assert P.excess(bad['y'].v, good['y']) > CLEAR
    assert P.excess(P.stage_scale(bad['y'], bad['cs']).v, P.stage_scale(good['y'], good['cs'])) > CLEAR
    # ... while alpha = 1.02 differs by 9.3e-7 relative in the constant: still outside the bound of the add
    assert abs(P.prior_shift_f32(1.001) / P.prior_shift(1.001) - 1) > 4e-5
    assert abs(P.prior_shift_f32(1.02) / P.prior_shift(1.02) - 1) < 1e-6
    # the Z kernel at alpha = 1.001: visible where the entries of Z are not large against alpha - 1 (rank 200: 1 / 200)
    zc = [c for c in P.Z_CASES if (c['rank'], c['alpha']) == (200, 1.001)][0]
    z, zg = P.z_problem(zc)
    good = P.stage_z(z, zg, zc['alpha'])
    bad = P.stage_z(z, zg, zc['alpha'], fault='alpha_f32')
    assert P.excess(bad['z'].v, good['z']) > CLEAR


def _dense_step(i, want):
    """Case i of DENSE_CASES and its first step that satisfies ``want(train, alphas)``."""
    case = P.DENSE_CASES[i]
    step = [s for s in P.dense_steps(i) if want(*s)][0]
    Vn, W, H, Z = P.dense_problem(case)
    numW, numH = P.dense_numerators(Vn, W, H, Z)
    r_pad = P.pad_rank(case['R'])
    kw = dict(train=step[0], alphas=step[1], kW=P.chain_rows(case['C'], r_pad), kH=P.chain_rows(case['N'], r_pad))
    return (W, H, Z, numW, numH), kw


@pytest.mark.parametrize('fault,case,want,keys', [
    ('z_new_for_old', 0, lambda t, a: all(t), ('W', 'H')),
    ('no_renorm', 0, lambda t, a: t[0] and a[0] != 1, ('W',)),
    ('prior_after', 1, lambda t, a: t[2] and t[0] and a[2] != 1, ('W',)),
    ('prior_after', 4, lambda t, a: t[2] and t[1] and not t[0] and a[2] != 1, ('H',)),
    ('alpha_f32', 0, lambda t, a: t[0] and a[0] == 1.001, ('W',)),
    ('alpha_f32', 5, lambda t, a: t[1] and a[1] == 1.001, ('H',)),
    ('clamp0', 0, lambda t, a: t[1] and a[1] == 0.99, ('H',)),
    ('no_relu', 2, lambda t, a: t[0], ()),
], ids=lambda x: x if isinstance(x, (str, int)) else '')
def test_seeded_faults_of_the_dense_em_step(fault, case, want, keys):
    args, kw = _dense_step(case, want)
    good = P.em_step(*args, **kw)
    bad = P.em_step(*args, fault=fault, **kw)
    if fault == 'no_relu':
        # the device's numerators are sums of non-negative products: the relu never acts in a fit (it is seeded at the ABI
        # level, test_seeded_faults_of_the_em_kernel); here it must make no difference
        assert all(P.excess(bad[k].v, good[k]) == 0.0 for k in ('W', 'H', 'Z'))
        return
    for k in keys:
        assert P.excess(bad[k].v, good[k]) > CLEAR, (fault, k, P.excess(bad[k].v, good[k]))


@pytest.mark.parametrize('i', [i for i, c in enumerate(P.DENSE_CASES) if (c['precision'] or '') == 'bf16x3'])
def test_start_states_leave_the_split_planes_unambiguous(i):
    """The numerator check of the GPU test holds the kernel to mu_emulation.TOL without an allowance for the lo word of bf16x3
    (``plca_emulation.split_plane_sensitivity``): that is sound where the emulation itself does not move under the AMBIGUITY
    band -- at every start state by less than half the tolerance -- and not after an alpha = 0.99 step."""
    import mu_emulation as E
    case = P.DENSE_CASES[i]
    Vn, W, H, Z = P.dense_problem(case)
    tol = E.TOL['bf16x3']
    for which in ('w', 'h'):
        assert P.split_plane_sensitivity(Vn, W, H, Z, which, 'bf16x3') < tol / 2
    if i == 0:
        numW, numH = P.dense_numerators(Vn, W, H, Z)
        r = P.em_step(W, H, Z, numW, numH, (True, True, False), P.PRIORS[1])       # H_alpha = 0.99: most of H at the clamp
        assert P.split_plane_sensitivity(Vn, r['W'].v, r['H'].v, Z, 'w', 'bf16x3') > tol


def test_every_combination_meets_every_prior_setting():
    seen = {(t, a) for i in range(len(P.DENSE_CASES)) for t, a in P.dense_steps(i)}
    assert seen == {(t, a) for t in P.TRAINS for a in P.PRIORS}
    assert len(P.TRAINS) == 7 and len(set(P.TRAINS)) == 7 and (False, False, False) not in P.TRAINS
    conv = {(t, a) for i in range(len(P.CONV_CASES)) for t, a in P.conv_steps(i)}
    assert conv == {(t, a) for t in (P.TRAINS[0], P.TRAINS[1], P.TRAINS[3]) for a in P.PRIORS}


def test_host_mirrors():
    from torchnmf_amd import _capi
    lib = _capi.load()
    for rank in (1, 5, 32, 33, 64, 100, 128, 129, 200, 256):
        r_pad = lib.nmfmu_pad_rank(rank)
        assert P.pad_rank(rank) == r_pad and P.groups(r_pad) * r_pad == 256
        for rows in (1, 31, 32, 33, 300, 7168, 7169, 9590):
            assert lib.nmfmu_plca_part_bytes(rows, r_pad) == P.part_bytes(rows, r_pad)
        assert lib.nmfmu_plca3_part_bytes(rank) == P.part3_bytes(rank)
    assert lib.nmfmu_plca_part_bytes(0, 32) == 0 == P.part_bytes(0, 32) and lib.nmfmu_plca3_part_bytes(0) == 0
    assert [P.nblk(r) for r in (1, 32, 33, 9590)] == [1, 1, 2, 300]
    # the unrolled loop of colsum_finalize_kernel starts at 225 partial blocks = 7 169 rows
    assert not P.finalize_plan(P.nblk(7168))['unrolled'] and P.finalize_plan(P.nblk(7169))['unrolled']
    big = [c for c in P.EM_CASES if c['rows'] > 7168][0]
    fp = P.finalize_plan(P.nblk(big['rows']))
    assert fp['unrolled'] and fp['tail_after_unrolled'] and fp['terms'] == 10
    assert P.chain_rows(33, 32) == 3 + 7 + 0 + 31 and P.chain_rows(300, 256) == 31 + 0 + 0 + 31
    assert P.chain_rows(9590, 32) == 3 + 7 + 9 + 31
    # every r_pad, groups == 1, no rank padding
    assert {P.pad_rank(c['rank']) for c in P.EM_CASES} == {32, 64, 128, 256}
    assert any(c['rank'] == 256 for c in P.EM_CASES) and any(P.groups(P.pad_rank(c['rank'])) == 1 for c in P.EM_CASES)
    assert {(c['update'], c['zgrad']) for c in P.EM_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c['nslab'] for c in P.EM_CASES} == {1, 3} and any(c['rows_pad'] > c['rows'] for c in P.EM_CASES)
    # plca_scale_kernel's grid-stride loop
    assert any(P.grid_scale(c['rows'] * c['rank'])[1] > 1 for c in P.NORM_CASES)
    assert P.grid_scale(4096 * 256) == (4096, 1) and P.grid_scale(4096 * 256 + 1) == (4096, 2)
    # plca3: chunk bounds
    for c in P.PLCA3_CASES:
        b = P.chunk_bounds(c['outer'], c['inner'])
        n = c['outer'] * c['inner']
        assert len(b) == 64 and sum(max(e1 - e0, 0) for e0, e1 in b) == n and b[0][0] == 0
    assert sum(e1 > e0 for e0, e1 in P.chunk_bounds(3, 5)) == 15                 # fewer elements than chunks
    assert any(c['rank'] > 64 and c['inner'] == 1 for c in P.PLCA3_CASES)
    assert any(c['pitch'] and c['pitch'] > c['rank'] * c['inner'] for c in P.PLCA3_CASES)
    assert any((c['outer'] * c['inner']) % 64 for c in P.PLCA3_CASES)
    assert P.chain_plca3(3, 5) == 71 and P.chain_plca3(300, 70) == 1 + 71
    assert P.prior_shift(1.0) == 0.0 and P.prior_shift(1.001) == float(np.float32(1.001 - 1.0))


def test_half_step_contraction_panel_defaults_to_the_reconstruction_panel():
    import mu_emulation as E
    g = np.random.default_rng(2)
    X, A, B, B2 = g.random((7, 9)), g.random((7, 3)), g.random((9, 3)), g.random((9, 3))
    for prec in ('bf16', 'bf16x3'):
        a = E.half_step(X, A, B, 1.0, prec)
        b = E.half_step(X, A, B, 1.0, prec, B2=B)
        assert np.array_equal(a['num'], b['num'])
        c = E.half_step(X, A, B, 1.0, prec, B2=B2)
        ex = E.half_step(X, A, B, 1.0, prec, rounding=False, B2=B2)['num']
        assert np.allclose(ex, (X / (A @ B.T + E.EPS)) @ B2, rtol=1e-12)
        assert np.abs(c['num'] - ex).max() / np.abs(ex).max() < (1e-2 if prec == 'bf16' else 1e-4)
        assert np.abs(c['num'] - a['num']).max() > 1e-3 * np.abs(ex).max()          # another panel, another numerator
