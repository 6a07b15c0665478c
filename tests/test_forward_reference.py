"""tests/forward_reference.py on the CPU, at every shape of tests/test_gpu_forward_parity.py and with its very inputs: the
float64 references are the oracle's, honest fp32 outputs pass the per-element checkers, and seeded faults of the kind the
forward kernels can have fail them at every shape where they apply."""
import numpy as np
import pytest
import torch

import conv_emulation as CE
import forward_reference as FR
import mu_emulation as E
from oracle import mu_oracle as O
from test_gpu_conv_autograd import SHAPES_1D, SHAPES_2D, SHAPES_3D

CONV_SHAPES = SHAPES_1D + SHAPES_2D + SHAPES_3D
SIPLCA_SHAPES = [SHAPES_1D[1], SHAPES_2D[0], SHAPES_3D[0]]
_ids = lambda s: '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in s)

_conv = {}


def _conv_case(shape, kind='rand'):
    """Factors, references and operand images of one convolutive case, computed once and shared (never modified)."""
    if (shape, kind) not in _conv:
        H, W = (x.numpy() for x in FR.conv_factors(shape, kind))
        ref, em, bound = FR.conv_ref(H, W)
        _conv[shape, kind] = dict(H=H, W=W, ref=ref, em=em, bound=bound, ops=CE.operands(W, H, 'bf16x3'))
    return _conv[shape, kind]


def _fails(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


# ---- the references are the oracle's ------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', FR.DENSE_SHAPES, ids=_ids)
def test_dense_reference_is_the_oracle(shape):
    for kind in ('rand', 'randn'):
        H, W = FR.dense_factors(shape, kind)
        ref, bound = FR.dense_ref(H, W)
        want = O.nmf_reconstruct(H.double(), W.double()).numpy()
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
        assert (bound >= np.abs(ref)).all() and bound.shape == shape[:2]
    if shape in FR.PLCA_SHAPES:
        H, W = FR.dense_factors(shape)
        Z = FR.rank_weights(shape[2])
        ref, bound = FR.plca_dense_ref(H, W, Z)
        want = O.plca_reconstruct(H.double(), W.double(), Z.double()).numpy()
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
        # the fp32 product the device forms is within one u of the true one, element by element
        Ws = FR.scaled_w(W, Z)
        assert Ws.dtype == torch.float32
        assert bool(((Ws.double() - W.double() * Z.double()).abs() <= FR.U * (W.double() * Z.double()).abs()).all())


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_ids)
def test_conv_reference_is_the_oracle_and_the_emulation_passes_tier2(shape):
    c = _conv_case(shape)
    H64, W64 = torch.from_numpy(c['H']).double(), torch.from_numpy(c['W']).double()
    want = O.convnd_reconstruct(H64, W64).numpy()
    assert c['ref'].shape == want.shape == c['em'].shape == c['bound'].shape
    assert np.abs(c['ref'] - want).max() <= 1e-12 * np.abs(want).max()
    if len(shape[3]) == 1:
        assert np.abs(c['ref'] - O.nmfd_reconstruct(H64, W64).numpy()).max() <= 1e-12 * np.abs(want).max()
    # the unrounded emulation is the same contraction (its layout and ``from_w`` are right) ...
    plain = FR.from_w(CE.reconstruction(CE.operands(c['W'], c['H'], 'bf16x3', rounding=False), 2), shape[0], want.shape[2:])
    assert np.abs(plain - want).max() <= 1e-12 * np.abs(want).max()
    # ... and the rounded one sits inside tier 2 on its own, using most of the 3 * 2^-16 only in the worst case
    used = FR.conv_tier2(c['em'], c['ref'], c['bound'], FR.conv_k(c['W']))
    assert used <= 1.0
    assert np.abs(c['em'] - c['ref']).max() <= 2.0 ** -16 * c['bound'].max()


@pytest.mark.parametrize('shape', SIPLCA_SHAPES, ids=_ids)
def test_siplca_reference_is_the_oracle(shape):
    H, W = FR.conv_factors(shape)
    Z = FR.rank_weights(shape[2])
    want = O.plca_reconstruct(H.double(), W.double(), Z.double()).numpy()
    got = FR._conv64(H.numpy(), FR._wz64(W.numpy(), Z.numpy()).numpy())
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # an honest output of the scaled model passes with and without Z named
    ops = CE.operands(FR.scaled_w(W, Z).numpy(), H.numpy(), 'bf16x3')
    for acc in FR.fp32_accumulations(ops):
        out = FR.from_w(acc, shape[0], want.shape[2:])
        FR.check_conv(out, H.numpy(), W.numpy(), Z.numpy())
        FR.check_conv(out, H.numpy(), FR.scaled_w(W, Z).numpy())


# ---- honest outputs pass -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_ids)
def test_honest_conv_outputs_pass(shape):
    c = _conv_case(shape)
    ops = c['ops']
    order = CE.fp32_order_error(ops['Wm'], (ops['Hu'][0].T, ops['Hu'][1].T), CE.target_w(c['em']))
    print(f'{shape}: reference-side fp32 order error {order:.3g}')
    assert order <= E.TOL['bf16x3']
    for acc in FR.fp32_accumulations(ops):
        fig = FR.check_conv(FR.from_w(acc, shape[0], c['ref'].shape[2:]), c['H'], c['W'])
        assert fig.elem_err <= E.TOL['bf16x3'] and fig.ratio <= 1.0
    FR.check_conv(c['em'], c['H'], c['W'])
    for kind in ('int', 'zeros'):
        k = _conv_case(shape, kind)
        for acc in FR.fp32_accumulations(k['ops']):
            out = FR.from_w(acc, shape[0], k['ref'].shape[2:])
            FR.check_conv(out, k['H'], k['W'])
            if kind == 'int':
                assert np.array_equal(out.astype(np.float64), k['ref'])       # every partial sum is below 2^24


@pytest.mark.parametrize('shape', FR.DENSE_SHAPES, ids=_ids)
def test_honest_dense_outputs_pass(shape):
    for kind in ('rand', 'randn', 'int', 'zeros'):
        H, W = (x.numpy() for x in FR.dense_factors(shape, kind))
        out = H @ W.T
        assert out.dtype == np.float32
        assert FR.check_dense(out, H, W) <= 1.0
        if kind == 'int':
            assert np.array_equal(out.astype(np.float64), FR.dense_ref(H, W)[0])
    if shape in FR.PLCA_SHAPES:
        H, W = FR.dense_factors(shape)
        Z = FR.rank_weights(shape[2])
        out = H.numpy() @ FR.scaled_w(W, Z).numpy().T
        FR.check_dense(out, H.numpy(), FR.scaled_w(W, Z).numpy())
        FR.check_dense(out, H.numpy(), W.numpy(), Z.numpy())


# ---- seeded faults fail -------------------------------------------------------------------------------------------------
def _planes_product(ops, lo_hi=True, cols=slice(None)):
    (wh, wl), (hh, hl) = ops['Wm'], ops['Hu']
    wh, wl, hh, hl = wh[:, cols], wl[:, cols], hh[:, cols], hl[:, cols]
    if lo_hi:
        return E._gemm([wh, wl], hh.T, hl.T)
    return wh @ hh.T + wh @ hl.T


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_ids)
def test_conv_faults_fail(shape):
    B, C, R, lh, taps = shape
    c = _conv_case(shape)
    H, W, ops = c['H'], c['W'], c['ops']
    ls = c['ref'].shape[2:]
    honest = FR.from_w(_planes_product(ops), B, ls)
    assert np.array_equal(honest, c['em'])
    applied = []
    # (a) the lo x hi product dropped (the left operand's lo plane never read)
    if ops['Wm'][1].any():
        bad = FR.from_w(_planes_product(ops, lo_hi=False), B, ls)
        err = float(E.elem_err(CE.target_w(bad), CE.target_w(c['em'])).max())
        print(f'{shape}: lo x hi dropped -> elem_err {err:.3g}')
        _fails(FR.conv_tier1, bad, c['em'])
        _fails(FR.check_conv, bad, H, W)
        applied.append('a')
    # (b) W flipped along one tap axis of extent > 1
    for ax, t in enumerate(taps):
        if t > 1:
            bad = FR.conv_ref(H, np.flip(W, axis=2 + ax).copy())[1]
            _fails(FR.check_conv, bad, H, W)
            _fails(FR.conv_tier2, bad, c['ref'], c['bound'], FR.conv_k(W))
            applied.append('b')
    # (c) H shifted by one along one axis
    for ax, n in enumerate(lh):
        if n > 1:
            bad = FR.conv_ref(np.roll(H, 1, axis=2 + ax), W)[1]
            _fails(FR.check_conv, bad, H, W)
            _fails(FR.conv_tier2, bad, c['ref'], c['bound'], FR.conv_k(W))
            applied.append('c')
    # (d) the last (r, t) column left out of the contraction
    bad = FR.from_w(_planes_product(ops, cols=slice(0, R * FR._prod(taps) - 1)), B, ls)
    _fails(FR.check_conv, bad, H, W)
    _fails(FR.conv_tier2, bad, c['ref'], c['bound'], FR.conv_k(W))
    # (e) the output rounded to bf16
    bad = E.round_bf16(c['em']).reshape(c['em'].shape)
    if not np.array_equal(bad, c['em']):
        _fails(FR.conv_tier1, bad, c['em'])
        _fails(FR.check_conv, bad, H, W)
        applied.append('e')
    # (h) one exact-zero output element (a silent channel) replaced by 2^-30
    z = _conv_case(shape, 'zeros')
    zero = np.argwhere(z['bound'] == 0)
    assert len(zero) and (z['em'][z['bound'] == 0] == 0).all()
    bad = z['em'].copy()
    bad[tuple(zero[len(zero) // 2])] = 2.0 ** -30
    FR.check_conv(z['em'], z['H'], z['W'])
    _fails(FR.check_conv, bad, z['H'], z['W'])
    _fails(FR.conv_tier2, bad, z['ref'], z['bound'], FR.conv_k(z['W']))
    # every fault applies wherever its premise holds: random factors carry lo planes and are no bf16 numbers
    assert 'a' in applied and 'e' in applied
    assert ('b' in applied) == any(t > 1 for t in taps) and ('c' in applied) == any(n > 1 for n in lh)


@pytest.mark.parametrize('shape', FR.DENSE_SHAPES, ids=_ids)
def test_dense_faults_fail(shape):
    N, C, R = shape
    for kind in ('rand', 'randn'):
        H, W = (x.numpy() for x in FR.dense_factors(shape, kind))
        honest = H @ W.T
        FR.check_dense(honest, H, W)
        # (e) the output rounded to bf16
        _fails(FR.check_dense, E.round_bf16(honest).reshape(N, C), H, W)
        # (f) the factors rounded to bf16 first
        Hb, Wb = E.round_bf16(H).reshape(N, R), E.round_bf16(W).reshape(C, R)
        _fails(FR.check_dense, Hb @ Wb.T, H, W)
        # (g) the term r = R - 1 dropped for the rows of the last, ragged 128-row tile only
        if N % 128:
            bad = honest.copy()
            m0 = N // 128 * 128
            bad[m0:] = H[m0:, :R - 1] @ W[:, :R - 1].T
            assert np.array_equal(bad[:m0], honest[:m0])
            _fails(FR.check_dense, bad, H, W)
    # (h) one exact-zero output element replaced by 2^-30
    H, W = (x.numpy() for x in FR.dense_factors(shape, 'zeros'))
    honest = H @ W.T
    FR.check_dense(honest, H, W)
    bad = honest.copy()
    assert bad[N // 2, C - 1] == 0
    bad[N // 2, C - 1] = 2.0 ** -30
    _fails(FR.check_dense, bad, H, W)
    # a NaN never passes
    bad = honest.copy()
    bad[0, 0] = np.nan
    _fails(FR.check_dense, bad, H, W)
