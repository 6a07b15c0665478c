"""The forward (reconstruct) kernels per element: ``reconstruct_kernel`` behind ``NMF / PLCA.reconstruct`` and the
pack2d -> unfold -> split-bf16 GEMM (``EPI_F32``) sequence of ``nmfd_engine.reconstruct`` behind ``NMFD / NMF2D / NMF3D /
SIPLCA*.reconstruct``.  References, bounds and inputs are tests/forward_reference.py's (its docstring derives the bounds;
tests/test_forward_reference.py shows on the CPU that seeded faults fail them at these very inputs).  Every element of every
output is compared; outputs the test allocates itself start as NaN.

1. Dense: ``|got - ref64| <= (R + 2) u |H| |W|^T`` with rand and randn factors at the shapes that reach each branch of the
   kernel (scalar / float4 loads, a short last stage, ragged tiles); integer factors 0..15 reproduce the integer product
   bit for bit; zero rows give exact zeros and nothing else is zero; an output row stride other than the column count leaves
   everything outside the valid block untouched; leading dimensions of ``H`` are the flattened call.
2. PLCA: the same bound with fp32(W * Z) as the left factor, and ``(R + 3) u`` against the true float64 ``H (W Z)^T``.
3. Convolutive: tier 1 against the emulated accumulators within ``mu_emulation.TOL['bf16x3']``, tier 2 against the float64
   convolution; integer factors are exact in bf16 and reproduce the float64 convolution bit for bit; a silent channel is
   exactly zero and a silent rank leaves the reduced model's values.
4. The operand planes of the stand-alone forward, through the C ABI as ``nmfd_engine.reconstruct`` calls it: bit-equal to
   ``conv_emulation.encode`` of the emulated operands inside the valid block, zero in all padding.

Recorded on the first MI355X run (worst error / bound; recorded, not used to set a bound):
dense 0.061 ... 0.275 of the bound with rand factors (0.275 at (33, 130, 7), 0.061 at rank 256) and 0.023 ... 0.343 with
randn; PLCA 0.153 ... 0.273 with fp32(W Z) and 0.152 ... 0.299 against the float64 W Z; convolutive ``elem_err`` against the
emulation 0 (single element) ... 4.26e-7 (C = 257, rank 33) of 4e-6 and 0.046 ... 0.342 of the float64 bound (0.342 at the 3-D
shape with the middle tap axis of extent 1); SIPLCA / SIPLCA2 / SIPLCA3 2.15e-7 / 2.56e-7 / 1.68e-7 and 0.158 / 0.162 / 0.185;
integer products, zeros, the strided output and all operand planes exact.  77 tests, 3 s.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record
import conv_emulation as CE
import forward_reference as FR
from test_gpu_conv_autograd import SHAPES_1D, SHAPES_2D, SHAPES_3D

pytestmark = pytest.mark.gpu

CONV_SHAPES = SHAPES_1D + SHAPES_2D + SHAPES_3D
SIPLCA_CASES = [('SIPLCA', SHAPES_1D[1]), ('SIPLCA2', SHAPES_2D[0]), ('SIPLCA3', SHAPES_3D[0])]
PLANE_SHAPES = [SHAPES_1D[2], SHAPES_1D[1], SHAPES_2D[1], SHAPES_3D[1]]
_ids = lambda s: '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in s)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _conv_model(nd):
    from torchnmf_amd import nmf
    return (nmf.NMFD, nmf.NMF2D, nmf.NMF3D)[nd - 1]


# ---- dense ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['rand', 'randn'])
@pytest.mark.parametrize('shape', FR.DENSE_SHAPES, ids=_ids)
def test_dense_per_element(dev, shape, kind):
    from torchnmf_amd.nmf import NMF
    H, W = FR.dense_factors(shape, kind)
    out = NMF.reconstruct(H.to(dev), W.to(dev))
    assert out.shape == shape[:2] and out.dtype == torch.float32 and out.is_contiguous()
    frac = FR.check_dense(out.cpu().numpy(), H.numpy(), W.numpy())
    record('forward_dense', case=str(shape), factors=kind, worst_fraction_of_bound=frac)
    print(f'forward_dense {shape} {kind}: worst |got - ref| / bound = {frac:.3f}')


@pytest.mark.parametrize('shape', FR.DENSE_SHAPES, ids=_ids)
def test_dense_integer_exact(dev, shape):
    """Integers 0..15: every partial sum is below 2^24, so any order gives the integer product -- no tolerance."""
    from torchnmf_amd.nmf import NMF
    H, W = FR.dense_factors(shape, 'int')
    out = NMF.reconstruct(H.to(dev), W.to(dev)).cpu()
    want = H.double() @ W.double().t()
    assert float(want.max()) < 2 ** 24
    assert torch.equal(out, want.float())


@pytest.mark.parametrize('shape', [s for s in FR.DENSE_SHAPES if s[0] > 1 and s[1] > 1], ids=_ids)
def test_dense_exact_zeros(dev, shape):
    from torchnmf_amd.nmf import NMF
    N, C, _ = shape
    H, W = FR.dense_factors(shape, 'zeros')
    out = NMF.reconstruct(H.to(dev), W.to(dev)).cpu()
    want_zero = torch.zeros(N, C, dtype=torch.bool)
    want_zero[N // 2] = True
    want_zero[:, C // 3] = True
    assert torch.equal(out == 0, want_zero)
    FR.check_dense(out.numpy(), H.numpy(), W.numpy())


def _reconstruct_capi(H, W, out, ld):
    from torchnmf_amd import _capi
    assert H.is_contiguous() and W.is_contiguous() and out.is_contiguous()
    _capi.check(_capi.load().nmfmu_reconstruct(H.data_ptr(), H.shape[0], W.data_ptr(), W.shape[0], H.shape[1],
                                               out.data_ptr(), ld, torch.cuda.current_stream().cuda_stream),
                'nmfmu_reconstruct')
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', [(300, 257, 33), (129, 127, 36)], ids=_ids)
def test_dense_row_stride(dev, shape):
    """``ld`` = columns + 5 into a NaN-filled (rows + 3, columns + 5) buffer: the valid block is the contiguous call's, and
    nothing outside it is written."""
    M, K, _ = shape
    H, W = (x.to(dev) for x in FR.dense_factors(shape))
    plain = torch.full((M, K), float('nan'), device=dev)
    _reconstruct_capi(H, W, plain, K)
    wide = torch.full((M + 3, K + 5), float('nan'), device=dev)
    _reconstruct_capi(H, W, wide, K + 5)
    assert bool(torch.isfinite(plain).all()) and torch.equal(wide[:M, :K], plain)
    outside = torch.ones(M + 3, K + 5, dtype=torch.bool, device=dev)
    outside[:M, :K] = False
    assert bool(torch.isnan(wide[outside]).all())
    FR.check_dense(plain.cpu().numpy(), H.cpu().numpy(), W.cpu().numpy())


@pytest.mark.parametrize('C,R', [(130, 7), (127, 36)])
def test_dense_leading_dimensions(dev, C, R):
    from torchnmf_amd.nmf import NMF
    g = torch.Generator().manual_seed(C + R)
    H, W = torch.rand(2, 3, 17, R, generator=g).to(dev), torch.rand(C, R, generator=g).to(dev)
    out = NMF.reconstruct(H, W)
    assert out.shape == (2, 3, 17, C)
    assert torch.equal(out.reshape(-1, C), NMF.reconstruct(H.reshape(-1, R), W))
    FR.check_dense(out.cpu().numpy(), H.cpu().numpy(), W.cpu().numpy())


# ---- PLCA -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', FR.PLCA_SHAPES, ids=_ids)
def test_plca_per_element(dev, shape):
    from torchnmf_amd.plca import PLCA
    H, W = FR.dense_factors(shape)
    Z = FR.rank_weights(shape[2])
    out = PLCA.reconstruct(H.to(dev), W.to(dev), Z.to(dev))
    assert out.shape == shape[:2] and out.dtype == torch.float32
    got = out.cpu().numpy()
    frac = FR.check_dense(got, H.numpy(), FR.scaled_w(W, Z).numpy())
    frac64 = FR.check_dense(got, H.numpy(), W.numpy(), Z.numpy())
    record('forward_plca', case=str(shape), worst_fraction_of_bound=frac, worst_fraction_of_bound_true_wz=frac64)
    print(f'forward_plca {shape}: worst |got - ref| / bound = {frac:.3f} (fp32 W Z), {frac64:.3f} (float64 W Z)')
    # the module: its own (normalised) tensors through the same static call, and norm = one fp32 multiplication
    m = PLCA(W=W, H=H, Z=Z).to(dev)
    plain = m()
    assert torch.equal(plain, PLCA.reconstruct(m.H.detach(), m.W.detach(), m.Z.detach()))
    FR.check_dense(plain.detach().cpu().numpy(), m.H.detach().cpu().numpy(), m.W.detach().cpu().numpy(),
                   m.Z.detach().cpu().numpy())
    assert torch.equal(m(norm=2.5).detach().cpu(), 2.5 * plain.detach().cpu())


# ---- convolutive ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_ids)
def test_conv_per_element(dev, shape):
    B, C, R, lh, taps = shape
    H, W = FR.conv_factors(shape)
    out = _conv_model(len(lh)).reconstruct(H.to(dev), W.to(dev))
    assert out.shape == (B, C) + tuple(a + t - 1 for a, t in zip(lh, taps)) and out.dtype == torch.float32
    assert out.is_contiguous()
    fig = FR.check_conv(out.cpu().numpy(), H.numpy(), W.numpy())
    record('forward_conv', case=str(shape), worst_elem_err=fig.elem_err, worst_fraction_of_bound=fig.ratio)
    print(f'forward_conv {shape}: elem_err {fig.elem_err:.3g} against the emulation, {fig.ratio:.3f} of the float64 bound')


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_ids)
def test_conv_integer_exact(dev, shape):
    """Integers 0..15 are bf16 numbers: the lo planes are zero, every partial sum is below 2^24 -- no tolerance."""
    H, W = FR.conv_factors(shape, 'int')
    out = _conv_model(len(shape[3])).reconstruct(H.to(dev), W.to(dev)).cpu()
    want = torch.from_numpy(FR.conv_ref(H.numpy(), W.numpy())[0])
    assert float(want.max()) < 2 ** 24
    assert torch.equal(out, want.float())


@pytest.mark.parametrize('shape', [s for s in CONV_SHAPES if s[1] > 1 and s[2] > 1], ids=_ids)
def test_conv_exact_zeros(dev, shape):
    """A silent channel reconstructs to exact zeros; a silent rank leaves the model without it."""
    B, C, R, lh, taps = shape
    H, W = FR.conv_factors(shape, 'zeros')
    out = _conv_model(len(lh)).reconstruct(H.to(dev), W.to(dev)).cpu()
    assert bool((out[:, C // 3] == 0).all())
    others = [c for c in range(C) if c != C // 3]
    assert bool((out[:, others] > 0).all())
    fig = FR.check_conv(out.numpy(), H.numpy(), W.numpy())
    Hr, Wr = H[:, :R - 1].contiguous().numpy(), W[:, :R - 1].contiguous().numpy()
    ref, _, bound = FR.conv_ref(Hr, Wr)
    frac = FR.conv_tier2(out.numpy(), ref, bound, FR.conv_k(Wr))
    record('forward_conv_zeros', case=str(shape), worst_elem_err=fig.elem_err, worst_fraction_of_bound=max(fig.ratio, frac))


# ---- SIPLCA ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,shape', SIPLCA_CASES, ids=[k for k, _ in SIPLCA_CASES])
def test_siplca_per_element(dev, kind, shape):
    from torchnmf_amd import plca
    cls = getattr(plca, kind)
    B, C, R, lh, taps = shape
    H, W = FR.conv_factors(shape)
    Z = FR.rank_weights(R)
    out = cls.reconstruct(H.to(dev), W.to(dev), Z.to(dev))
    assert out.shape == (B, C) + tuple(a + t - 1 for a, t in zip(lh, taps)) and out.dtype == torch.float32
    fig = FR.check_conv(out.cpu().numpy(), H.numpy(), W.numpy(), Z.numpy())
    record('forward_siplca', case=kind, worst_elem_err=fig.elem_err, worst_fraction_of_bound=fig.ratio)
    print(f'forward_siplca {kind}: elem_err {fig.elem_err:.3g} against the emulation, {fig.ratio:.3f} of the float64 bound')
    m = cls(W=W, H=H, Z=Z).to(dev)
    plain = m()
    assert torch.equal(plain, cls.reconstruct(m.H.detach(), m.W.detach(), m.Z.detach()))
    FR.check_conv(plain.detach().cpu().numpy(), m.H.detach().cpu().numpy(), m.W.detach().cpu().numpy(),
                  m.Z.detach().cpu().numpy())


# ---- the operand planes of the stand-alone forward ---------------------------------------------------------------------
def _pad128(n):
    return (n + 127) // 128 * 128


def _nan_plane(rows, cols, dev):
    return torch.full((rows * cols,), CE.nan_word('bf16'), dtype=torch.int16, device=dev)


def _expect_plane(vals, rows_pad, cols_pad):
    full = np.zeros((rows_pad, cols_pad), dtype=np.int16)
    full[:vals.shape[0], :vals.shape[1]] = CE.encode(vals, 'bf16')
    return full


@pytest.mark.parametrize('shape', PLANE_SHAPES, ids=_ids)
def test_operand_planes(dev, shape):
    """nmfmu_pack2d and nmfmu_conv_unfold / nmfmu_convnd_unfold with the arguments of ``nmfd_engine.reconstruct`` into
    NaN-filled planes: Wm [c][(r, t)], Hu [(b, l)][(r, t)] and HuT [(r, t)][(b, l)], hi and lo, word for word."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    B, C, R, lh, taps = shape
    nd = len(lh)
    H, W = FR.conv_factors(shape)
    Hd, Wd = H.to(dev), W.to(dev)
    T = FR._prod(taps)
    L = FR._prod([a + t - 1 for a, t in zip(lh, taps)])
    RT = R * T
    cp, blp, rpp = _pad128(C), _pad128(B * L), _pad128(RT)
    wm = [_nan_plane(cp, rpp, dev) for _ in range(2)]
    hu = [_nan_plane(blp, rpp, dev) for _ in range(2)]
    hut = [_nan_plane(rpp, blp, dev) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.nmfmu_pack2d(Wd.data_ptr(), C, RT, 1, RT, 0, 1, 1, 0, cp, rpp, None, wm[0].data_ptr(), wm[1].data_ptr(),
                                 None, stream), 'nmfmu_pack2d')
    if nd == 1:
        _capi.check(lib.nmfmu_conv_unfold(Hd.data_ptr(), B, R, lh[0], T, hu[0].data_ptr(), hu[1].data_ptr(),
                                          hut[0].data_ptr(), hut[1].data_ptr(), blp, rpp, stream), 'nmfmu_conv_unfold')
    else:
        _capi.check(lib.nmfmu_convnd_unfold(Hd.data_ptr(), B, R, nd, (ctypes.c_int32 * nd)(*lh), (ctypes.c_int32 * nd)(*taps),
                                            hu[0].data_ptr(), hu[1].data_ptr(), hut[0].data_ptr(), hut[1].data_ptr(), blp,
                                            rpp, stream), 'nmfmu_convnd_unfold')
    torch.cuda.synchronize()
    ops = CE.operands(W.numpy(), H.numpy(), 'bf16x3')
    assert ops['Wm'][0].shape == (C, RT) and ops['Hu'][0].shape == (B * L, RT)
    for name, planes, rows_pad, cols_pad, vals in (('Wm', wm, cp, rpp, ops['Wm']), ('Hu', hu, blp, rpp, ops['Hu']),
                                                   ('HuT', hut, rpp, blp, [p.T for p in ops['Hu']])):
        for part, plane, v in zip(('hi', 'lo'), planes, vals):
            got = plane.cpu().numpy().reshape(rows_pad, cols_pad)
            want = _expect_plane(v, rows_pad, cols_pad)
            assert not (got == np.int16(CE.nan_word('bf16'))).any(), (name, part, 'a word nobody wrote')
            assert np.array_equal(got, want), (name, part, int((got != want).sum()))
