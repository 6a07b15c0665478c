"""torch.autograd through NMFD / NMF2D / NMF3D.forward: ``nmfmu_conv_backward`` per element, then end to end.

References are computed here on the CPU in float64 with plain torch: ``F.convNd(H64, W64.flip(..), padding=T - 1)`` and
``torch.autograd.grad`` with the given ``G``; every element of every output is compared.  u = 2^-24 throughout.  ``G`` is
``randn``, the factors are ``rand`` (non-negative), seeds are fixed; outputs and scratch start as NaN, so an element nobody
wrote cannot pass.

1. Through the C ABI, per element: ``|got - ref64| <= (K + 2) u bound64`` -- the standard bound of an fp32 dot product, which
   holds for any summation order and so covers the MFMA's order, the split of the contraction and the slab sum (zero terms
   of a padded stage only loosen it).  ``bound64`` is the same contraction with ``|G|`` and the non-negative factor;
   ``K = B prod(L)`` for grad_W and ``K = C prod(T)`` for grad_H.
2. A ``grad_h``-only and a ``grad_w``-only call are ``torch.equal`` to the both-outputs call, the scratch of both is the sum of
   the two, and the same call twice gives ``torch.equal`` results (no floating-point atomics).
3. End to end for NMFD, NMF2D and NMF3D: ``m()`` carries a ``grad_fn`` and ``_nmf_source`` and is bit-equal to the ``no_grad``
   forward; the device's own upstream gradient of ``beta_div(out, V, beta)`` is captured with ``out.register_hook`` and
   ``m.W.grad`` / ``m.H.grad`` are compared per element, under the bound of 1, with the float64 backward of that captured
   ``G`` -- which isolates the new kernels from the split-bf16 forward's rounding.
4. Surface: a frozen factor, a non-leaf ``H``, a float64 module, a non-contiguous upstream gradient, ``torch.no_grad()``,
   three SGD steps.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (B, C, R, lh, taps)
SHAPES_1D = [(1, 1, 1, (1,), (1,)), (2, 33, 7, (50,), (5,)), (1, 130, 3, (40,), (45,)), (3, 129, 8, (300,), (16,)),
             (1, 257, 33, (129,), (4,)), (1, 40, 8, (70,), (1,))]
SHAPES_2D = [(2, 20, 5, (9, 14), (3, 4)), (1, 130, 4, (33, 40), (5, 2)), (1, 8, 3, (6, 5), (1, 7))]
SHAPES_3D = [(1, 10, 3, (4, 5, 6), (2, 3, 2)), (2, 33, 2, (3, 9, 8), (3, 1, 4))]
# chosen from the split rule (include/nmfmu.h; rows / contraction = B prod(lh) / C prod(T) for grad_H and the reverse for
# grad_W): 1000 / 1100 at rank 7 gives 7 and 8 parts, 700 / 650 at rank 130 (two 128-wide rank tiles) gives 5 and 5, the last
# part short every time
SPLIT_SHAPES = [(2, 55, 7, (500,), (20,)), (1, 13, 130, (20, 35), (5, 10))]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def _arr(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def _ws(shape, want_h=True, want_w=True):
    from torchnmf_amd import _capi
    B, C, R, lh, taps = shape
    s = (ctypes.c_int * 2)()
    n = _capi.load().nmfmu_conv_backward_ws(B, C, R, len(lh), _arr(lh), _arr(taps), int(want_h), int(want_w), s)
    assert n >= 0, n
    return n, s[0], s[1]


def _backward(shape, G, W, H, want_h=True, want_w=True):
    """nmfmu_conv_backward on contiguous device tensors; outputs and scratch start as NaN."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    B, C, R, lh, taps = shape
    assert G.is_contiguous() and W.is_contiguous() and H.is_contiguous()
    n_ws, _, _ = _ws(shape, want_h, want_w)
    ws = torch.full((max(n_ws, 1),), float('nan'), device=G.device)
    gh = torch.full_like(H, float('nan')) if want_h else None
    gw = torch.full_like(W, float('nan')) if want_w else None
    _capi.check(lib.nmfmu_conv_backward(G.data_ptr(), W.data_ptr(), H.data_ptr(), B, C, R, len(lh), _arr(lh), _arr(taps),
                                        gh.data_ptr() if want_h else None, gw.data_ptr() if want_w else None,
                                        ws.data_ptr() if n_ws else None, torch.cuda.current_stream().cuda_stream),
                'nmfmu_conv_backward')
    torch.cuda.synchronize()
    return gh, gw


def _reference(G, H, W):
    """float64 (grad_H, bound_H, grad_W, bound_W) of the reference's reconstruction for the upstream gradient G (CPU)."""
    nd = H.dim() - 2
    conv = (F.conv1d, F.conv2d, F.conv3d)[nd - 1]
    dims = tuple(range(2, 2 + nd))
    H64, W64 = H.double().requires_grad_(), W.double().requires_grad_()
    out = conv(H64, W64.flip(dims), padding=tuple(t - 1 for t in W.shape[2:]))
    assert out.shape == G.shape
    gH, gW = torch.autograd.grad(out, (H64, W64), G.double(), retain_graph=True)
    aH, aW = torch.autograd.grad(out, (H64, W64), G.double().abs())      # the factors are non-negative
    k_h = W.shape[0] * _prod(W.shape[2:])                                  # C prod(T)
    k_w = G.shape[0] * _prod(G.shape[2:])                                  # B prod(L)
    return gH, (k_h + 2) * U * aH, gW, (k_w + 2) * U * aW


_cases = {}


def _case(shape):
    """Inputs and float64 references of one shape, computed once and shared."""
    if shape not in _cases:
        B, C, R, lh, taps = shape
        g = torch.Generator().manual_seed(B * 7 + C * 3 + R + 11 * _prod(lh) + 13 * _prod(taps))
        G = torch.randn(B, C, *(a + t - 1 for a, t in zip(lh, taps)), generator=g)
        H, W = torch.rand(B, R, *lh, generator=g), torch.rand(C, R, *taps, generator=g)
        ref_h, bound_h, ref_w, bound_w = _reference(G, H, W)
        _cases[shape] = dict(G=G, H=H, W=W, ref_h=ref_h, bound_h=bound_h, ref_w=ref_w, bound_w=bound_w)
    return _cases[shape]


def _check(name, tag, what, got, ref, bound):
    got = got.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (what, tag)
    frac = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    record(name, case=str(what), output=tag, worst_fraction_of_bound=frac)
    print(f'{name} {what} grad_{tag}: worst |got - ref| / bound = {frac:.3f}')
    assert bool(((got - ref).abs() <= bound).all()), (what, tag, frac)


@pytest.mark.parametrize('shape', SHAPES_1D + SHAPES_2D + SHAPES_3D + SPLIT_SHAPES)
def test_conv_backward_per_element(dev, shape):
    c = _case(shape)
    B, C, R, lh, taps = shape
    if shape in SPLIT_SHAPES:
        _, sh, sw = _ws(shape)
        assert sh >= 3 and sw >= 3, (sh, sw)
        bj, ct = B * _prod(lh), C * _prod(taps)
        for contraction, parts in ((ct, sh), (bj, sw)):      # the rule: parts of ceil(stages / parts) * 32 steps
            stages = -(-contraction // 32)
            part_len = -(-stages // parts) * 32
            assert contraction % part_len != 0 and (parts - 1) * part_len < contraction < parts * part_len
    gh, gw = _backward(shape, c['G'].to(dev), c['W'].to(dev), c['H'].to(dev))
    _check('conv_backward', 'H', shape, gh, c['ref_h'], c['bound_h'])
    _check('conv_backward', 'W', shape, gw, c['ref_w'], c['bound_w'])


@pytest.mark.parametrize('shape', [SHAPES_1D[3], SHAPES_2D[1], SHAPES_3D[1]] + SPLIT_SHAPES)
def test_conv_backward_one_output_and_determinism(dev, shape):
    """Either output NULL: the other one is bit-equal to the both-outputs call (and, the scratch being NaN, does not depend
    on the slab of the half that was left out); the same call twice is bit-equal."""
    c = _case(shape)
    G, W, H = c['G'].to(dev), c['W'].to(dev), c['H'].to(dev)
    gh, gw = _backward(shape, G, W, H)
    gh1, none_w = _backward(shape, G, W, H, want_w=False)
    none_h, gw1 = _backward(shape, G, W, H, want_h=False)
    assert none_w is None and none_h is None
    assert torch.equal(gh, gh1) and torch.equal(gw, gw1)
    assert _ws(shape)[0] == _ws(shape, want_w=False)[0] + _ws(shape, want_h=False)[0]
    gh2, gw2 = _backward(shape, G, W, H)
    assert torch.equal(gh, gh2) and torch.equal(gw, gw2)


# ---- end to end -----------------------------------------------------------------------------------------------------
# (class name, H shape, W shape): B = 2, an odd channel count, sizes off every tile
MODELS = {'NMFD': ((2, 3, 21), (9, 3, 5)), 'NMF2D': ((2, 3, 7, 9), (9, 3, 2, 3)), 'NMF3D': ((2, 2, 4, 5, 6), (5, 2, 2, 3, 2))}


def _model(kind, dev, seed=5, **kw):
    from torchnmf_amd import nmf
    hs, ws = MODELS[kind]
    g = torch.Generator().manual_seed(seed)
    H0, W0 = torch.rand(*hs, generator=g) + 0.1, torch.rand(*ws, generator=g) + 0.1
    out_shape = (hs[0], ws[0]) + tuple(a + t - 1 for a, t in zip(hs[2:], ws[2:]))
    V = torch.rand(*out_shape, generator=g) * 5 + 0.5
    return getattr(nmf, kind)(W=W0, H=H0, **kw).to(dev), H0, W0, V


@pytest.mark.parametrize('beta', [2, 1, 0.5])
@pytest.mark.parametrize('kind', ['NMFD', 'NMF2D', 'NMF3D'])
def test_end_to_end(dev, kind, beta):
    from torchnmf_amd.metrics import beta_div
    m, H0, W0, V = _model(kind, dev)
    with torch.no_grad():
        plain = m()
    assert plain.grad_fn is None
    out = m()
    assert out.grad_fn is not None and out._nmf_source[0] is m
    assert torch.equal(out.detach(), plain)
    seen = []
    out.register_hook(seen.append)
    beta_div(out, V.to(dev), beta).backward()
    assert len(seen) == 1 and seen[0].shape == out.shape
    ref_h, bound_h, ref_w, bound_w = _reference(seen[0].cpu(), H0, W0)
    assert m.H.grad.shape == m.H.shape and m.W.grad.shape == m.W.shape
    _check('conv_autograd_end_to_end', 'H', (kind, beta), m.H.grad, ref_h, bound_h)
    _check('conv_autograd_end_to_end', 'W', (kind, beta), m.W.grad, ref_w, bound_w)


def _fixed_upstream(out, seed=9):
    return torch.randn(*out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)


def _grads(m, upstream=None, **fwd):
    """(H.grad, W.grad) of sum(m() * upstream) with a fixed upstream gradient."""
    m.zero_grad()
    out = m(**fwd)
    (out * (_fixed_upstream(out) if upstream is None else upstream)).sum().backward()
    return m.H.grad, m.W.grad


@pytest.mark.parametrize('kind', ['NMFD', 'NMF2D'])
def test_frozen_W(dev, kind):
    m, _, _, _ = _model(kind, dev)
    gh = _grads(m)[0].clone()
    frozen, _, _, _ = _model(kind, dev, trainable_W=False)
    gh_frozen, gw_frozen = _grads(frozen)
    assert gw_frozen is None and frozen.W.grad is None
    assert torch.equal(gh_frozen, gh)


def test_non_leaf_H(dev):
    m, H0, _, _ = _model('NMFD', dev)
    leaf = (H0 - 0.5).to(dev).requires_grad_()
    h = F.softplus(leaf)
    seen = []
    h.register_hook(seen.append)
    out = m(H=h)
    assert out._nmf_source[1] is h
    up = _fixed_upstream(out)
    (out * up).sum().backward()
    assert m.H.grad is None and leaf.grad is not None and len(seen) == 1
    # what reached h is the kernel's grad_H for these factors ...
    direct = h.detach().clone().requires_grad_()
    (m(H=direct) * up).sum().backward()
    assert torch.equal(seen[0], direct.grad)
    # ... and torch carried it on to the leaf
    leaf2 = leaf.detach().clone().requires_grad_()
    expect, = torch.autograd.grad(F.softplus(leaf2), leaf2, seen[0])
    assert torch.equal(leaf.grad, expect) and bool((leaf.grad != 0).any())


def test_double_module(dev):
    m, _, _, _ = _model('NMF2D', dev)
    gh, gw = (t.clone() for t in _grads(m))
    m64, _, _, _ = _model('NMF2D', dev)
    m64 = m64.double()
    gh64, gw64 = _grads(m64)
    assert gh64.dtype == torch.float64 and gw64.dtype == torch.float64
    assert torch.equal(gh64, gh.double()) and torch.equal(gw64, gw.double())


@pytest.mark.parametrize('kind', ['NMFD', 'NMF3D'])
def test_non_contiguous_upstream(dev, kind):
    m, _, _, _ = _model(kind, dev)
    gh, gw = (t.clone() for t in _grads(m))
    m.zero_grad()
    out = m()
    up_t = _fixed_upstream(out).transpose(-1, -2).contiguous()
    seen = []
    out.register_hook(seen.append)
    (out.transpose(-1, -2) * up_t).sum().backward()
    assert not seen[0].is_contiguous()
    assert torch.equal(m.H.grad, gh) and torch.equal(m.W.grad, gw)


@pytest.mark.parametrize('kind', ['NMFD', 'NMF2D', 'NMF3D'])
def test_no_grad_records_nothing(dev, kind):
    m, _, _, _ = _model(kind, dev)
    with torch.no_grad():
        out = m()
    assert out.grad_fn is None and not out.requires_grad and out._nmf_source[0] is m


def test_sgd_steps_lower_the_loss(dev):
    from torchnmf_amd.metrics import euclidean
    m, _, _, V = _model('NMFD', dev)
    Vd = V.to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = euclidean(m(), Vd)
        loss.backward()
        opt.step()
        with torch.no_grad():
            for p in m.parameters():
                p.clamp_(min=0)                       # plain gradient steps do not keep the factors non-negative
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(euclidean(m(), Vd)))
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2], losses
    assert bool((m.W >= 0).all()) and bool((m.H >= 0).all())
