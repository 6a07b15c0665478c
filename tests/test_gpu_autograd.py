"""torch.autograd through NMF.forward and the divergences: the HIP backward kernels per element, then end to end.

References are computed here on the CPU in float64 with plain torch (closed-form products, or torch.autograd on float64
leaves); every element of every output is compared.  u = 2^-24 throughout.

1. ``nmfmu_reconstruct_backward`` through the C ABI: ``|got - ref64| <= (K + 2) u (|G| |B|)`` per element, K the contraction
   length -- the standard bound of an fp32 dot product, which holds for any summation order and so covers the MFMA's
   order, the split of the contraction and the slab sum.
2. The same launch twice gives ``torch.equal`` gradients (no floating-point atomics).
3. ``nmfmu_beta_div_grad``: beta = 2 bit-equal to fp32 ``upstream * (x - y)``; the other beta within
   ``TOL_GRAD (|term1| + |term2|)`` of float64 per element.
4. End to end: ``beta_div(m(), V, beta).backward()`` against float64 autograd under the two bounds composed
   (``_single_layer_bounds``), against ``BetaMu``'s ``p.grad``, through a two-layer chain, with a frozen factor, leading
   dimensions, a float64 module, three SGD steps, ``torch.no_grad()`` and the bit-equality of ``m()``.
"""
import ctypes

import pytest
import torch

from conftest import record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = torch.finfo(torch.float32).eps
# Measured on the inputs of test 3: torch's own fp32 CPU autograd of the reference's formula (metrics.py:6-96) against
# float64 is off by at most 1.68e-7 (|term1| + |term2|) (2.82 u; beta = 3 with exact zeros; 1.61e-7 at beta = 1.5).
# 4 x that, floor 2^-22 = 2.38e-7:
TOL_GRAD = max(4 * 1.6812647723219986e-07, 2.0 ** -22)

SHAPES = [(1, 1, 1), (33, 130, 7), (128, 128, 32), (300, 257, 33), (513, 1000, 128), (200, 90, 256)]
# chosen from the split rule (include/nmfmu.h): both contractions in >= 3 parts, the last part short
SPLIT_SHAPES = [(1000, 1100, 7), (700, 650, 130)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _splits(m, k, rank, want_owner=True, want_panel=True):
    from torchnmf_amd import _capi
    s = (ctypes.c_int * 2)()
    n = _capi.load().nmfmu_reconstruct_backward_ws(m, k, rank, int(want_owner), int(want_panel), s)
    return n, s[0], s[1]


def _backward(G, owner, panel, want_owner=True, want_panel=True):
    """nmfmu_reconstruct_backward on device tensors; G may be a column slice (its row stride is passed as ld).  Outputs
    and scratch start as NaN, so an element nobody wrote cannot pass."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    m, k = G.shape
    rank = owner.shape[1]
    assert G.stride(1) == 1 and owner.is_contiguous() and panel.is_contiguous()
    n_ws, _, _ = _splits(m, k, rank, want_owner, want_panel)
    ws = torch.full((max(n_ws, 1),), float('nan'), device=G.device)
    go = torch.full((m, rank), float('nan'), device=G.device) if want_owner else None
    gp = torch.full((k, rank), float('nan'), device=G.device) if want_panel else None
    _capi.check(lib.nmfmu_reconstruct_backward(G.data_ptr(), G.stride(0) if m > 1 else k, m, k, owner.data_ptr(),
                                               panel.data_ptr(), rank, go.data_ptr() if want_owner else None,
                                               gp.data_ptr() if want_panel else None, ws.data_ptr() if n_ws else None,
                                               _stream()), 'nmfmu_reconstruct_backward')
    torch.cuda.synchronize()
    return go, gp


_cases = {}


def _case(shape):
    """Inputs and float64 references of one shape, computed once and shared."""
    if shape not in _cases:
        m, k, rank = shape
        g = torch.Generator().manual_seed(m * 7 + k * 3 + rank)
        G = torch.randn(m, k, generator=g)
        owner, panel = torch.rand(m, rank, generator=g), torch.rand(k, rank, generator=g)
        G64, o64, p64 = G.double(), owner.double(), panel.double()
        _cases[shape] = dict(G=G, owner=owner, panel=panel,
                             ref_o=G64 @ p64, bound_o=(k + 2) * U * (G64.abs() @ p64),
                             ref_p=G64.t() @ o64, bound_p=(m + 2) * U * (G64.abs().t() @ o64))
    return _cases[shape]


def _check_backward(name, shape, go, gp, c):
    for tag, got, ref, bound in (('owner', go, c['ref_o'], c['bound_o']), ('panel', gp, c['ref_p'], c['bound_p'])):
        if got is None:
            continue
        got = got.double().cpu()
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (shape, tag)
        frac = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
        record(name, shape=list(shape), output=tag, worst_fraction_of_bound=frac)
        print(f'{name} {shape} grad_{tag}: worst |got - ref| / bound = {frac:.3f}')
        assert bool(((got - ref).abs() <= bound).all()), (shape, tag, frac)


@pytest.mark.parametrize('shape', SHAPES + SPLIT_SHAPES)
def test_backward_kernel_per_element(dev, shape):
    c = _case(shape)
    m, k, rank = shape
    if shape in SPLIT_SHAPES:
        _, so, sp = _splits(m, k, rank)
        assert so >= 3 and sp >= 3, (so, sp)
        for contraction, parts in ((k, so), (m, sp)):        # the rule: parts of ceil(stages / parts) * 32 steps
            stages = -(-contraction // 32)
            part_len = -(-stages // parts) * 32
            assert contraction % part_len != 0 and (parts - 1) * part_len < contraction < parts * part_len
    go, gp = _backward(c['G'].to(dev), c['owner'].to(dev), c['panel'].to(dev))
    _check_backward('reconstruct_backward', shape, go, gp, c)


@pytest.mark.parametrize('offset,extra', [(5, 11), (4, 12)])
def test_backward_kernel_strided_gradient(dev, offset, extra):
    """ld > k: G is a column slice of a wider buffer (offset 5: rows off the 16-byte grid, scalar loads; offset 4 of a
    buffer whose width is a multiple of 4: 16-byte loads); what lies around the slice is NaN."""
    shape = (300, 257, 33)
    c = _case(shape)
    m, k, _ = shape
    width = k + extra + (-(k + extra) % 4 if offset % 4 == 0 else 0)
    wide = torch.full((m, width), float('nan'), device=dev)
    wide[:, offset:offset + k] = c['G'].to(dev)
    G = wide[:, offset:offset + k]
    assert G.stride(0) == width > k
    go, gp = _backward(G, c['owner'].to(dev), c['panel'].to(dev))
    _check_backward('reconstruct_backward_ld', shape, go, gp, c)
    go2, gp2 = _backward(c['G'].to(dev), c['owner'].to(dev), c['panel'].to(dev))
    assert torch.equal(go, go2) and torch.equal(gp, gp2)       # the same arithmetic whatever the load width


@pytest.mark.parametrize('shape', [(300, 257, 33), (1000, 1100, 7)])
def test_backward_kernel_one_output(dev, shape):
    """Either output NULL: the other one is bit-equal to the both-outputs call (and, the scratch being NaN, does not
    depend on the slab of the half that was left out)."""
    c = _case(shape)
    G, owner, panel = c['G'].to(dev), c['owner'].to(dev), c['panel'].to(dev)
    go, gp = _backward(G, owner, panel)
    go1, none_p = _backward(G, owner, panel, want_panel=False)
    none_o, gp1 = _backward(G, owner, panel, want_owner=False)
    assert none_p is None and none_o is None
    assert torch.equal(go, go1) and torch.equal(gp, gp1)
    n_both, n_o, n_p = _splits(*shape)[0], _splits(*shape, want_panel=False)[0], _splits(*shape, want_owner=False)[0]
    assert n_both == n_o + n_p


@pytest.mark.parametrize('shape', [(513, 1000, 128), (700, 650, 130)])
def test_backward_kernel_deterministic(dev, shape):
    c = _case(shape)
    G, owner, panel = c['G'].to(dev), c['owner'].to(dev), c['panel'].to(dev)
    go, gp = _backward(G, owner, panel)
    go2, gp2 = _backward(G, owner, panel)
    assert torch.equal(go, go2) and torch.equal(gp, gp2)


# ---- the divergence gradient ---------------------------------------------------------------------------------------
def _terms64(x, y, beta):
    """(term1, term2) of d beta_div / d x = term1 - term2 in float64 (metrics.py:6-96 differentiated, eps as there)."""
    s = x + EPS
    if beta == 2:
        return x, y
    if beta == 1:
        return torch.ones_like(x), y / s
    if beta == 0:
        return 1 / s, (y + EPS) / s ** 2
    yb = y + EPS if beta < 0 else y
    return s ** (beta - 1), yb * s ** (beta - 2)


def _div_inputs(zeros):
    g = torch.Generator().manual_seed(1000)
    x = torch.rand(1000, generator=g) * 0.99 + 0.01
    y = torch.rand(1000, generator=g) * 0.99 + 0.01
    if zeros:
        x[::7] = 0
        y[3::5] = 0
    return x, y


@pytest.mark.parametrize('beta,zeros', [(b, False) for b in (-1, 0, 0.5, 1, 1.5, 2, 3)] + [(b, True) for b in (1, 1.5, 2, 3)])
def test_beta_div_grad_per_element(dev, beta, zeros):
    from torchnmf_amd import _capi
    lib = _capi.load()
    x, y = _div_inputs(zeros)
    up = torch.tensor([0.75 if beta == 2 else 1.0])
    xd, yd, upd = x.to(dev), y.to(dev), up.to(dev)
    gx = torch.full((1000,), float('nan'), device=dev)
    _capi.check(lib.nmfmu_beta_div_grad(xd.data_ptr(), yd.data_ptr(), 1000, float(beta), upd.data_ptr(), gx.data_ptr(),
                                        _stream()), 'nmfmu_beta_div_grad')
    got = gx.cpu()
    if beta == 2:
        assert torch.equal(got, up * (x - y))
        return
    t1, t2 = _terms64(x.double(), y.double(), beta)
    err = (got.double() - (t1 - t2)).abs() / (t1.abs() + t2.abs())
    record('beta_div_grad', beta=beta, zeros=zeros, worst=float(err.max()), tol=TOL_GRAD)
    print(f'beta_div_grad beta={beta} zeros={zeros}: worst error {float(err.max()):.3e} (|t1| + |t2|), tol {TOL_GRAD:.3e}')
    assert bool(torch.isfinite(got).all()) and bool((err <= TOL_GRAD).all()), (beta, zeros, float(err.max()))


# ---- end to end -----------------------------------------------------------------------------------------------------
def _ref_beta_div(x, y, beta):
    """The reference's metrics.beta_div (metrics.py:6-96) in plain torch, for float64 autograd."""
    if beta == 2:
        return 0.5 * ((x - y) ** 2).sum()
    if beta == 1:
        return y.reshape(-1) @ ((y + EPS).log() - (x + EPS).log()).reshape(-1) - y.sum() + x.sum()
    if beta == 0:
        return ((y + EPS) / (x + EPS)).sum() - (y + EPS).log().sum() + (x + EPS).log().sum() - y.numel()
    i, t = x.reshape(-1) + EPS, y.reshape(-1)
    if beta < 0:
        t = t + EPS
    return (t.pow(beta).sum() + (beta - 1) * i.pow(beta).sum() - beta * (t @ i.pow(beta - 1))) / (beta * (beta - 1))


def _single_layer_bounds(H, W, V, beta):
    """float64 gradients of beta_div(H W^T, V) and the per-element bounds of tests 1 and 3 composed, to first order:
      dS = (R + 2) u |H| |W|^T                            the fp32 reconstruction (a dot product of length R)
      dG = TOL_GRAD (|t1| + |t2|) + 2 |l''(S)| dS         test 3's bound, plus the gradient's sensitivity to S; the factor 2
                                                          covers the higher-order terms (dS / S is of order 1e-6) and the
                                                          terms being evaluated at the exact S here
      d grad = (K + 2) u (|G| + dG) |B| + dG |B|          test 1's bound on the perturbed G, plus the perturbation itself
    H may have leading dimensions; they are flattened (grad_W sums over all of them)."""
    R = H.shape[-1]
    H64, W64, V64 = H.double().reshape(-1, R), W.double(), V.double().reshape(-1, W.shape[0])
    S = H64 @ W64.t()
    t1, t2 = _terms64(S, V64, beta)
    G = t1 - t2
    s = S + EPS
    if beta == 2:
        curv = torch.ones_like(S)
    elif beta == 1:
        curv = V64 / s ** 2
    else:
        curv = abs(beta - 1) * s ** (beta - 2) + abs(beta - 2) * V64 * s ** (beta - 3)
    dS = (R + 2) * U * S
    dG = TOL_GRAD * (t1.abs() + t2.abs()) + 2 * curv * dS
    Gb = G.abs() + dG
    N, C = S.shape
    gH, bH = G @ W64, (C + 2) * U * (Gb @ W64) + dG @ W64
    gW, bW = G.t() @ H64, (N + 2) * U * (Gb.t() @ H64) + dG.t() @ H64
    return gH.reshape(H.shape), bH.reshape(H.shape), gW, bW


def _assert_within(name, got, ref, bound, **info):
    got = got.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (name, info)
    frac = float(((got - ref).abs() / bound).max())
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert bool(((got - ref).abs() <= bound).all()), (name, info, frac)


def _factors(shape_h=(70, 5), C=90, seed=5):
    g = torch.Generator().manual_seed(seed)
    H0 = torch.rand(*shape_h, generator=g) + 0.05
    W0 = torch.rand(C, shape_h[-1], generator=g) + 0.05
    V = torch.rand(*shape_h[:-1], C, generator=g) + 1e-3
    return H0, W0, V


@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_backward_end_to_end(dev, beta):
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import BetaMu
    H0, W0, V = _factors()
    m = NMF(W=W0, H=H0).to(dev)
    Vd = V.to(dev)
    pred = m()
    assert pred.requires_grad and pred.grad_fn is not None
    loss = beta_div(pred, Vd, beta)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert float(loss.detach()) == pytest.approx(float(_ref_beta_div(H0.double() @ W0.double().t(), V.double(), beta)), rel=1e-5)
    loss.backward()
    gH, bH, gW, bW = _single_layer_bounds(H0, W0, V, beta)
    assert m.H.grad.dtype == torch.float32 and m.W.grad.dtype == torch.float32
    _assert_within('autograd_end_to_end', m.H.grad, gH, bH, beta=beta, param='H')
    _assert_within('autograd_end_to_end', m.W.grad, gW, bW, beta=beta, param='W')
    # float64 autograd itself agrees with the closed form used for the bounds
    Hl, Wl = H0.double().requires_grad_(), W0.double().requires_grad_()
    _ref_beta_div(Hl @ Wl.t(), V.double(), beta).backward()
    assert torch.allclose(Hl.grad, gH, rtol=1e-9, atol=1e-12) and torch.allclose(Wl.grad, gW, rtol=1e-9, atol=1e-12)
    # ... and with what BetaMu.step leaves in p.grad at the same point (tolerance of test_betamu_grad_is_beta_div_gradient)
    for attr in ('W', 'H'):
        m2 = NMF(W=W0, H=H0).to(dev)
        trainer = BetaMu([getattr(m2, attr)], beta, precision='bf16x3')

        def closure():
            trainer.zero_grad()
            return Vd, m2
        trainer.step(closure)
        mine, theirs = getattr(m, attr).grad.cpu(), getattr(m2, attr).grad.cpu()
        scale = float(theirs.abs().max())
        assert float((mine - theirs).abs().max()) < 1e-4 * max(scale, 1.0) * 50, (beta, attr)


def test_backward_through_a_chain(dev):
    """nn.Sequential of two layers: the gradient reaches the first layer's factors through the second layer's grad_H.
    beta = 2, G = S - V.  Every product of the forward and backward pass is a non-negative matrix times (a perturbation
    of) S, V or G, so to first order each gradient is within c u of the same chain of products evaluated on S + V in place
    of G, with c the sum of (length + 2) over the contractions that feed it; c below counts every contraction of both
    passes twice."""
    from torch import nn
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    N, R1, C1, C2 = 70, 5, 20, 90
    g = torch.Generator().manual_seed(11)
    H1, W1, W2 = torch.rand(N, R1, generator=g), torch.rand(C1, R1, generator=g), torch.rand(C2, C1, generator=g)
    V = torch.rand(N, C2, generator=g)
    chain = nn.Sequential(NMF(W=W1, H=H1), NMF(W=W2)).to(dev)
    beta_div(chain(None), V.to(dev), 2).backward()
    leaves = [t.double().requires_grad_() for t in (H1, W1, W2)]
    _ref_beta_div(leaves[0] @ leaves[1].t() @ leaves[2].t(), V.double(), 2).backward()
    H64, W164, W264 = H1.double(), W1.double(), W2.double()
    X1 = H64 @ W164.t()
    A = X1 @ W264.t() + V.double()                      # |G| <= S + V
    c = 2 * ((R1 + 2) + (C1 + 2) + (N + 2) + (C2 + 2)) + 2
    scale = {'H': (A @ W264) @ W164, 'W1': (A @ W264).t() @ H64, 'W2': A.t() @ X1}
    for name, p, leaf in (('H', chain[0].H, leaves[0]), ('W1', chain[0].W, leaves[1]), ('W2', chain[1].W, leaves[2])):
        assert p.grad is not None, name
        _assert_within('autograd_chain', p.grad, leaf.grad, c * U * scale[name], param=name)


def test_backward_frozen_factor(dev):
    from torchnmf_amd.metrics import kl_div
    from torchnmf_amd.nmf import NMF
    H0, W0, V = _factors()
    m = NMF(W=W0, H=H0, trainable_W=False).to(dev)
    kl_div(m(), V.to(dev)).backward()
    assert m.W.grad is None
    gH, bH, _, _ = _single_layer_bounds(H0, W0, V, 1)
    _assert_within('autograd_frozen_W', m.H.grad, gH, bH, param='H')


def test_backward_leading_dimensions(dev):
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    H0, W0, V = _factors(shape_h=(3, 40, 5), C=33, seed=9)
    H = H0.to(dev).requires_grad_()
    W = W0.to(dev).requires_grad_()
    out = NMF.reconstruct(H, W)
    assert out.shape == (3, 40, 33)
    beta_div(out, V.to(dev), 1).backward()
    gH, bH, gW, bW = _single_layer_bounds(H0, W0, V, 1)
    assert H.grad.shape == (3, 40, 5) and W.grad.shape == (33, 5)
    _assert_within('autograd_leading_dims', H.grad, gH, bH, param='H')
    _assert_within('autograd_leading_dims', W.grad, gW, bW, param='W')


def test_backward_double_module(dev):
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    H0, W0, V = _factors()
    m = NMF(W=W0, H=H0).double().to(dev)
    beta_div(m(), V.double().to(dev), 2).backward()
    assert m.W.grad.dtype == torch.float64 and m.H.grad.dtype == torch.float64
    gH, bH, gW, bW = _single_layer_bounds(H0, W0, V, 2)
    _assert_within('autograd_double', m.H.grad, gH, bH, param='H')
    _assert_within('autograd_double', m.W.grad, gW, bW, param='W')


def test_sgd_steps_lower_the_loss(dev):
    from torchnmf_amd.metrics import euclidean
    from torchnmf_amd.nmf import NMF
    H0, W0, V = _factors()
    m = NMF(W=W0, H=H0).to(dev)
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
    assert losses[3] < losses[0], losses
    assert bool((m.W >= 0).all()) and bool((m.H >= 0).all())


def test_no_grad_records_nothing_and_forward_is_unchanged(dev):
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    H0, W0, V = _factors()
    m = NMF(W=W0, H=H0).to(dev)
    with torch.no_grad():
        y = m()
        assert not y.requires_grad and y.grad_fn is None
        assert not beta_div(y, V.to(dev), 1).requires_grad
    out = m()
    assert out.requires_grad and out._nmf_source[0] is m
    assert torch.equal(out.detach(), NMF.reconstruct(m.H.detach(), m.W.detach()))
    assert torch.equal(out.detach(), y)
    # a prediction that does not require grad gives a plain value, and the value is the same launch either way
    plain = beta_div(out.detach(), V.to(dev), 1)
    assert not plain.requires_grad and torch.equal(plain, beta_div(out, V.to(dev), 1).detach())
