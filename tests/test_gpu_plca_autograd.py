"""torch.autograd through PLCA / SIPLCA / SIPLCA2 / SIPLCA3.forward: ``nmfmu_plca_backward`` and ``nmfmu_conv_plca_backward`` per
element, then end to end.

References are float64, computed here on the CPU (plca_autograd_reference.py: the unscaled products ``rawH``, ``rawW`` of the
upstream gradient ``G`` with the factors, then ``grad_H = Z rawH``, ``grad_W = Z rawW``, ``grad_Z[r] = sum rawW W``); every element
of every output is compared.  u = 2^-24, K = the product's contraction length (dense: C for grad_H, N for grad_W;
shift-invariant: C prod(T) and B prod(Lh)), P = the number of terms of the Z dot product.  First-order bounds, valid for any
summation order -- the MFMA's, the split of the contraction, the order the parts and the workgroups' partial sums are added in:

    |grad_F - ref|   <= (K + 3) u |Z[r]| (|G| . |F'|)          the (K + 2) u of the NMF backward + the one rounding of the scale
    |grad_Z[r] - ref| <= (K + P + 3) u sum (|G| . |F'|) |F|     K + P = C prod(T) + B prod(Lh) whichever half it comes from

``G`` is ``randn`` (signed), the factors are ``rand``, ``Z`` has one exact zero (its gradients' bound is zero there), seeds are
fixed; outputs and scratch start as NaN, so an element nobody wrote cannot pass.

1. Through the C ABI: the dense and the shift-invariant shapes, every code path of the finishing kernel (16-byte and scalar
   accesses, several rank passes, inner segments), split contractions with a short last part.
2. All seven non-empty subsets of {grad_h, grad_w, grad_z}: an output is ``torch.equal`` to the all-outputs call when it comes
   from the same half by the rule of include/nmfmu.h (grad_z with grad_h and without grad_w comes from the H half: bound only);
   the same call twice is ``torch.equal``.
3. End to end for the four classes at beta 1 and 2 through ``kl_div`` / ``beta_div`` with ``norm``: ``out`` is bit-equal to the
   ``no_grad`` forward; the device's own upstream gradient is captured where it enters the backward and the three ``.grad`` are
   compared, under the bounds above, with the float64 formulas of that captured ``G``.
4. Surface: frozen W (grad_Z from the H half), frozen Z, a float64 module, a non-contiguous upstream gradient, ``no_grad``,
   ``fit()`` recording nothing, SGD steps.
5. Golden g18: the reference's own float64 gradients (tools/make_golden_plca_autograd.py) under the same bounds.
"""
import ctypes

import pytest
import torch

from conftest import load_golden, record
from plca_autograd_reference import reference

pytestmark = pytest.mark.gpu

# (m, k, rank): sizes off every tile; rank 256 > the 128-wide rank tile; ranks 259 / 1028 take two rank passes of the finishing
# kernel (scalar: 256 ranks per pass, 16-byte: 1024)
DENSE = [(33, 130, 7), (300, 257, 33), (200, 90, 256), (20, 30, 259), (12, 9, 1028)]
# from the split rule (include/nmfmu.h): 1000 / 1100 at rank 7 gives 7 and 8 parts, 700 / 650 at rank 130 gives 5 and 5
DENSE_SPLIT = [(1000, 1100, 7), (700, 650, 130)]
# (B, C, R, lh, taps); the last two cut H's lines into two inner segments (16-byte and scalar)
CONV = [(2, 33, 7, (50,), (5,)), (1, 130, 4, (33, 40), (5, 2)), (2, 33, 2, (3, 9, 8), (3, 1, 4)), (1, 3, 2, (4500,), (2,)),
        (1, 2, 2, (4501,), (3,))]
CONV_SPLIT = [(2, 55, 7, (500,), (20,)), (1, 13, 130, (20, 35), (5, 10))]
SUBSETS = [(h, w, z) for h in (1, 0) for w in (1, 0) for z in (1, 0) if h or w or z]


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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(shape, wants=(1, 1, 1)):
    from torchnmf_amd import _capi
    info = (ctypes.c_int * 5)()
    if len(shape) == 3:
        n = _capi.load().nmfmu_plca_backward_ws(*shape, *wants, info)
    else:
        B, C, R, lh, taps = shape
        n = _capi.load().nmfmu_conv_plca_backward_ws(B, C, R, len(lh), _arr(lh), _arr(taps), *wants, info)
    assert n >= 0, n
    return n, list(info)


_cases = {}


def _case(shape):
    """Inputs and float64 references of one shape, computed once and shared."""
    if shape not in _cases:
        g = torch.Generator().manual_seed(sum(shape[:3]) + (0 if len(shape) == 3 else 11 * _prod(shape[3]) + 13 * _prod(shape[4])))
        if len(shape) == 3:
            m, k, R = shape
            G, H, W = torch.randn(m, k, generator=g), torch.rand(m, R, generator=g), torch.rand(k, R, generator=g)
        else:
            B, C, R, lh, taps = shape
            G = torch.randn(B, C, *(a + t - 1 for a, t in zip(lh, taps)), generator=g)
            H, W = torch.rand(B, R, *lh, generator=g), torch.rand(C, R, *taps, generator=g)
        Z = torch.rand(R, generator=g) + 0.05
        Z[R // 2] = 0.0
        _cases[shape] = dict(G=G, H=H, W=W, Z=Z, ref=reference(G, H, W, Z))
    return _cases[shape]


def _backward(shape, c, dev, wants=(1, 1, 1)):
    """The C ABI entry on device copies of the case; outputs and scratch start as NaN.  Dense: G is an unaligned slice of a
    NaN-filled buffer (ld = k + 5, 12 bytes off a 16-byte boundary)."""
    from torchnmf_amd import _capi
    lib = _capi.load()
    H, W, Z = c['H'].to(dev), c['W'].to(dev), c['Z'].to(dev)
    n_ws, _ = _ws(shape, wants)
    ws = torch.full((max(n_ws, 1),), float('nan'), device=dev)
    gh = torch.full_like(H, float('nan')) if wants[0] else None
    gw = torch.full_like(W, float('nan')) if wants[1] else None
    gz = torch.full_like(Z, float('nan')) if wants[2] else None
    stream = torch.cuda.current_stream().cuda_stream
    if len(shape) == 3:
        m, k, R = shape
        buf = torch.full((m, k + 5), float('nan'), device=dev)
        G = buf[:, 3:3 + k]
        G.copy_(c['G'])
        assert G.stride(0) == k + 5 and G.data_ptr() % 16 == 12
        _capi.check(lib.nmfmu_plca_backward(G.data_ptr(), G.stride(0), m, k, H.data_ptr(), W.data_ptr(), Z.data_ptr(), R,
                                            _ptr(gh), _ptr(gw), _ptr(gz), ws.data_ptr() if n_ws else None, stream),
                    'nmfmu_plca_backward')
    else:
        B, C, R, lh, taps = shape
        G = c['G'].to(dev)
        _capi.check(lib.nmfmu_conv_plca_backward(G.data_ptr(), W.data_ptr(), H.data_ptr(), Z.data_ptr(), B, C, R, len(lh),
                                                 _arr(lh), _arr(taps), _ptr(gh), _ptr(gw), _ptr(gz),
                                                 ws.data_ptr() if n_ws else None, stream), 'nmfmu_conv_plca_backward')
    torch.cuda.synchronize()
    return gh, gw, gz


def _check(name, tag, what, got, ref, bound):
    got = got.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (what, tag)
    err = (got - ref).abs()
    frac = float((err / bound.clamp_min(1e-300)).max())
    record(name, case=str(what), output=tag, worst_fraction_of_bound=frac)
    print(f'{name} {what} grad_{tag}: worst |got - ref| / bound = {frac:.3f}')
    assert bool((err <= bound).all()), (what, tag, frac)


def _check_all(name, what, ref, gh, gw, gz):
    if gh is not None:
        _check(name, 'H', what, gh, ref['gH'], ref['bH'])
    if gw is not None:
        _check(name, 'W', what, gw, ref['gW'], ref['bW'])
    if gz is not None:
        _check(name, 'Z', what, gz, ref['gZ'], ref['bZ'])


def _assert_split(shape, rows, contraction):
    """>= 3 parts on both halves, the last part short (the rule of nmfmu_reconstruct_backward)."""
    _, info = _ws(shape)
    assert info[0] >= 3 and info[1] >= 3, info
    for c_len, parts in ((contraction, info[0]), (rows, info[1])):
        part_len = -(-(-(-c_len // 32)) // parts) * 32
        assert c_len % part_len != 0 and (parts - 1) * part_len < c_len < parts * part_len


@pytest.mark.parametrize('shape', DENSE + DENSE_SPLIT)
def test_dense_per_element(dev, shape):
    c = _case(shape)
    if shape in DENSE_SPLIT:
        _assert_split(shape, shape[0], shape[1])
    gh, gw, gz = _backward(shape, c, dev)
    zero = shape[2] // 2
    assert bool((gh[:, zero] == 0).all()) and bool((gw[:, zero] == 0).all())
    _check_all('plca_backward', shape, c['ref'], gh, gw, gz)


@pytest.mark.parametrize('shape', CONV + CONV_SPLIT)
def test_conv_per_element(dev, shape):
    c = _case(shape)
    B, C, R, lh, taps = shape
    if shape in CONV_SPLIT:
        _assert_split(shape, B * _prod(lh), C * _prod(taps))
    if shape in CONV[-2:]:
        assert _ws(shape)[1][2] == 2                          # H's lines in two inner segments
    gh, gw, gz = _backward(shape, c, dev)
    assert bool((gh[:, R // 2] == 0).all()) and bool((gw[:, R // 2] == 0).all())
    _check_all('conv_plca_backward', shape, c['ref'], gh, gw, gz)


@pytest.mark.parametrize('shape', [DENSE_SPLIT[0], CONV_SPLIT[0]])
def test_output_subsets_and_determinism(dev, shape):
    c = _case(shape)
    full = _backward(shape, c, dev)
    again = _backward(shape, c, dev)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert _ws(shape)[1][4] == 2                              # all outputs: grad_z from the W half
    for wants in SUBSETS:
        got = _backward(shape, c, dev, wants)
        z_half = _ws(shape, wants)[1][4]
        assert z_half == (0 if not wants[2] else 1 if wants[0] and not wants[1] else 2)
        for idx, (g, f) in enumerate(zip(got, full)):
            assert (g is not None) == bool(wants[idx])
        if wants[0]:
            assert torch.equal(got[0], full[0]), wants
        if wants[1]:
            assert torch.equal(got[1], full[1]), wants
        if wants[2] and z_half == 2:
            assert torch.equal(got[2], full[2]), wants
        elif wants[2]:
            _check('plca_backward_subsets', 'Z', (shape, wants), got[2], c['ref']['gZ'], c['ref']['bZ'])
            assert torch.equal(got[2], _backward(shape, c, dev, wants)[2])


# ---- end to end -----------------------------------------------------------------------------------------------------
# (class name, H shape, W shape): B = 2, odd channel counts, sizes off every tile
MODELS = {'PLCA': ((37, 5), (21, 5)), 'SIPLCA': ((2, 3, 21), (9, 3, 5)), 'SIPLCA2': ((2, 3, 7, 9), (9, 3, 2, 3)),
          'SIPLCA3': ((2, 2, 4, 5, 6), (5, 2, 2, 3, 2))}


def _model(kind, dev, seed=5, **kw):
    from torchnmf_amd import plca
    hs, ws = MODELS[kind]
    g = torch.Generator().manual_seed(seed)
    H0, W0, Z0 = torch.rand(*hs, generator=g) + 0.1, torch.rand(*ws, generator=g) + 0.1, torch.rand(hs[1], generator=g) + 0.1
    out_shape = (hs[0], ws[0]) + tuple(a + t - 1 for a, t in zip(hs[2:], ws[2:]))
    V = torch.rand(*out_shape, generator=g) * 5 + 0.5
    return getattr(plca, kind)(W=W0, H=H0, Z=Z0, **kw).to(dev), V


def _capture_upstream(out, seen):
    """Record the gradient that enters the reconstruction's backward node (below the ``* norm`` of ``forward``)."""
    todo, found = [out.grad_fn], []
    while todo:
        node = todo.pop()
        if 'PlcaReconstructFn' in node.name():
            found.append(node)
            continue
        todo += [n for n, _ in node.next_functions if n is not None]
    assert len(found) == 1, [n.name() for n in found]
    found[0].register_prehook(lambda grads: seen.append(grads[0]))


@pytest.mark.parametrize('beta', [1, 2])
@pytest.mark.parametrize('kind', list(MODELS))
def test_end_to_end(dev, kind, beta):
    from torchnmf_amd.metrics import beta_div, kl_div
    m, V = _model(kind, dev)
    Vd = V.to(dev)
    norm = Vd.sum()
    with torch.no_grad():
        plain = m(norm=norm)
    assert plain.grad_fn is None
    out = m(norm=norm)
    assert out.grad_fn is not None and not hasattr(out, '_nmf_source')
    assert torch.equal(out.detach(), plain)
    seen = []
    _capture_upstream(out, seen)
    (kl_div(out, Vd) if beta == 1 else beta_div(out, Vd, beta)).backward()
    assert len(seen) == 1 and seen[0].shape == out.shape
    ref = reference(seen[0].cpu(), m.H.detach().cpu(), m.W.detach().cpu(), m.Z.detach().cpu())
    for p in (m.H, m.W, m.Z):
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype
    _check_all('plca_autograd_end_to_end', (kind, beta), ref, m.H.grad, m.W.grad, m.Z.grad)


def _fixed_upstream(out, seed=9):
    return torch.randn(*out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)


def _grads(m, upstream=None):
    """(H.grad, W.grad, Z.grad) of sum(m() * upstream) with a fixed upstream gradient."""
    m.zero_grad()
    out = m()
    up = _fixed_upstream(out) if upstream is None else upstream
    (out * up).sum().backward()
    return m.H.grad, m.W.grad, m.Z.grad


@pytest.mark.parametrize('kind', ['PLCA', 'SIPLCA2'])
def test_frozen_W(dev, kind):
    """No grad_W: grad_H is the same launch; grad_Z comes from the H half (another summation, the same bound)."""
    m, _ = _model(kind, dev)
    gh, _, gz = (t.clone() for t in _grads(m))
    frozen, _ = _model(kind, dev, trainable_W=False)
    gh_f, gw_f, gz_f = _grads(frozen)
    assert gw_f is None and frozen.W.grad is None
    assert torch.equal(gh_f, gh)
    out = frozen()
    ref = reference(_fixed_upstream(out).cpu(), frozen.H.detach().cpu(), frozen.W.detach().cpu(), frozen.Z.detach().cpu())
    _check('plca_autograd_frozen_W', 'Z', kind, gz_f, ref['gZ'], ref['bZ'])
    _check('plca_autograd_frozen_W', 'Z', (kind, 'trainable W'), gz, ref['gZ'], ref['bZ'])


@pytest.mark.parametrize('kind', ['PLCA', 'SIPLCA'])
def test_frozen_Z(dev, kind):
    m, _ = _model(kind, dev)
    gh, gw, _ = (t.clone() for t in _grads(m))
    frozen, _ = _model(kind, dev, trainable_Z=False)
    gh_f, gw_f, gz_f = _grads(frozen)
    assert gz_f is None and frozen.Z.grad is None
    assert torch.equal(gh_f, gh) and torch.equal(gw_f, gw)


@pytest.mark.parametrize('kind', ['PLCA', 'SIPLCA3'])
def test_double_module(dev, kind):
    m, _ = _model(kind, dev)
    g32 = [t.clone() for t in _grads(m)]
    m64, _ = _model(kind, dev)
    m64 = m64.double()
    g64 = _grads(m64)
    for a, b in zip(g64, g32):
        assert a.dtype == torch.float64 and torch.equal(a, b.double())


@pytest.mark.parametrize('kind', ['PLCA', 'SIPLCA', 'SIPLCA3'])
def test_non_contiguous_upstream(dev, kind):
    m, _ = _model(kind, dev)
    want = [t.clone() for t in _grads(m)]
    m.zero_grad()
    out = m()
    up_t = _fixed_upstream(out).transpose(-1, -2).contiguous()
    seen = []
    _capture_upstream(out, seen)
    (out.transpose(-1, -2) * up_t).sum().backward()
    assert not seen[0].is_contiguous()
    assert all(torch.equal(p.grad, w) for p, w in zip((m.H, m.W, m.Z), want))


@pytest.mark.parametrize('kind', list(MODELS))
def test_no_grad_records_nothing(dev, kind):
    m, V = _model(kind, dev)
    with torch.no_grad():
        out = m(norm=3.0)
    assert out.grad_fn is None and not out.requires_grad and not hasattr(out, '_nmf_source')
    frozen, _ = _model(kind, dev, trainable_W=False, trainable_H=False, trainable_Z=False)
    assert frozen().grad_fn is None                           # nothing requires grad: today's path


def test_fit_records_nothing(dev):
    m, V = _model('PLCA', dev)
    m.fit(V.to(dev), max_iter=3)
    assert all(p.grad is None and p.grad_fn is None for p in m.parameters())


def test_betamu_still_rejects_plca(dev):
    """The output carries no provenance tag, so trainer.BetaMu answers a PLCA prediction exactly as before."""
    m, V = _model('PLCA', dev)
    out = m()
    assert getattr(out, '_nmf_source', None) is None


@pytest.mark.parametrize('kind', ['PLCA', 'SIPLCA'])
def test_sgd_steps_lower_the_loss(dev, kind):
    from torchnmf_amd.metrics import kl_div
    m, V = _model(kind, dev)
    Vd = V.to(dev)
    norm = Vd.sum()
    opt = torch.optim.SGD(m.parameters(), lr=1e-6)           # gradients are of order norm: see the golden tool's printout
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = kl_div(m(norm=norm), Vd)
        loss.backward()
        opt.step()
        with torch.no_grad():
            for p in m.parameters():
                p.clamp_(min=0)                               # plain gradient steps do not keep the factors non-negative
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(kl_div(m(norm=norm), Vd)))
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2], losses
    assert all(bool((p >= 0).all()) for p in m.parameters())


# ---- golden: the reference's own float64 gradients ---------------------------------------------------------------------
@pytest.mark.parametrize('tag,kind', [('plca', 'PLCA'), ('siplca', 'SIPLCA'), ('siplca2', 'SIPLCA2'), ('siplca3', 'SIPLCA3')])
def test_golden_g18(dev, tag, kind):
    from torchnmf_amd import plca
    d = load_golden('g18_plca_autograd')
    T = lambda k: torch.from_numpy(d[f'{tag}_{k}'])
    W0, H0, Z0, G = T('W0'), T('H0'), T('Z0'), T('G')
    m = getattr(plca, kind)(W=W0, H=H0, Z=Z0)
    for p, v in ((m.W, W0), (m.H, H0), (m.Z, Z0)):
        p.data.copy_(v)                                       # the reference's parameters, bit for bit
    m = m.to(dev)
    out = m()
    out.backward(G.to(dev))
    ref = reference(G, H0, W0, Z0)                            # (bounds; its gradients agree with the golden ones to 1e-12:
    ref.update(gH=T('gH'), gW=T('gW'), gZ=T('gZ'))            #  test_plca_autograd_host.py)
    _check_all('plca_autograd_golden', tag, ref, m.H.grad, m.W.grad, m.Z.grad)
