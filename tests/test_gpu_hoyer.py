"""The batched Hoyer projection kernel per element against the float64 restatement (tests/hoyer_emulation.py), then
trainer.SparsityProj and sparse_fit end to end against the reference's recorded runs (g16 / g17).

Kernel bound: per-slice relative Frobenius error <= 8 x the largest e_ref of g15_hoyer_proj -- e_ref is the reference's own
fp32 error against a float64 run of itself on the same kind of data (s = |randn|, the same sigma and n); the kernel sums in
another order and across 256 lanes, an algorithmic slip shows at 1e-3 or more.  An element the restatement leaves at 0 must
stay within that bound x the slice's largest element.  The measured maxima go to conftest.record (MI355X: 4.1e-7 = 0.22 x the
largest e_ref against the bound of 1.49e-5; 2.8e-9 at zeroed elements).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, record, rel_err
from hoyer_emulation import project_slice

pytestmark = pytest.mark.gpu

TOL = 1e-4                                    # the project's parity bar against the reference
G15 = load_golden('g15_hoyer_proj')
BOUND = 8 * float(G15['e_ref'].max())
SIGMAS = (0.2, 0.4, 0.8)
SIZES = (2, 3, 63, 64, 65, 255, 257, 1000, 5000)
SLICES = (1, 3, 130)
LAYOUTS = ('rows', 'cols', '3d')
FORCED = 256                                  # lds_max_elems that sends n in {257, 258, 300, 1000} to the streamed residency


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.asarray(a))


@functools.lru_cache(maxsize=None)
def _case(n, J):
    """Slice-major inputs [J][n] (fp32), fp32-rounded targets, and the restatement's result: computed once per (n, J) and
    shared by every layout and residency."""
    rng = np.random.default_rng(1000 * n + J)
    s = np.abs(rng.standard_normal((J, n))).astype(np.float32)
    sigma = np.asarray([SIGMAS[j % 3] for j in range(J)])
    nrm = np.sqrt((s.astype(np.float64) ** 2).sum(1))
    k1 = ((n ** 0.5 * (1 - sigma) + sigma) * nrm).astype(np.float32)
    k2 = (nrm * nrm).astype(np.float32)
    ref = np.empty((J, n))
    passes = np.empty(J, dtype=np.int64)
    for j in range(J):
        ref[j], passes[j] = project_slice(s[j], k1[j], k2[j])
    for a in (s, sigma, k1, k2, ref, passes):
        a.setflags(write=False)
    return s, sigma, k1, k2, ref, passes


def _inner(n):
    """The trailing extent of the 3-D (W-like) layout: 3 where it divides n, else the smallest of 2 / 5 that does; a prime n
    has outer = 1 only."""
    return next((d for d in (3, 2, 5) if n % d == 0 and n > d), n)


def _arrange(sm, layout):
    """Slice-major [J][n] -> (tensor, dim) in the layout under test."""
    J, n = sm.shape
    if layout == 'rows':                      # (n, J), slices are columns: outer = n, inner = 1
        return np.ascontiguousarray(sm.T), 1
    if layout == 'cols':                      # (J, n), slices are rows: outer = 1, inner = n
        return np.ascontiguousarray(sm), 0
    inner = _inner(n)                         # (n / inner, J, inner)
    return np.ascontiguousarray(sm.reshape(J, n // inner, inner).transpose(1, 0, 2)), 1


def _slice_major(x, layout):
    J = x.shape[0] if layout == 'cols' else x.shape[1]
    if layout == 'rows':
        return x.T
    if layout == 'cols':
        return x
    return x.transpose(1, 0, 2).reshape(J, -1)


def _run_kernel(dev, n, J, layout, lds_max_elems=None):
    from torchnmf_amd import hoyer
    s, sigma, k1, k2, ref, passes = _case(n, J)
    x_host, dim = _arrange(s, layout)
    x = t(x_host).to(dev)
    status = hoyer.project_(x, t(k1).to(dev), t(k2).to(dev), dim, lds_max_elems)
    torch.cuda.synchronize()
    got = _slice_major(x.cpu().numpy(), layout).astype(np.float64)
    return got, status.cpu().numpy(), ref, passes


def _check(got, status, ref, n, name):
    err = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    zero = ref == 0
    leak = (np.abs(got) * zero).max(1) / np.abs(ref).max(1)
    record(name, n=n, J=len(ref), max_rel=float(err.max()), max_zero_leak=float(leak.max()), bound=BOUND,
           ratio_to_e_ref=float(err.max() / float(G15['e_ref'].max())))
    print(f'{name}: max rel {err.max():.2e} zero leak {leak.max():.2e} bound {BOUND:.2e} passes {status.min()}..{status.max()}')
    assert np.isfinite(got).all()
    assert err.max() <= BOUND, (err.max(), BOUND)
    assert leak.max() <= BOUND, (leak.max(), BOUND)
    assert (status >= 1).all() and (status <= n).all(), status       # 1 <= passes <= n, never the (negative) cap code


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('J', SLICES)
@pytest.mark.parametrize('n', SIZES)
def test_kernel_matches_restatement(dev, n, J, layout):
    """Default residency: slices up to 4032 elements in the small LDS request, n = 5000 in the large one."""
    got, status, ref, _ = _run_kernel(dev, n, J, layout)
    _check(got, status, ref, n, f'hoyer_kernel[{n}-{J}-{layout}]')


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('J', SLICES)
@pytest.mark.parametrize('n', (257, 258, 1000))
def test_kernel_streamed_residency(dev, n, J, layout):
    """lds_max_elems = 256 sends these to the streamed residency: through a transposed copy in ws (rows), a regrouped one
    (3d; 257 is prime, 258 = 86 x 3 stands in for it there), or in place where the tensor is slice-major already (cols, J = 1)."""
    from torchnmf_amd import _capi, hoyer
    x_host, dim = _arrange(_case(n, J)[0], layout)
    outer = int(np.prod(x_host.shape[:dim]))
    inner = int(np.prod(x_host.shape[dim + 1:]))
    n_ws = _capi.load().nmfmu_hoyer_project_ws(outer, J, inner, FORCED)
    assert n_ws == (0 if outer == 1 or J == 1 else 4 * J * n)
    got, status, ref, _ = _run_kernel(dev, n, J, layout, FORCED)
    _check(got, status, ref, n, f'hoyer_kernel_streamed[{n}-{J}-{layout}]')
    lds, _, _, _ = _run_kernel(dev, n, J, layout)
    assert np.array_equal(lds, got), 'the two residencies run the same arithmetic'


def test_invariants(dev):
    """J = 130, n = 1000: non-negative, the two norms on target, and metrics.sparseness of every slice = its sigma."""
    from torchnmf_amd import hoyer, metrics
    n, J = 1000, 130
    s, sigma, k1, k2, _, _ = _case(n, J)
    x = t(np.ascontiguousarray(s.T)).to(dev)
    hoyer.project_(x, t(k1).to(dev), t(k2).to(dev), 1)
    v = x.double().cpu().numpy()
    assert (v >= 0).all()
    e1 = np.abs(v.sum(0) - k1) / k1
    e2 = np.abs((v * v).sum(0) - k2) / k2
    sp = np.asarray([float(metrics.sparseness(x[:, j].contiguous())) for j in range(J)])
    record('hoyer_invariants', l1=float(e1.max()), l2=float(e2.max()), sparseness=float(np.abs(sp - sigma).max()), bound=BOUND)
    assert e1.max() <= BOUND and e2.max() <= BOUND, (e1.max(), e2.max())
    assert np.abs(sp - sigma).max() <= 1e-5


@pytest.mark.parametrize('lds_max_elems', [None, FORCED])
def test_degenerate_slices_stay_confined(dev, lds_max_elems):
    """An all-zero slice and a slice with k2 = 0 among ordinary ones (n = 300, both residencies): the call returns, and the
    neighbours still match the restatement."""
    from torchnmf_amd import hoyer
    n, J = 300, 5
    s, _, k1, k2, ref, _ = (np.array(a) for a in _case(n, J))
    s[1] = 0.0
    k2[3] = 0.0
    x = t(np.ascontiguousarray(s.T)).to(dev)
    status = hoyer.project_(x, t(k1).to(dev), t(k2).to(dev), 1, lds_max_elems)
    torch.cuda.synchronize()
    got = x.cpu().numpy().T.astype(np.float64)
    status = status.cpu().numpy()
    keep = [0, 2, 4]
    _check(got[keep], status[keep], ref[keep], n, f'hoyer_degenerate[{lds_max_elems}]')
    assert (np.abs(status) >= 1).all() and (np.abs(status) <= n).all()


def test_public_wrapper(dev):
    """hoyer_project: a new tensor by default, in place with out=x, float targets, other dtypes and strides through a copy."""
    from torchnmf_amd.hoyer import hoyer_project, slice_norms
    n, J = 63, 3
    s, _, k1, k2, ref, _ = _case(n, J)
    x = t(np.ascontiguousarray(s.T)).to(dev)
    x0 = x.clone()
    y = hoyer_project(x, t(k1).to(dev), t(k2).to(dev))
    assert torch.equal(x, x0) and y is not x
    assert hoyer_project(x, t(k1).to(dev), t(k2).to(dev), out=x) is x and torch.equal(x, y)
    yd = hoyer_project(x0.double(), t(k1).to(dev), t(k2).to(dev))
    assert yd.dtype == torch.float64 and torch.equal(yd.float(), y)
    xt = x0.t().contiguous().t()                                  # same values, column-major strides
    assert not xt.is_contiguous()
    hoyer_project(xt, t(k1).to(dev), t(k2).to(dev), out=xt)
    assert torch.equal(xt, y)
    # float targets: unit L2 norm at sparseness 0.4 for every slice
    l1 = n ** 0.5 * 0.6 + 0.4
    z = hoyer_project(x0, l1, 1.0)
    assert float((slice_norms(z, 1) - 1).abs().max()) < 1e-5 and float((z.sum(0) - l1).abs().max()) < 1e-4 and bool((z >= 0).all())
    assert rel_err(y.cpu().numpy().T, ref) <= BOUND


# ---- trainer.SparsityProj ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('attr', ['W', 'H'])
def test_sparsity_proj_g16(dev, attr):
    from torchnmf_amd.metrics import beta_div
    from torchnmf_amd.nmf import NMF
    from torchnmf_amd.trainer import SparsityProj
    g = load_golden('g16_sparsity_proj')
    V = t(g['V']).to(dev)
    m = NMF(W=t(g['W0']), H=t(g['H0'])).to(dev)
    opt = SparsityProj([getattr(m, attr)], 0.3)

    def closure():
        opt.zero_grad()
        return beta_div(m(), V, 2)
    lrs = []
    for step in range(1, 11):
        loss = opt.step(closure)
        lrs.append(opt.param_groups[0]['lr'])
        if step in (1, 10):
            ew = rel_err(m.W.data.cpu(), g[f'{attr}_W{step}'])
            eh = rel_err(m.H.data.cpu(), g[f'{attr}_H{step}'])
            record(f'sparsity_proj_g16[{attr}-{step}]', W=ew, H=eh)
            assert ew < TOL and eh < TOL, (step, ew, eh)
    assert lrs == list(g[f'{attr}_lr']), (lrs, list(g[f'{attr}_lr']))
    assert loss.device.type == 'cuda' and loss.dim() == 0


def test_sparsity_proj_convolutive_layer_and_dtype(dev):
    """One step on the W of an NMFD (dim 1 of a (C, R, T) tensor) leaves every slice at the target sparseness; other dtypes
    are refused."""
    from torchnmf_amd import metrics
    from torchnmf_amd.nmf import NMFD
    from torchnmf_amd.trainer import SparsityProj
    torch.manual_seed(3)
    V = torch.rand(1, 33, 50).to(dev)
    m = NMFD((1, 33, 50), rank=4, T=3).to(dev)
    opt = SparsityProj([m.W], 0.5)

    def closure():
        opt.zero_grad()
        return metrics.beta_div(m(), V, 2)
    # a step whose ten tries were all rejected leaves the last gradient step un-projected (as in the reference) and a smaller
    # lr behind; the first accepted step must leave every slice projected
    for _ in range(4):
        first = float(closure())
        last = float(opt.step(closure))
        if last <= first:
            break
    assert last <= first, (first, last, opt.param_groups[0]['lr'])
    for r in range(4):
        assert abs(float(metrics.sparseness(m.W.data[:, r].contiguous())) - 0.5) < 1e-5
    assert bool((m.W.data >= 0).all())
    md = NMFD((1, 33, 50), rank=4, T=3).double().to(dev)
    with pytest.raises(NotImplementedError):
        SparsityProj([md.W], 0.5).step(lambda: metrics.beta_div(md(), V, 2))


# ---- sparse_fit ----------------------------------------------------------------------------------------------------------
G17_CLASSES = {'nmf': 'NMF', 'nmfd': 'NMFD', 'nmf2d': 'NMF2D'}


@pytest.mark.parametrize('name', [str(c) for c in load_golden('g17_sparse_fit')['cases']])
def test_sparse_fit_g17(dev, name):
    from torchnmf_amd import nmf
    from torchnmf_amd.hoyer import slice_norms
    g = load_golden('g17_sparse_fit')
    tag, b, w, h = name.split('_')
    beta = float(b[1:])
    sW = None if w[1:] == 'None' else float(w[1:])
    sH = None if h[1:] == 'None' else float(h[1:])
    m = getattr(nmf, G17_CLASSES[tag])(W=t(g[f'{tag}_W0']), H=t(g[f'{tag}_H0'])).to(dev)
    n = m.sparse_fit(t(g[f'{tag}_V']).to(dev), beta=beta, max_iter=20, sW=sW, sH=sH)
    ew, eh = rel_err(m.W.data.cpu(), g[f'{name}_W']), rel_err(m.H.data.cpu(), g[f'{name}_H'])
    record(f'sparse_fit_g17[{name}]', W=ew, H=eh, n_iter=n)
    print(f'{name}: n_iter {n} W {ew:.2e} H {eh:.2e}')
    assert n == int(g[f'{name}_n'])
    assert ew < TOL and eh < TOL, (ew, eh)
    if sW is not None:
        assert bool((m.W.data >= 0).all())
    if sH is not None:
        assert bool((m.H.data >= 0).all())
        assert float((slice_norms(m.H.data, 1) - 1).abs().max()) < 1e-5          # _renorm(W, H, 'H')


def test_sparse_fit_nmf3d_and_wide_rank(dev):
    """The two engines no golden case reaches: NMF3D (three shift axes) and NMF above rank 128 (the GEMM engine behind
    WideRankMU).  Constrained slices end non-negative at their sparseness."""
    from torchnmf_amd import metrics
    from torchnmf_amd.nmf import NMF, NMF3D
    torch.manual_seed(5)
    for m, V, kw in ((NMF3D((1, 3, 8, 9, 10), rank=2, kernel_size=(2, 3, 2)), torch.rand(1, 3, 8, 9, 10), dict(sW=0.4)),
                     (NMF((150, 140), rank=130), torch.rand(150, 140), dict(sW=0.4)),
                     (NMF((150, 140), rank=130), torch.rand(150, 140), dict(sH=0.4))):
        m, V = m.to(dev), V.to(dev)
        assert m.sparse_fit(V, max_iter=0, **kw) == 0                      # the initial projection alone
        assert m.sparse_fit(V, max_iter=3, **kw) == 3
        assert bool(torch.isfinite(m.W.data).all()) and bool(torch.isfinite(m.H.data).all())
        p, s = (m.W, kw['sW']) if 'sW' in kw else (m.H, kw['sH'])
        for r in range(0, p.shape[1], 37):
            assert abs(float(metrics.sparseness(p.data[:, r].contiguous())) - s) < 1e-5
        assert bool((p.data >= 0).all())


def test_sparse_fit_wide_rank_engine_follows_external_edits(dev):
    """NMF above rank 128 with H constrained: the W half-step of iteration 2 is a multiplicative update on the GEMM engine,
    which keeps a transposed copy of H; it must see the H that the projected step and the renormalisation of iteration 1 left.
    That update depends on (W, H) after iteration 1 only, and W's column directions survive the later rescaling -- so two
    iterations in one call and one iteration in each of two calls (a fresh engine for the second) must agree on them."""
    from torchnmf_amd.hoyer import slice_norms
    from torchnmf_amd.nmf import NMF
    torch.manual_seed(6)
    V = torch.rand(150, 140).to(dev)
    W0, H0 = torch.randn(140, 130).abs(), torch.randn(150, 130).abs()
    a, b = NMF(W=W0, H=H0).to(dev), NMF(W=W0, H=H0).to(dev)
    a.sparse_fit(V, max_iter=2, sH=0.4)
    b.sparse_fit(V, max_iter=1, sH=0.4)
    b.sparse_fit(V, max_iter=1, sH=0.4)
    da, db = (m.W.data / slice_norms(m.W.data, 1) for m in (a, b))
    err = rel_err(da.cpu(), db.cpu())
    record('sparse_fit_wide_rank_refresh', err=err)
    assert err < 1e-5, err


def test_sparse_fit_errors_and_dtypes(dev):
    from torchnmf_amd.nmf import NMF
    torch.manual_seed(7)
    V = torch.rand(30, 20)
    m = NMF((30, 20), 4).to(dev)
    Vz = V.clone()
    Vz[3, 4] = 0.0
    with pytest.raises(ValueError):
        m.sparse_fit(Vz.to(dev), beta=0, sW=0.4)
    Vn = V.clone()
    Vn[1, 1] = -0.5
    with pytest.raises(AssertionError):
        m.sparse_fit(Vn.to(dev), sW=0.4)
    with pytest.raises(NotImplementedError):
        m.sparse_fit(torch.where(V > 0.5, V, torch.zeros(())).to_sparse().to(dev), sW=0.4)
    # a float64 module fits on fp32 working copies and keeps its dtype
    W0, H0 = torch.randn(20, 4).abs(), torch.randn(30, 4).abs()
    m32 = NMF(W=W0, H=H0).to(dev)
    m64 = NMF(W=W0, H=H0).double().to(dev)
    assert m32.sparse_fit(V.to(dev), max_iter=3, sW=0.4, sH=0.3) == 3
    assert m64.sparse_fit(V.double().to(dev), max_iter=3, sW=0.4, sH=0.3) == 3
    assert m64.W.dtype == torch.float64 and m64.H.dtype == torch.float64
    assert torch.equal(m64.W.data.float(), m32.W.data) and torch.equal(m64.H.data.float(), m32.H.data)
