"""``PLCA.fit`` on sparse-COO targets on the device (csrc/nmfmu_sparse_plca.hip, plca._SparsePlcaEM): g and both numerator
planes per element against the float64 reference under the bounds derived in tests/sparse_plca_emulation.py (no element left
out), one EM step per element from the device's own numerators (tests/plca_emulation.py), the loss, the reference's recorded
runs (golden g21, and g10 with everything stored), agreement with the dense path and the oracle, indifference to how the target
is handed over, and reproducibility.

The per-element target is the 37 x 29 pattern of ``masked_emulation.make_problem``: the owner axis cycles through 0, 1, 4, 5, 8,
9 and 20 stored entries (unroll tails, whole trips, and with chunk = 8 a row of exactly one chunk and rows split in two and
three), once drawn on the rows of V and once on its columns, so that both sides meet every count; one index of the other axis
holds no entry.

Measured on an MI355X (worst |got - ref| / bound over every element, golden errors): see DESIGN.md section 20.
"""
import functools

import numpy as np
import pytest
import torch

import plca_emulation as P
import sparse_plca_emulation as S
from conftest import load_golden, record, rel_err

pytestmark = pytest.mark.gpu

N, C = 37, 29
RANKS = [3, 33, 100, 200]             # r_pad 32 / 64 / 128 / 256, RL 1 / 1 / 2 / 4
CHUNKS = [512, 8]
TOL = 1e-4                            # the project's bar for factors after a recorded run
NO_STOP = -1e9
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(R, axis):
    return S.make_problem(N, C, R, axis)


def t(x):
    return torch.from_numpy(np.asarray(x))


def _sparse(idx, vals, shape, dev):
    return torch.sparse_coo_tensor(t(idx), t(vals), shape).to(dev)


def _state(idx, vn, W, H, Z, dev, chunk):
    """(_SparsePlcaEM on device copies of the factors, its target): the values are taken as already normalised."""
    from torchnmf_amd.metrics import SparseTarget
    from torchnmf_amd.plca import _SparsePlcaEM
    T = SparseTarget(_sparse(idx, vn, (N, C), dev), chunk=chunk)
    assert torch.equal(T.vals.cpu(), t(vn))                 # coalesced already: CSR order is the order of ``idx``
    em = _SparsePlcaEM(T, T.vals, t(W).to(dev), t(H).to(dev), t(Z).to(dev))
    return em, T


def _nan_fill(em):
    for b in (em.g, em.num_h, em.num_w, em.ws_h, em.ws_w):
        b.fill_(NAN)


def _check(name, got, ref, bound, **info):
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (name, info)
    err = S.bound_err(got, np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    frac = float(np.max(err)) if err.size else 0.0
    record(name, worst_fraction_of_bound=frac, **info)
    print(f'{name} {info}: worst |got - ref| / bound = {frac:.3f}')
    assert frac <= 1.0, (name, info, frac)
    return frac


# ---- per element against the float64 reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('R', RANKS)
def test_g_and_numerators_per_element(dev, R, chunk):
    for axis in (0, 1):
        idx, vn, W, H, Z = _problem(R, axis)
        info = dict(R=R, chunk=chunk, axis=axis)
        em, T = _state(idx, vn, W, H, Z, dev, chunk)
        assert ((T.n_ws_w if axis else T.n_ws_h) > 0) == (chunk == 8)
        r_pad = em.r_pad
        assert r_pad == P.pad_rank(R) and em.num_h.shape == (N, r_pad) and em.num_w.shape == (C, r_pad)
        em.z_old[:R].copy_(em.Z)
        _nan_fill(em)                                       # every output element and every used ws slot is written
        em.numerators()
        torch.cuda.synchronize()
        ref = S.estep(idx, vn, (N, C), H, W, Z, chunk)
        assert em.g.shape == (len(vn),)
        _check('sparse_plca_g', em.g, ref['g'], ref['g_bound'], **info)
        for side, num, key in (('h', em.num_h, 'num_h'), ('w', em.num_w, 'num_w')):
            assert bool((num[:, R:] == 0).all()), (side, info)                  # padded columns: exactly 0
            _check('sparse_plca_' + key, num[:, :R], ref[key], ref[key + '_bound'], **info)
            empty = t(ref['count_' + side] == 0).to(dev)
            assert bool(empty.any()) and bool((num[empty] == 0).all()), (side, info)    # nothing stored: exactly 0
        # the W side alone, from the device's own g: one multiply per term
        nw, nw_bound, _ = S.gather(idx, em.g.double().cpu().numpy(), (N, C), H, chunk)
        _check('sparse_plca_gather', em.num_w[:, :R], nw, nw_bound, **info)
        # the factors are inputs only
        assert torch.equal(em.W.cpu(), t(W)) and torch.equal(em.H.cpu(), t(H)) and torch.equal(em.Z.cpu(), t(Z))


STEPS = [((True, True, True), (1.0, 1.0, 1.0)), ((True, True, True), (1.02, 0.99, 1.01)),
         ((True, True, False), (1.0, 1.0, 1.0)), ((True, True, False), (1.001, 1.001, 1.001)),
         ((False, True, True), (1.0, 1.0, 1.0)), ((False, True, True), (1.02, 0.99, 1.01))]      # (W, H, Z), (aW, aH, aZ)


@pytest.mark.parametrize('R', RANKS)
def test_em_step_per_element(dev, R):
    """The device's numerators, read back, as a single slab through ``plca_emulation.em_step``."""
    idx, vn, W, H, Z = _problem(R, 0)
    for chunk, (train, alphas) in zip([512, 8] * 3, STEPS):
        em, _ = _state(idx, vn, W, H, Z, dev, chunk)
        em.em_step(*train, *alphas)
        torch.cuda.synchronize()
        nw, nh = (x[:, :R].double().cpu().numpy() for x in (em.num_w, em.num_h))
        ref = P.em_step(W, H, Z, nw, nh, train, alphas, kW=P.chain_rows(C, em.r_pad), kH=P.chain_rows(N, em.r_pad))
        tag = ''.join(n for n, on in zip('WHZ', train) if on)
        for key, new, old, on in (('W', em.W, W, train[0]), ('H', em.H, H, train[1]), ('Z', em.Z, Z, train[2])):
            new = new.cpu().numpy()
            if on:
                frac = P.excess(new, ref[key])
                record('sparse_plca_em_step', R=R, chunk=chunk, train=tag, alphas=alphas, factor=key, worst_fraction_of_bound=frac)
                print(f'sparse_plca_em_step R {R} chunk {chunk} {tag} {alphas} {key}: {frac:.3f}')
                assert frac <= 1.0, (R, chunk, tag, alphas, key, frac)
            else:
                assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), key
        assert torch.equal(em.z_old[:R].cpu(), t(Z))        # the numerators were formed with the old Z


@pytest.mark.parametrize('R', RANKS)
def test_loss(dev, R):
    for axis in (0, 1):
        idx, vn, W, H, Z = _problem(R, axis)
        em, _ = _state(idx, vn, W, H, Z, dev, 512)
        got = em.divergence()
        want, bound = S.loss(idx, vn, (N, C), H, W, Z)
        assert isinstance(got, float)
        _check('sparse_plca_loss', np.asarray(got), want, bound, R=R, axis=axis)


# ---- the reference's recorded runs ----------------------------------------------------------------------------------------------
G21 = load_golden('g21_sparse_plca')
GOLDEN_CASES = {'plain': ({}, {}), 'prior': ({}, dict(W_alpha=1.02, H_alpha=0.99, Z_alpha=1.01)),
                'frozenZ': (dict(trainable_Z=False), {}), 'frozenW': (dict(trainable_W=False), {}),
                'stop': ({}, dict(tol=1e-3, max_iter=200))}


def _golden(dev, g, V, name):
    from torchnmf_amd.plca import PLCA
    ctor, fitkw = GOLDEN_CASES[name]
    fitkw = dict(fitkw)
    fitkw.setdefault('tol', NO_STOP)
    fitkw.setdefault('max_iter', 30)
    m = PLCA(W=t(g['W0']), H=t(g['H0']), Z=t(g['Z0']), **ctor).to(dev)
    n, norm = m.fit(V, **fitkw)
    assert isinstance(norm, torch.Tensor) and norm.dim() == 0 and norm.dtype == torch.float32
    errs = {k: rel_err(p.data.cpu(), g[f'{name}_{k}']) for p, k in ((m.W, 'W'), (m.H, 'H'), (m.Z, 'Z'))}
    return n, float(norm), errs


@pytest.mark.parametrize('name', list(GOLDEN_CASES))
def test_golden_g21(dev, name):
    g = G21
    assert [str(c) for c in g['cases']] == list(GOLDEN_CASES)
    V = _sparse(g['indices'], g['values'], tuple(int(x) for x in g['shape']), dev)
    n, norm, errs = _golden(dev, g, V, name)
    record('sparse_plca_g21', case=name, n=n, **errs)
    print(f'sparse_plca_g21 {name}: n {n} W {errs["W"]:.2e} H {errs["H"]:.2e} Z {errs["Z"]:.2e}')
    assert n == int(g[f'{name}_n']) and norm == pytest.approx(float(g[f'{name}_norm']), rel=1e-5)
    assert max(errs.values()) < TOL, (name, errs)


@pytest.mark.parametrize('name', ['plain', 'prior'])
def test_golden_g10_with_everything_stored(dev, name):
    g = load_golden('g10_plca')
    V = t(g['V']).to_sparse().coalesce()
    assert V._nnz() == g['V'].size                      # the recorded target holds no zero: the two problems coincide
    n, norm, errs = _golden(dev, g, V.to(dev), name)
    record('sparse_plca_g10', case=name, n=n, **errs)
    print(f'sparse_plca_g10 {name}: n {n} W {errs["W"]:.2e} H {errs["H"]:.2e} Z {errs["Z"]:.2e}')
    assert n == int(g[f'{name}_n']) and norm == pytest.approx(float(g[f'{name}_norm']), rel=1e-5)
    assert max(errs.values()) < TOL, (name, errs)


# ---- against the dense path on the device and the oracle ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide_target():
    g = torch.Generator().manual_seed(330)
    keep = torch.rand(330, 520, generator=g) < 0.1
    V = (torch.floor(torch.rand(330, 520, generator=g) * 9) + 1) * keep
    return V


@pytest.mark.parametrize('R', [5, 100, 200])
def test_against_the_dense_path_and_the_oracle(dev, R):
    from oracle import mu_oracle as O
    from torchnmf_amd.plca import PLCA
    V = _wide_target()
    g = torch.Generator().manual_seed(R)
    W0, H0, Z0 = (torch.rand(*s, generator=g) * 0.9 + 0.1 for s in ((520, R), (330, R), (R,)))
    kw = dict(tol=NO_STOP, max_iter=6, W_alpha=1.001)
    a = PLCA(W=W0, H=H0, Z=Z0).to(dev)
    b = PLCA(W=W0, H=H0, Z=Z0).to(dev)
    na, norm_a = a.fit(V.to_sparse().to(dev), **kw)
    # the dense path's fp32-grade mode 'bf16x3' exists up to padded rank 128 (nmfmu_supported: its four image planes do not fit
    # the LDS at 256); at rank 200 it is refused, the dense path offers single-plane bf16 only, and the comparison is held to
    # the bar the project keeps for that mode (tests/test_gpu_plca_emulated_parity.py: 2e-2) -- the oracle is held to TOL at
    # every rank
    if R > 128:
        with pytest.raises(NotImplementedError, match="'bf16x3' is not available for rank 200"):
            b.fit(V.to(dev), precision='bf16x3', **kw)
    prec, dense_bar = ('bf16x3', TOL) if R <= 128 else ('bf16', 2e-2)
    nb, norm_b = b.fit(V.to(dev), precision=prec, **kw)
    Wr, Hr, Zr, nr, norm_r, _ = O.plca_fit(V, W0, H0, Z0, **kw)
    assert na == nb == nr == 5 and float(norm_a) == float(norm_b) == pytest.approx(norm_r, rel=1e-6)
    for what, ref, bar in (('dense', (b.W.data.cpu(), b.H.data.cpu(), b.Z.data.cpu()), dense_bar), ('oracle', (Wr, Hr, Zr), TOL)):
        errs = [rel_err(p.data.cpu(), r) for p, r in zip((a.W, a.H, a.Z), ref)]
        record('sparse_plca_vs_' + what, R=R, W=errs[0], H=errs[1], Z=errs[2])
        print(f'sparse_plca_vs_{what} R {R}: W {errs[0]:.2e} H {errs[1]:.2e} Z {errs[2]:.2e}')
        assert max(errs) < bar, (what, R, errs)


# ---- indifference and reproducibility -------------------------------------------------------------------------------------------
def _fit(dev, V, W, H, Z, **kw):
    from torchnmf_amd.plca import PLCA
    m = PLCA(W=t(W), H=t(H), Z=t(Z)).to(dev)
    kw.setdefault('tol', NO_STOP)
    kw.setdefault('max_iter', 10)
    n, norm = m.fit(V, **kw)
    return n, norm, m.W.data.clone(), m.H.data.clone(), m.Z.data.clone()


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize('chunk', CHUNKS)
def test_target_object_and_repeated_fits_are_bitwise_equal(dev, chunk):
    from torchnmf_amd.metrics import SparseTarget
    idx, vn, W, H, Z = _problem(200, 0)
    vals = (vn * np.float32(977.0)).astype(np.float32)
    V = _sparse(idx, vals, (N, C), dev)
    T = SparseTarget(V, chunk=chunk)
    assert (T.n_ws_h > 0) == (chunk == 8)
    first, second = _fit(dev, T, W, H, Z, W_alpha=1.02), _fit(dev, T, W, H, Z, W_alpha=1.02)
    assert _same(first, second) and bool(torch.isfinite(first[2]).all()) and not torch.equal(first[2].cpu(), t(W))
    if chunk == 512:                                       # the tensor is prepared with the default chunk
        assert _same(first, _fit(dev, V, W, H, Z, W_alpha=1.02))
    assert float(first[1]) == float(V.coalesce().values().sum())


def test_stored_zeros_change_nothing_beyond_rounding(dev):
    """Explicit zeros among the stored entries: g = 0 there.  They lengthen rows (other trips, other segments), so the factors
    move within the bounds of one EM step from the same numerators."""
    idx, vn, W, H, Z = _problem(33, 0)
    Vd, Mk = S.dense(idx, vn, (N, C))
    extra = np.argwhere(~Mk)[::7]
    idx2 = np.concatenate([np.asarray(idx), extra.T], 1)
    vals2 = np.concatenate([vn, np.zeros(len(extra), dtype=np.float32)])
    order = np.lexsort((idx2[1], idx2[0]))
    idx2, vals2 = idx2[:, order], vals2[order]
    em, _ = _state(idx2, vals2, W, H, Z, dev, 8)
    assert em.T.nnz == len(vn) + len(extra) and em.T.has_zero
    em.em_step(True, True, True, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    ref_t = S.estep(idx, vn, (N, C), H, W, Z, 8)            # the float64 numerators of the target WITHOUT the zeros
    # bounds with the counts of the longer rows
    lng = S.estep(idx2, vals2, (N, C), H, W, Z, 8)
    assert np.array_equal(lng['num_h'], ref_t['num_h']) and np.array_equal(lng['num_w'], ref_t['num_w'])
    _check('sparse_plca_zeros_num_h', em.num_h[:, :33], ref_t['num_h'], lng['num_h_bound'])
    _check('sparse_plca_zeros_num_w', em.num_w[:, :33], ref_t['num_w'], lng['num_w_bound'])
    nw, nh = (x[:, :33].double().cpu().numpy() for x in (em.num_w, em.num_h))
    ref = P.em_step(W, H, Z, nw, nh, kW=P.chain_rows(C, em.r_pad), kH=P.chain_rows(N, em.r_pad))
    for key, new in (('W', em.W), ('H', em.H), ('Z', em.Z)):
        assert P.excess(new.cpu().numpy(), ref[key]) <= 1.0, key


def test_a_target_that_sums_to_zero_raises(dev):
    from torchnmf_amd.plca import PLCA
    idx, vn, W, H, Z = _problem(3, 0)
    m = PLCA(W=t(W), H=t(H), Z=t(Z)).to(dev)
    before = [p.data.clone() for p in (m.W, m.H, m.Z)]
    with pytest.raises(ValueError, match='sum to 0'):
        m.fit(_sparse(idx, np.zeros_like(vn), (N, C), dev))
    with pytest.raises(ValueError, match='sum to 0'):
        m.fit(torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (N, C)).to(dev))
    with pytest.raises(AssertionError, match='Target should be non-negative'):
        m.fit(_sparse(idx, -vn, (N, C), dev))
    assert all(torch.equal(p.data, b) for p, b in zip((m.W, m.H, m.Z), before))       # nothing was touched


def test_float64_target_fits_like_its_fp32_copy(dev):
    idx, vn, W, H, Z = _problem(100, 1)
    vals = (vn * np.float32(123.0)).astype(np.float32)
    a = _fit(dev, _sparse(idx, vals, (N, C), dev), W, H, Z)
    b = _fit(dev, _sparse(idx, vals.astype(np.float64), (N, C), dev), W, H, Z)
    assert _same(a, b) and a[1].dtype == b[1].dtype == torch.float32 and float(a[1]) == float(b[1])
