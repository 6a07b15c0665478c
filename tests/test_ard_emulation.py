"""ARD-NMF without a GPU: the float64 model (tests/ard_emulation.py) keeps its promises -- the objective never rises, the planted
rank is found -- and ``ard.ArdMU`` / ``NMF.fit_ard`` driven on the CPU by an oracle-backed stand-in backend agree with it."""
import numpy as np
import pytest
import torch

import ard_emulation as E
from cpu_backend import OracleBackend
from torchnmf_amd import _capi, ard, engine, metrics
from torchnmf_amd import nmf as anmf
from torchnmf_amd.nmf import NMF, NMFD

PRIORS = ('l1', 'l2')
BETAS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)


class ArdOracleBackend(OracleBackend):
    """cpu_backend.OracleBackend plus the two ARD entries, in fp32 torch arithmetic (same buffer contracts as HipBackend)."""

    def ard_apply(self, st, kl_den, pen, prior, norm_part, norm):
        f = st.owner.f
        rows, rank = f.shape
        neg = st.slab_num.view(st.nsplit, st.owner.rows_pad, st.r_pad).sum(0)[:rows, :rank].relu() + E.EPS
        if kl_den is not None:
            pos = kl_den[:rank].expand(rows, rank)
        else:
            pos = st.slab_den.view(st.nsplit, st.owner.rows_pad, st.r_pad).sum(0)[:rows, :rank].relu() + E.EPS
        p = pen[:rank]
        pos = pos + (p if prior == 'l1' else p * f)
        mult = neg / pos
        gamma = float(st.struct.gamma)
        f.mul_(mult if gamma == 1 else mult.pow(gamma))
        self.pack_factor(st.owner, rank, st.r_pad, 0)
        norm.zero_()
        norm[:rank] = f.sum(0) if prior == 'l1' else 0.5 * (f * f).sum(0)

    def ard_relevance(self, norm_w, norm_h, rank, r_pad, b, c, phi, lam, pen, delta):
        new = ((norm_w[:rank] + norm_h[:rank]) + b) / c
        delta[0] = ((new - lam[:rank]).abs() / lam[:rank]).max()
        lam.zero_(), pen.zero_()
        lam[:rank] = new
        pen[:rank] = phi / new


@pytest.fixture
def cpu_engine(monkeypatch):
    monkeypatch.setattr(engine, 'DEFAULT_BACKEND_FACTORY', ArdOracleBackend)
    monkeypatch.setattr(anmf, '_require_device', lambda t_, what: None)


def _problem(N, C, R, seed):
    rng = np.random.default_rng(seed)
    V = rng.random((N, C)) + 0.05
    return V, np.abs(rng.standard_normal((C, R))), np.abs(rng.standard_normal((N, R)))


# ---- the float64 model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prior', PRIORS)
@pytest.mark.parametrize('beta', BETAS)
def test_objective_never_rises(prior, beta):
    """After every sub-step (W, H, relevance) of 100 iterations on 41 x 23 at rank 6: no rise above 1e-12 relative."""
    V, W0, H0 = _problem(41, 23, 6, 1)
    b = E.default_b(V.mean(), 6, 5.0, prior)
    tr = []
    E.iterate(V, W0, H0, beta, prior, 0.1, 5.0, b, 100, trace=tr)
    tr = np.array(tr)
    assert tr.size == 1 + 3 * 100 and np.all(np.isfinite(tr))
    rise = (tr[1:] - tr[:-1]) / np.abs(tr[:-1])
    print(f'{prior} beta={beta:g}: worst relative rise {rise.max():.3e}, objective {tr[0]:.6g} -> {tr[-1]:.6g}')
    assert rise.max() <= 1e-12
    assert tr[-1] < tr[0]


@pytest.mark.parametrize('prior', PRIORS)
def test_planted_rank_is_found(prior):
    """40 x 60 of rank 3 with 2 % multiplicative noise at R = 8, beta = 1, phi = 0.1: exactly three components keep a relative
    relevance well above 0, five sit at 0; phi = 0.01 and phi = 1 do not recover 3 (the docstring's warning)."""
    p = E.PLANTED
    V, W0, H0 = E.planted()
    b, c = E.default_b(V.mean(), p['R'], p['a'], prior), E.c_of(p['N'], p['C'], p['a'], prior)
    found = {}
    for phi in (0.01, p['phi'], 1.0):
        _, _, lam = E.iterate(V, W0, H0, p['beta'], prior, phi, p['a'], b, p['n_iter'])
        rr = np.sort(E.relative_relevance(lam, b, c))[::-1]
        found[phi] = int((rr > 1e-2).sum())
        if phi == p['phi']:
            print(f'{prior}: relative relevance {np.round(rr, 3)}')
            assert rr[2] > 10 and np.all(np.abs(rr[3:]) < 1e-3)
    assert found[p['phi']] == 3 and found[0.01] != 3 and found[1.0] != 3, found


# ---- the engine, driven on the CPU, against the model ---------------------------------------------------------------------------
@pytest.mark.parametrize('prior', PRIORS)
@pytest.mark.parametrize('beta', (0.5, 1.0, 2.0))
def test_engine_matches_emulation(cpu_engine, prior, beta):
    V, W0, H0 = _problem(41, 23, 6, 2)
    a, phi = 5.0, 0.1
    b = E.default_b(V.mean(), 6, a, prior)
    W, H = torch.from_numpy(W0).float().contiguous(), torch.from_numpy(H0).float().contiguous()
    eng = ard.ArdMU(torch.from_numpy(V).float(), W, H, beta, prior, phi, a, b, 'bf16x3')
    assert eng.exponent == E.exponent(beta, prior) and float(eng.eng.step_w.struct.gamma) == np.float32(eng.exponent)
    V32 = V.astype(np.float32).astype(np.float64)
    lam0 = E.relevance(W0.astype(np.float32), H0.astype(np.float32), prior, b, eng.c)
    np.testing.assert_allclose(eng.lam.numpy(), lam0, rtol=1e-6)
    obj0 = eng.objective()
    for _ in range(20):
        eng.w_step()
        eng.h_step()
        eng.relevance_step()
    Wr, Hr, lam = E.iterate(V32, W0.astype(np.float32), H0.astype(np.float32), beta, prior, phi, a, b, 20)
    for got, ref in ((eng.lam, lam), (W, Wr), (H, Hr)):
        err = np.abs(got.numpy() - ref).max() / np.abs(ref).max()
        assert err < 1e-5, err
    # the objective: the engine's, the functional form and the model agree, and it fell
    obj = eng.objective()
    ref = E.objective(Hr, Wr, V32, lam, beta, prior, phi, a, b)
    fn = float(metrics.ard_objective(H, W, torch.from_numpy(V).float(), eng.lam, beta, prior, phi, a, b))
    assert abs(obj - ref) <= 1e-5 * abs(ref) + 1e-3 and abs(fn - ref) <= 1e-5 * abs(ref) + 1e-3 and obj < obj0
    np.testing.assert_allclose(eng.relative_relevance().numpy(), E.relative_relevance(lam, b, eng.c), rtol=1e-4, atol=1e-4)
    assert float(eng.pen[6:].abs().max()) == 0 and float(eng._lam[6:].abs().max()) == 0


def test_frozen_factor_keeps_its_norm_in_lambda(cpu_engine):
    V, W0, H0 = _problem(41, 23, 6, 3)
    b = E.default_b(V.mean(), 6, 5.0, 'l2')
    W, H = torch.from_numpy(W0).float().contiguous(), torch.from_numpy(H0).float().contiguous()
    m = NMF(W=W, H=H, trainable_W=False)
    n = m.fit_ard(torch.from_numpy(V).float(), beta=1, prior='l2', phi=0.1, b=b, tol=0, max_iter=20, precision='bf16x3')
    Wr, Hr, lam = E.iterate(V.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), 1.0, 'l2', 0.1, 5.0, b, 20,
                            update_W=False)
    assert n == 20 and torch.equal(m.W.data, W)
    np.testing.assert_allclose(m.last_relevance.numpy(), lam, rtol=1e-5)
    np.testing.assert_allclose(m.H.data.numpy(), Hr, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize('prior', PRIORS)
def test_fit_ard_prunes_the_planted_case(cpu_engine, prior):
    """The whole driver on the stand-in backend (fp32): default b, stop rule, effective_rank and prune."""
    p = E.PLANTED
    V, W0, H0 = E.planted()
    m = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float())
    with pytest.raises(RuntimeError, match='fit_ard first'):
        m.effective_rank()
    with pytest.raises(RuntimeError, match='fit_ard first'):
        m.prune()
    Vt = torch.from_numpy(V).float()
    n = m.fit_ard(Vt, beta=p['beta'], prior=prior, phi=p['phi'], a=p['a'], tol=0, max_iter=p['n_iter'], precision='bf16x3')
    assert n == p['n_iter'] and m.last_precision == 'bf16x3'
    assert m.last_relevance.shape == (p['R'],) and m.last_relevance.dtype == torch.float32
    rr = m.last_relative_relevance
    assert m.effective_rank() == 3 and int((rr > 10).sum()) == 3 and int((rr.abs() < 1e-3).sum()) == 5
    small = m.prune()
    keep = (rr > 1e-2).nonzero().flatten()
    assert isinstance(small, NMF) and small.rank == 3 and m.rank == p['R']            # the fit removes nothing
    assert torch.equal(small.W.data, m.W.data[:, keep]) and torch.equal(small.H.data, m.H.data[:, keep])
    # the stop rule: judged every 10th iteration on that iteration's delta
    m2 = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float())
    tol = 1e-5 if prior == 'l1' else 1e-3      # (the float64 model's delta falls below these near iteration 900 / 350)
    n2 = m2.fit_ard(Vt, beta=p['beta'], prior=prior, phi=p['phi'], a=p['a'], tol=tol, max_iter=2000, precision='bf16x3')
    assert n2 % 10 == 0 and 10 <= n2 < 2000
    m3 = NMF(W=torch.from_numpy(W0).float(), H=torch.from_numpy(H0).float()).double()      # another dtype: fp32 working copies
    assert m3.fit_ard(Vt, phi=p['phi'], prior=prior, tol=tol, max_iter=2000, precision='bf16x3') == n2 and m3.W.dtype == torch.float64
    assert m3.prune().W.dtype == torch.float64
    np.testing.assert_allclose(m3.W.data.numpy(), m2.W.data.numpy(), rtol=1e-6, atol=1e-12)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_fit_ard_argument_errors(cpu_engine):
    V = torch.rand(20, 12) + 0.1
    new = lambda R=4: NMF((20, 12), R)
    with pytest.raises(NotImplementedError, match='sparse targets'):
        new().fit_ard(V.to_sparse())
    with pytest.raises(NotImplementedError, match='NMF only, not NMFD'):
        NMFD((1, 12, 20), 4, 3).fit_ard(torch.rand(1, 12, 20))
    with pytest.raises(NotImplementedError, match='rank 300 > 256'):
        NMF((20, 12), 300).fit_ard(V)
    with pytest.raises(NotImplementedError, match='not available for rank 200'):      # split bf16 stops at rank 128
        NMF((20, 12), 200).fit_ard(V, precision='bf16x3')
    for phi in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='phi'):
            new().fit_ard(V, phi=phi)
    for prior, a in (('l1', 2.0), ('l1', 1.5), ('l2', 1.0), ('l2', float('nan'))):
        with pytest.raises(ValueError, match='a must be >'):
            new().fit_ard(V, prior=prior, a=a)
    new().fit_ard(V, prior='l2', a=1.5, max_iter=1, precision='bf16x3')               # (1 < a <= 2 is fine for 'l2')
    with pytest.raises(ValueError, match="prior must be 'l1' or 'l2'"):
        new().fit_ard(V, prior='l0')
    with pytest.raises(ValueError, match='b must be > 0'):
        new().fit_ard(V, b=0.0)
    with pytest.raises(ValueError, match='precision must be one of'):
        new().fit_ard(V, precision='fp8')
    with pytest.raises(AssertionError, match='non-negative'):
        new().fit_ard(V - 1.0, precision='bf16x3')
    Vz = V.clone()
    Vz[3, 4] = 0
    with pytest.raises(ValueError, match='beta <= 0 and V contains zeros'):
        new().fit_ard(Vz, beta=0, precision='bf16x3')
    with pytest.raises(AssertionError, match='V must be'):
        new().fit_ard(V.t().contiguous(), precision='bf16x3')


def test_fit_ard_needs_the_device():
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        NMF((20, 12), 4).fit_ard(torch.rand(20, 12))


def test_abi_surface():
    import os
    from conftest import ROOT
    assert _capi.ABI_VERSION == 10 and _capi.ARD_PRIORS == {'l1': 1, 'l2': 2}
    for name in ('nmfmu_ard_apply', 'nmfmu_ard_relevance'):
        assert name in _capi.SIGNATURES
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    assert '#define NMFMU_ARD_L1 1' in hdr and '#define NMFMU_ARD_L2 2' in hdr and 'int nmfmu_ard_relevance(' in hdr
    assert 'nmfmu_ard.hip' in open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'Makefile')).read()
    assert 'ard_objective' in metrics.__all__
