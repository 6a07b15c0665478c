"""NTF on the device against plain float64 numpy: the per-element terms, step and loss of ``nmfmu_ntf_*`` at the shapes where
the two walks, the flat stages, the load widths and the split can go wrong, then the fit.

Bound of ``num``, ``den`` and the updated factor (derived, not measured): every summand is non-negative, so the first-order
relative error of the pinned arithmetic is at most ``(R + L + 64) 2^-24`` -- ``R`` for the reconstruction, ``L`` (the mode's
contraction length) for the accumulation, 64 for the panel rounding, the seed arithmetic and ``exp2f`` / ``log2f`` at
``|beta - 2| <= 3`` on this data range; asserted with a factor 2, per element.  Loss: ``2 (R + 64) 2^-24 S_abs`` with ``S_abs``
the float64 sum of the loss term with every piece replaced by its absolute value."""
import functools

import numpy as np
import pytest
import torch

from conftest import record, rel_err
from torchnmf_amd import ntf
from torchnmf_amd.constants import eps
from torchnmf_amd.engine import mu_gamma

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = [(131, 6, 11), (5, 132, 36), (7, 70, 2), (3, 5, 131)]


def ref_terms(V, M, fs, mode, beta):
    """(num, den) of nmf.py:61-74 with both seeds times m, float64.  V: clean where m == 0."""
    y = np.einsum('ir,jr,kr->ijk', *fs)
    if beta == 2:
        gn, gp = V, y
    elif beta == 1:
        gn, gp = V / (y + eps), np.ones_like(y)
    elif beta == 0:
        gn, gp = V / (y + eps) ** 2, 1 / (y + eps)
    else:
        gn, gp = (y + eps) ** (beta - 2) * V, (y + eps) ** (beta - 1)
    pa, pb = (f for n, f in enumerate(fs) if n != mode)
    P = pa[:, None, :] * pb[None, :, :]          # [a, b, r]; moveaxis: [rows of the mode, a, b], the other modes in order
    return tuple(np.einsum('oab,abr->or', np.moveaxis(M * g, mode, 0), P) for g in (gn, gp))


def ref_update(f, num, den, gamma, l1=0.0, l2=0.0):
    return f * ((np.maximum(num, 0) + eps) / (np.maximum(den, 0) + eps + l1 + l2 * f)) ** gamma      # nmf.py:78-92


def ref_loss(V, M, fs, beta):
    """(the loss of metrics.beta_div times m, the same with every piece replaced by its absolute value), float64."""
    s = np.einsum('ir,jr,kr->ijk', *fs)
    if beta == 2:
        return (M * 0.5 * (s - V) ** 2).sum(), (M * 0.5 * (s + V) ** 2).sum()
    if beta == 1:
        pieces = [s, -V * np.log(s + eps), V * np.log(V + eps), -V]
    elif beta == 0:
        pieces = [(V + eps) / (s + eps), np.log(s + eps), -np.log(V + eps), -np.ones_like(s)]
    else:
        vt, se, c = (V + eps if beta < 0 else V), s + eps, 1 / (beta * (beta - 1))
        pieces = [c * (beta - 1) * se ** beta, -c * beta * vt * se ** (beta - 1), c * vt ** beta]
    return sum((M * p).sum() for p in pieces), sum((M * np.abs(p)).sum() for p in pieces)


@functools.lru_cache(maxsize=None)
def problem(shape, R):
    """fp32 factors in [0.25, 1.25), V = reconstruction x [0.5, 2), weights in [0.25, 4) with ~30 % zeros and one weightless
    owner row per mode (`dead`), Vj = V with NaN / Inf / -1 / 1000 in turn under the zero weights."""
    rng = np.random.default_rng(sum(shape) + R)
    fs = [(rng.random((d, R)) + 0.25).astype(np.float32) for d in shape]
    V = (np.einsum('ir,jr,kr->ijk', *[f.astype(np.float64) for f in fs]) * rng.uniform(0.5, 2, shape)).astype(np.float32)
    M = rng.uniform(0.25, 4, shape).astype(np.float32)
    M[rng.random(shape) < 0.3] = 0
    dead = tuple(d // 2 for d in shape)
    M[dead[0]], M[:, dead[1]], M[:, :, dead[2]] = 0, 0, 0
    Vj = V.copy()
    z = np.flatnonzero(M == 0)
    Vj.flat[z] = np.resize(np.array([np.nan, np.inf, -1, 1000], np.float32), z.size)
    return fs, V, M, Vj, dead


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


host = lambda t: t.cpu().double().numpy()      # noqa: E731


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('nsplit', (1, 3))
@pytest.mark.parametrize('beta', (-1, 0, 0.5, 1, 2, 3))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', SHAPES)
def test_terms_step_loss(shape, R, beta, nsplit, weighted):
    fs, V, M, Vj, dead = problem(shape, R)
    T = ntf.NtfTarget(dev(Vj if weighted else V), dev(M) if weighted else None)
    dfs = [dev(f) for f in fs]
    f64 = [f.astype(np.float64) for f in fs]
    Vd, Md = V.astype(np.float64), (M.astype(np.float64) if weighted else np.ones(shape))
    gamma, worst = mu_gamma(beta), {}

    def within(got, ref, bound, what):
        assert np.isfinite(got).all(), what
        err = np.abs(got - ref)
        assert (err <= bound * ref).all(), (what, float((err / np.maximum(bound * ref, 1e-300)).max()))
        worst[what] = max(worst.get(what, 0.0), float((err[ref > 0] / (bound * ref[ref > 0])).max()))

    for mode in range(3):
        bound = 2 * (R + V.size // shape[mode] + 64) * U
        refs = ref_terms(Vd, Md, f64, mode, beta)
        got = ntf._ntf_call(T, dfs, mode, beta, nsplit=nsplit, _fill=float('nan'))
        again = ntf._ntf_call(T, dfs, mode, beta, nsplit=nsplit, _fill=7.0)
        for g, a, ref, what in zip(got, again, refs, ('num', 'den')):
            assert torch.equal(g, a), 'a repeated call is bitwise identical whatever the workspace held'
            g = host(g)
            assert (g[:, R:] == 0).all(), 'padded rank columns'
            within(g[:, :R], ref, bound, what)
            assert not weighted or (g[dead[mode]] == 0).all(), 'the weightless owner row'
        for l1, l2 in ((0.0, 0.0), (0.021, 0.049)):
            facs = [f.clone() for f in dfs]
            ntf._ntf_call(T, facs, mode, beta, step=(l1, l2, gamma), nsplit=nsplit, _fill=float('nan'))
            within(host(facs[mode]), ref_update(f64[mode], *refs, gamma, l1, l2), bound * max(1, gamma), 'step')
            assert all(torch.equal(facs[n], dfs[n]) for n in range(3) if n != mode), 'the panel factors are untouched'
            if weighted and l1 == 0:
                assert torch.equal(facs[mode][dead[mode]], dfs[mode][dead[mode]]), 'a weightless row keeps its bits'
    ref, s_abs = ref_loss(Vd, Md, f64, beta)
    got = float(ntf._ntf_loss(T, dfs, beta).item())
    assert abs(got - ref) <= 2 * (R + 64) * U * s_abs
    record('ntf_terms_step_loss', shape=shape, R=R, beta=beta, nsplit=nsplit, weighted=weighted,
           loss=abs(got - ref) / (2 * (R + 64) * U * s_abs), **worst)


@pytest.mark.parametrize('beta', (0.5, 2))
def test_weightless_entries_are_ignored(beta):
    fs, V, M, Vj, _ = problem((5, 132, 36), 3)
    out = []
    for target in (Vj, np.where(M > 0, V, 0).astype(np.float32)):
        m = ntf.NTF(factors=[torch.from_numpy(f) for f in fs]).cuda()
        assert m.fit(dev(target), beta=beta, tol=-1e9, max_iter=10, weights=dev(M)) == 10
        out.append([f.data for f in m.factors])
    for a, b in zip(*out):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def planted(weighted):
    rng = np.random.default_rng(5)
    shape = (20, 30, 25)
    V = np.einsum('ir,jr,kr->ijk', *[rng.random((d, 3)) + 0.1 for d in shape]).astype(np.float32)
    M = (rng.uniform(0.25, 4, shape) * (rng.random(shape) > 0.3)).astype(np.float32) if weighted else None
    start = [np.abs(rng.standard_normal((d, 3))).astype(np.float32) + 0.05 for d in shape]
    return V, M, start


def mu_loop64(V, M, start, beta, tol, max_iter):
    """The reference's fit in float64: (factors, iterations, the losses sqrt(2 div) after every iteration, loss_init)."""
    Vd, Md, fs = V.astype(np.float64), (np.ones(V.shape) if M is None else M.astype(np.float64)), [f.astype(np.float64) for f in start]
    loss_init = previous = np.sqrt(2 * ref_loss(Vd, Md, fs, beta)[0])
    losses = []
    for it in range(max_iter):
        for mode in range(3):
            fs[mode] = ref_update(fs[mode], *ref_terms(Vd, Md, fs, mode, beta), mu_gamma(beta))
        losses.append(np.sqrt(2 * ref_loss(Vd, Md, fs, beta)[0]))
        if it % 10 == 9:
            if (previous - losses[-1]) / loss_init < tol:
                break
            previous = losses[-1]
    return fs, it + 1, losses, loss_init


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('beta', (0.5, 1, 2))
def test_fit_against_float64(beta, weighted):
    """20 iterations from the same start: every factor within 1e-4 relative Frobenius of the float64 loop, the loss
    non-increasing within its own bound; then the stop rule returns the float64 loop's count.

    The issue asks for a seed whose deciding margin |(previous - loss) / loss_init - tol| in the float64 run is >= 10 x the
    loss bound.  That is NOT met, and the equality of the counts does not follow from the derived bound: it rests on the
    observed error of the loss, about 0.003 of its bound (the kernels are deterministic, so the test is not flaky).  The
    figures, computed on the CPU for this seed (beta 0.5, 1, 2; unweighted then weighted), smallest margin over the
    checkpoints against 10 x the bound in the same unit.  tol = 1e-4, no run stops before max_iter = 200: 4.8e-5, 4.6e-5,
    1.2e-4, 1.4e-3, 2.5e-4, 9.5e-5 against 7e-3 .. 1.4e-1 (on a planted tensor the loss tends to 0 and S_abs does not; a
    checkpoint that stops has a margin below tol itself, so no seed reaches the ratio).  tol = 1e-2 is checked too because
    there the rule fires, after 80, 60, 30, 70, 50, 40 iterations: 4.2e-3, 3.6e-3, 1.9e-3, 1.4e-3, 1.5e-3, 2.2e-3 against
    7.1e-2, 1.9e-2, 1.1e-3, 1.6e-2, 4.3e-3, 2.1e-3 -- only beta = 2 meets the ratio."""
    V, M, start = planted(weighted)
    Vd, Md = dev(V), (None if M is None else dev(M))
    m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
    T = ntf.NtfTarget(Vd, Md)
    ref, _, ref_losses, _ = mu_loop64(V, M, start, beta, -1e9, 20)
    Mn = np.ones(V.shape) if M is None else M.astype(np.float64)
    losses = []
    for _ in range(20):
        assert m.fit(Vd, beta=beta, tol=-1e9, max_iter=1, weights=Md) == 1
        losses.append(float(ntf._ntf_loss(T, [f.data for f in m.factors], beta).item()))
    errs = [rel_err(host(f.data), r) for f, r in zip(m.factors, ref)]
    record('ntf_fit', beta=beta, weighted=weighted, errs=errs)
    assert max(errs) < 1e-4, errs
    slack = 2 * (3 + 64) * U * ref_loss(V.astype(np.float64), Mn, ref, beta)[1]
    assert all(b <= a + 2 * slack for a, b in zip(losses, losses[1:])), losses
    assert abs(np.sqrt(2 * losses[-1]) - ref_losses[-1]) <= 1e-4 * ref_losses[-1]
    for tol in (1e-4, 1e-2):
        m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
        assert m.fit(Vd, beta=beta, tol=tol, max_iter=200, weights=Md) == mu_loop64(V, M, start, beta, tol, 200)[1], tol
