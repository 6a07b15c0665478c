"""NTF on sparse 3-way targets against plain float64 numpy on the densified tensor (the formulas of test_gpu_ntf.py; the mask
``M`` is the stored set under 'missing' and 1 under 'zero'): per-element terms, step and loss of ``nmfmu_sp_ntf_*`` where the
segment walk, the 64-entry blocks, the split rows and the two gather routes can go wrong, then the fit.

Bounds (derived, not measured; every summand is non-negative, so first-order relative errors add; asserted with a factor 2):
``num`` / ``den`` under 'missing' and ``num`` under 'zero': ``(R + n_max + 64) 2^-24`` -- ``R`` for the dot product, ``n_max`` (the
longest row of the mode) for the accumulation in storage order, 64 for the Khatri-Rao product, the seed arithmetic and
``exp2f`` / ``log2f`` at ``|beta - 2| <= 3``.  The 'zero' denominators: ``n_max`` replaced by the two panels' row counts summed
-- the column sums or Gram matrices of the two panels (``rows_a`` and ``rows_b`` additions), their product, and ``R`` for the
row-times-matrix product at beta 2.  The updated factor: the larger of its two terms' bounds times ``max(1, gamma)``.  Loss:
``2 (R + 64) 2^-24 S_abs`` with ``S_abs`` the float64 sum of the loss with every piece replaced by its absolute value."""
import functools

import numpy as np
import pytest
import torch

from conftest import record, rel_err
from test_gpu_ntf import U, dev, host, mu_loop64, planted, ref_loss, ref_terms, ref_update
from torchnmf_amd import ntf
from torchnmf_amd.engine import mu_gamma

pytestmark = pytest.mark.gpu
CASES = [('missing', -1), ('missing', 0), ('missing', 0.5), ('missing', 1), ('missing', 2), ('missing', 3), ('zero', 1), ('zero', 2)]


@functools.lru_cache(maxsize=None)
def problem(shape, R, full):
    """fp32 factors in [0.25, 1.25), values = reconstruction x [0.5, 2), about 35 % stored.  A full mode-0 slice leaves no slice
    of mode 1 or 2 empty, so the target comes in two variants.  ``full``: slice 0 of mode 0 stored in full (350 / 655 entries),
    slice ``dead[0]`` empty.  Otherwise: an empty slice in every mode and rows of exactly 1, 63, 64 and 65 entries (mode 0, or
    mode 1 where mode 0 has too few rows).  Returns (factors, dense V with zeros at the unstored places, the stored mask, dead)."""
    rng = np.random.default_rng(sum(shape) + R + full)
    fs = [(rng.random((d, R)) + 0.25).astype(np.float32) for d in shape]
    V = (np.einsum('ir,jr,kr->ijk', *[f.astype(np.float64) for f in fs]) * rng.uniform(0.5, 2, shape)).astype(np.float32)
    S, dead = rng.random(shape) < 0.35, tuple(d // 2 for d in shape)
    if full:
        S[0], S[dead[0]] = True, False
    else:
        S[dead[0]], S[:, dead[1]], S[:, :, dead[2]] = False, False, False
        live = np.ones(shape, bool)
        live[dead[0]], live[:, dead[1]], live[:, :, dead[2]] = False, False, False
        ax = 0 if shape[0] >= 6 else 1
        rows = [r for r in range(shape[ax]) if r != dead[ax]][:4]
        for r, count in zip(rows, (1, 63, 64, 65)):
            row = np.zeros(live.size // shape[ax], bool)
            row[rng.choice(np.flatnonzero(np.moveaxis(live, ax, 0)[r].reshape(-1)), count, replace=False)] = True
            np.moveaxis(S, ax, 0)[r] = row.reshape(np.moveaxis(S, ax, 0)[r].shape)
            assert np.moveaxis(S, ax, 0)[r].sum() == count
    return fs, np.where(S, V, 0).astype(np.float32), S, dead


def sparse_of(V, S, junk=None):
    """The sparse COO device tensor of the stored set ``S`` with the values of ``V`` (or of ``junk``) at it."""
    idx = np.stack(np.nonzero(S))
    return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy((V if junk is None else junk)[S]), V.shape).cuda()


@pytest.mark.parametrize('unstored,beta', CASES)
@pytest.mark.parametrize('stage', (1, 2))
@pytest.mark.parametrize('chunk', (5, 512))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', [(9, 70, 5), (3, 5, 131)])
def test_terms_step_loss(shape, R, chunk, stage, unstored, beta):
    gamma, worst, zero = mu_gamma(beta), {}, unstored == 'zero'

    def within(got, ref, bound, what):
        assert np.isfinite(got).all(), what
        err = np.abs(got - ref)
        assert (err <= bound * ref).all(), (what, float((err / np.maximum(bound * ref, 1e-300)).max()))
        worst[what] = max(worst.get(what, 0.0), float((err[ref > 0] / (bound * ref[ref > 0])).max()))

    for full in (True, False):
        fs, V, S, dead = problem(shape, R, full)
        T, T1 = ntf.SparseNtfTarget(sparse_of(V, S), chunk=chunk), ntf.SparseNtfTarget(sparse_of(V, S), chunk=None)
        dfs, f64 = [dev(f) for f in fs], [f.astype(np.float64) for f in fs]
        Vd, Md = V.astype(np.float64), (np.ones(shape) if zero else S.astype(np.float64))
        for mode in range(3):
            counts = np.moveaxis(S, mode, 0).reshape(shape[mode], -1).sum(1)
            b_num = 2 * (R + int(counts.max()) + 64) * U
            b_den = 2 * (R + sum(shape) - shape[mode] + 64) * U if zero else b_num
            refs = ref_terms(Vd, Md, f64, mode, beta)
            got = ntf._sparse_call(T, dfs, mode, beta, unstored, stage=stage, _fill=float('nan'))
            again = ntf._sparse_call(T, dfs, mode, beta, unstored, stage=stage, _fill=7.0)
            other = ntf._sparse_call(T, dfs, mode, beta, unstored, stage=3 - stage)
            whole = ntf._sparse_call(T1, dfs, mode, beta, unstored, stage=stage)
            fits = torch.from_numpy(counts <= chunk).cuda()
            for g, a, o, w, ref, bound, what in zip(got, again, other, whole, refs, (b_num, b_den), ('num', 'den')):
                assert torch.equal(g, a), 'a repeated call is bitwise identical whatever the workspace held'
                assert torch.equal(g, o), 'a panel row from LDS has the bits of the row from memory'
                assert torch.equal(g[fits], w[fits]), 'a row that fits one segment does not depend on the chunk'
                g = host(g)
                assert (g[:, R:] == 0).all(), 'padded rank columns'
                within(g[:, :R], ref, bound, what)
            for l1, l2 in ((0.0, 0.0), (0.021, 0.049)):
                facs = [f.clone() for f in dfs]
                ntf._sparse_call(T, facs, mode, beta, unstored, step=(l1, l2, gamma), stage=stage, _fill=float('nan'))
                within(host(facs[mode]), ref_update(f64[mode], *refs, gamma, l1, l2), max(b_num, b_den) * max(1, gamma), 'step')
                assert all(torch.equal(facs[n], dfs[n]) for n in range(3) if n != mode), 'the panel factors are untouched'
                if not zero and l1 == 0 and (mode == 0 or not full):
                    assert counts[dead[mode]] == 0 and torch.equal(facs[mode][dead[mode]], dfs[mode][dead[mode]]), 'an empty row'
        ref, s_abs = ref_loss(Vd, Md, f64, beta)
        got = [float(ntf._sparse_loss(T, dfs, beta, unstored, stage=s).item()) for s in (stage, 3 - stage)]
        assert got[0] == got[1] and abs(got[0] - ref) <= 2 * (R + 64) * U * s_abs, (got, ref, 2 * (R + 64) * U * s_abs)
        worst['loss'] = max(worst.get('loss', 0.0), abs(got[0] - ref) / (2 * (R + 64) * U * s_abs))
    record('sparse_ntf_terms_step_loss', shape=shape, R=R, chunk=chunk, stage=stage, unstored=unstored, beta=beta, **worst)


def test_unstored_entries_are_never_read():
    """Ten 'missing' iterations on the stored set, and again on the same stored set taken from a dense tensor that holds
    NaN / Inf / -1 at the unstored places: equal bits (the sparse tensor never carries the junk, so this pair is a
    repeatability check).  What can fail on a kernel that reads a wrong entry is the third fit: the dense weighted NTF
    kernels on the junk-holding dense tensor with the stored mask as weights.  Both fits are held to 1e-4 relative
    Frobenius of the float64 loop by their own tests, so they are within 2e-4 of each other."""
    fs, V, S, _ = problem((9, 70, 5), 3, False)
    Vj = np.where(S, V, np.resize(np.array([np.nan, np.inf, -1], np.float32), V.size).reshape(V.shape))
    out = []
    for target, kw in ((sparse_of(V, S), dict(unstored='missing')), (sparse_of(V, S, junk=Vj), dict(unstored='missing')),
                       (dev(Vj), dict(weights=dev(S.astype(np.float32))))):
        m = ntf.NTF(factors=[torch.from_numpy(f) for f in fs]).cuda()
        assert m.fit(target, beta=0.5, tol=-1e9, max_iter=10, **kw) == 10
        out.append([f.data for f in m.factors])
    for a, b, d in zip(*out):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        assert rel_err(host(a), host(d)) < 2e-4


def test_persistent_workgroups_take_several_quads():
    """More segment quads than the staged route has workgroups (8 per CU at most), so each persistent workgroup walks a run
    of quads and the loss kernel reuses its partials: the bits of every mode's step and of the loss must not depend on which
    workgroup took a segment -- stage 2 against stage 1 -- and the loss stays within its bound of float64."""
    shape, R = (20000, 8, 6), 3
    rng = np.random.default_rng(2)
    fs = [(rng.random((d, R)) + 0.25).astype(np.float32) for d in shape]
    S = rng.random(shape) < 0.07
    V = np.where(S, np.einsum('ir,jr,kr->ijk', *fs) * rng.uniform(0.5, 2, shape), 0).astype(np.float32)
    T, dfs = ntf.SparseNtfTarget(sparse_of(V, S), chunk=5), [dev(f) for f in fs]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for unstored, beta in (('missing', 0.5), ('zero', 1)):
        for mode in range(3):
            assert (T.modes[mode]['seg'].shape[0] + 3) // 4 > 8 * cus, 'the shape no longer gives a workgroup two quads'
            facs = [[f.clone() for f in dfs] for _ in range(2)]
            for stage, f in zip((1, 2), facs):
                ntf._sparse_call(T, f, mode, beta, unstored, step=(0.0, 0.0, mu_gamma(beta)), stage=stage)
            assert torch.equal(facs[0][mode], facs[1][mode]) and not torch.equal(facs[0][mode], dfs[mode])
        got = [float(ntf._sparse_loss(T, dfs, beta, unstored, stage=s).item()) for s in (1, 2)]
        ref, s_abs = ref_loss(V.astype(np.float64), np.ones(shape) if unstored == 'zero' else S.astype(np.float64),
                              [f.astype(np.float64) for f in fs], beta)
        assert got[0] == got[1] and abs(got[0] - ref) <= 2 * (R + 64) * U * s_abs


# (unstored, beta) -> the positive tols at which the float64 margin exceeds the loss bound (test_fit_against_float64)
STOP_TOLS = {('missing', 0.5): (), ('missing', 1): (1e-2,), ('missing', 2): (1e-2,), ('zero', 1): (1e-4, 1e-2),
             ('zero', 2): (1e-4, 1e-2)}


@pytest.mark.parametrize('unstored,beta', [('missing', 0.5), ('missing', 1), ('missing', 2), ('zero', 1), ('zero', 2)])
def test_fit_against_float64(unstored, beta):
    """20 iterations from a fixed start on the planted rank-3 (20, 30, 25) tensor with 70 % stored (under 'zero' the unstored
    entries are zeros of the target): every factor within 1e-4 relative Frobenius of the float64 loop, the loss
    non-increasing within twice its own bound, 20 iterations returned at tol = -1e9.

    The stop rule at a positive tol returns the float64 loop's count where the float64 margin
    ``|(previous - loss) / loss_init - tol|`` exceeds the loss bound at every checkpoint up to the deciding one.  The bound is
    ``2 (3 + 64) 2^-24 S_abs`` carried into the unit of ``sqrt(2 div)`` at both checkpoints of the difference, plus the share
    of ``loss_init``.  Computed on the CPU with ``mu_loop64`` for this seed, smallest margin / bound ratio (margin, bound,
    iterations at the stop; max_iter = 200):
      'missing' 0.5: tol 1e-4 0.003 (3.9e-5, 1.5e-2, no stop), tol 1e-2 0.55 (2.3e-3, 4.1e-3, 80)   -- not asserted
      'missing' 1:   tol 1e-4 0.008 (3.8e-5, 4.7e-3, no stop) -- not asserted; tol 1e-2 3.0 (5.3e-3, 1.8e-3, 60)
      'missing' 2:   tol 1e-4 0.015 (2.6e-5, 1.8e-3, no stop) -- not asserted; tol 1e-2 7.5 (7.9e-4, 1.1e-4, 30)
      'zero' 1:      tol 1e-4 1.7 (4.8e-5, 2.9e-5, 60), tol 1e-2 178 (5.0e-3, 2.8e-5, 20)
      'zero' 2:      tol 1e-4 2.7 (4.1e-5, 1.5e-5, 70), tol 1e-2 505 (7.2e-3, 1.4e-5, 20)
    (under 'missing' the loss of the planted tensor tends to 0 and ``S_abs`` does not; under 'zero' it does not tend to 0)."""
    V, _, start = planted(False)
    S = np.random.default_rng(11).random(V.shape) < 0.7
    V = np.where(S, V, 0).astype(np.float32)
    M = None if unstored == 'zero' else S.astype(np.float32)
    T = ntf.SparseNtfTarget(sparse_of(V, S))
    ref, _, _, _ = mu_loop64(V, M, start, beta, -1e9, 20)
    m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
    assert m.fit(T, beta=beta, tol=-1e9, max_iter=20, unstored=unstored) == 20
    errs = [rel_err(host(f.data), r) for f, r in zip(m.factors, ref)]
    record('sparse_ntf_fit', unstored=unstored, beta=beta, errs=errs)
    assert max(errs) < 1e-4, errs
    m, losses = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda(), []
    for _ in range(20):
        assert m.fit(T, beta=beta, tol=-1e9, max_iter=1, unstored=unstored) == 1
        losses.append(float(ntf._sparse_loss(T, [f.data for f in m.factors], beta, unstored).item()))
    Mn = np.ones(V.shape) if M is None else M.astype(np.float64)
    slack = 2 * (3 + 64) * U * ref_loss(V.astype(np.float64), Mn, ref, beta)[1]
    assert all(b <= a + 2 * slack for a, b in zip(losses, losses[1:])), losses
    for tol in STOP_TOLS[(unstored, beta)]:
        m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
        assert m.fit(T, beta=beta, tol=tol, max_iter=200, unstored=unstored) == mu_loop64(V, M, start, beta, tol, 200)[1], tol
