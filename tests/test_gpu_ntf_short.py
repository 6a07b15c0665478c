"""The 32-row NTF tile (``tile='short'``, csrc/nmfmu_ntf_short.hip) against the float64 references of ``test_gpu_ntf``: terms
and step per element, agreement with the 128-row tile, the fit, and the ``tile`` argument.

The bound is ``test_gpu_ntf``'s: ``2 (R + L + 64) 2^-24`` relative, ``L`` the mode's contraction length.  It holds for any
summation order of non-negative summands, so it is this kernel's too, whose waves split a stage along the contraction.

The shapes, with WS = 4 / 2 / 1 waves of 32 steps per stage at r_pad 32 / 128 / 256 (R = 3 / 100 / 200): owner modes of 2 .. 8
rows (one partly filled tile), 33 and 36 (a second tile of 1 / 4 rows), 129 and 131 (five tiles, the last partial); a
contraction of 15 (one wave busy), of 66 and 198 (the last stage ends inside wave 2's steps at WS = 4, and is a lone wave or a
short second wave at WS = 2), of 393 .. 4644 (several stages, unequal parts under nsplit = 3 for every WS); a last dimension
of 2 (sixteen slices inside a wave's 32 steps), of 131 and 11 (slice ends inside the 32-lane runs of the INNER walk; in mode 2
K = 131 and 11 refuse the 16-byte loads of the OUTER walk, K = 36 takes them on whole quads and K = 2 has none)."""
import functools

import numpy as np
import pytest
import torch

from conftest import record, rel_err
from test_gpu_ntf import U, dev, host, mu_loop64, planted, problem, ref_terms, ref_update
from torchnmf_amd import _capi, ntf
from torchnmf_amd.engine import mu_gamma

pytestmark = pytest.mark.gpu
SHAPES = [(3, 5, 131), (33, 6, 11), (7, 70, 2), (8, 129, 36)]


@functools.lru_cache(maxsize=None)
def refs(shape, R, beta, weighted):
    """float64 (num, den) per mode, once per problem: shared by the cases that differ in nsplit or in what they compare."""
    fs, V, M, _, _ = problem(shape, R)
    Md = M.astype(np.float64) if weighted else np.ones(shape)
    return [ref_terms(V.astype(np.float64), Md, [f.astype(np.float64) for f in fs], mode, beta) for mode in range(3)]


def target(shape, R, weighted):
    fs, V, M, Vj, dead = problem(shape, R)
    return ntf.NtfTarget(dev(Vj if weighted else V), dev(M) if weighted else None), [dev(f) for f in fs]


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('nsplit', (1, 3))
@pytest.mark.parametrize('beta', (-1, 0, 0.5, 1, 2, 3))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', SHAPES)
def test_terms_and_step(shape, R, beta, nsplit, weighted):
    fs, V, _, _, dead = problem(shape, R)
    T, dfs = target(shape, R, weighted)
    gamma, worst = mu_gamma(beta), {}

    def within(got, ref, bound, what):
        assert np.isfinite(got).all(), what
        err = np.abs(got - ref)
        assert (err <= bound * ref).all(), (what, float((err / np.maximum(bound * ref, 1e-300)).max()))
        worst[what] = max(worst.get(what, 0.0), float((err[ref > 0] / (bound * ref[ref > 0])).max()))

    for mode in range(3):
        bound = 2 * (R + V.size // shape[mode] + 64) * U
        ref = refs(shape, R, beta, weighted)[mode]
        got = ntf._ntf_call(T, dfs, mode, beta, nsplit=nsplit, _fill=float('nan'), tile='short')
        again = ntf._ntf_call(T, dfs, mode, beta, nsplit=nsplit, _fill=7.0, tile='short')
        for g, a, r, what in zip(got, again, ref, ('num', 'den')):
            assert torch.equal(g, a), 'a repeated call is bitwise identical whatever the workspace held'
            g = host(g)
            assert (g[:, R:] == 0).all(), 'padded rank columns'
            within(g[:, :R], r, bound, what)
            assert not weighted or (g[dead[mode]] == 0).all(), 'the weightless owner row'
        for l1, l2 in ((0.0, 0.0), (0.021, 0.049)):
            facs = [f.clone() for f in dfs]
            ntf._ntf_call(T, facs, mode, beta, step=(l1, l2, gamma), nsplit=nsplit, _fill=float('nan'), tile='short')
            within(host(facs[mode]), ref_update(fs[mode].astype(np.float64), *ref, gamma, l1, l2), bound * max(1, gamma), 'step')
            assert all(torch.equal(facs[n], dfs[n]) for n in range(3) if n != mode), 'the panel factors are untouched'
            if weighted and l1 == 0:
                assert torch.equal(facs[mode][dead[mode]], dfs[mode][dead[mode]]), 'a weightless row keeps its bits'
    record('ntf_short_terms_step', shape=shape, R=R, beta=beta, nsplit=nsplit, weighted=weighted, **worst)


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('beta', (-1, 1, 2))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', SHAPES)
def test_the_two_tiles_agree(shape, R, beta, weighted):
    """Each tile is within its bound of float64, so they differ by at most the sum of the two (equal) bounds."""
    T, dfs = target(shape, R, weighted)
    for mode in range(3):
        bound = 2 * (R + np.prod(shape) // shape[mode] + 64) * U
        short = ntf._ntf_call(T, dfs, mode, beta, nsplit=3, tile='short')
        wide = ntf._ntf_call(T, dfs, mode, beta, nsplit=3, tile='wide')
        for s, w, ref in zip(short, wide, refs(shape, R, beta, weighted)[mode]):
            assert (np.abs(host(s) - host(w))[:, :R] <= 2 * bound * ref).all(), mode


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('beta', (0.5, 1, 2))
def test_fit_against_float64(beta, weighted):
    """20 iterations on the short tile from the same start: every factor within 1e-4 relative Frobenius of the float64 loop."""
    V, M, start = planted(weighted)
    m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
    assert m.fit(dev(V), beta=beta, tol=-1e9, max_iter=20, weights=None if M is None else dev(M), tile='short') == 20
    errs = [rel_err(host(f.data), r) for f, r in zip(m.factors, mu_loop64(V, M, start, beta, -1e9, 20)[0])]
    record('ntf_short_fit', beta=beta, weighted=weighted, errs=errs)
    assert max(errs) < 1e-4, errs


def test_tile_argument():
    V, _, start = planted(False)
    m = ntf.NTF(factors=[torch.from_numpy(f) for f in start]).cuda()
    with pytest.raises(ValueError, match='tile'):
        m.fit(dev(V), tile='banana')
    with pytest.raises(ValueError, match='tile'):
        ntf.ntf_terms(dev(V), None, [f.data for f in m.factors], 0, 1, tile='banana')
    with pytest.raises(NotImplementedError, match='sparse'):
        m.fit(dev(V).to_sparse(), unstored='missing', tile='short')
    lib = _capi.load()
    assert lib.nmfmu_ntf_tile(8, 1025 * 8192, 32) == 1 and lib.nmfmu_ntf_tile(128, 8 * 8192, 32) == 0
    assert lib.nmfmu_ntf_tile(8, 2048, 32) == 0, 'a short contraction is launch-bound on either tile: the wide one stays'
    # tile=None asks nmfmu_ntf_tile per mode: the 8-row mode over 65536 steps takes the short entries, the other two the wide
    assert [lib.nmfmu_ntf_tile(d, 8 * 256 * 256 // d, 32) for d in (8, 256, 256)] == [1, 0, 0]
    Vd = torch.rand(8, 256, 256, device='cuda') + 0.1
    fs = [torch.rand(d, 5, device='cuda') + 0.25 for d in Vd.shape]
    for mode, forced in enumerate(('short', 'wide', 'wide')):
        for a, b in zip(ntf.ntf_terms(Vd, None, fs, mode, 1), ntf.ntf_terms(Vd, None, fs, mode, 1, tile=forced)):
            assert torch.equal(a, b), mode
