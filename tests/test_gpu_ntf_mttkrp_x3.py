"""The split-bf16 MTTKRP (``precision='bf16x3'``) on the device: per element against float64 numpy at the shapes of
test_gpu_ntf_hals (a second row tile in either arrangement, octets that straddle slices, misaligned rows, part tails shorter
than a stage, contractions shorter than a short stage, every r_pad), then ``NTF.fit(solver='hals', precision='bf16x3')`` against
the chain of its public pieces and its objective in float64.

The bound, derived and not measured.  bf16 keeps 8 significant bits, so ``|x - hi| <= 2^-9 |x|`` and ``|x - hi - lo| <= 2^-9 |lo|
<= 2^-18 |x|``: each operand is held to 2^-18 relative by its two planes.  The three products formed are ``(hi + lo)(hi' + lo') -
lo lo'``: two operand errors (2 * 2^-18 + 2^-36) and the dropped ``|lo lo'| <= 2^-18 x x'`` give ``3 * 2^-18 (1 + 2^-8)`` per
product at most.  All ``x x'`` are non-negative and the lo terms are at most 2^-8 of them in size, so the fp32 accumulation of
the 3 L terms, the rounding of ``fl32(Pa Pb)``, the sum over parts and waves and the finish add ``(3 L + 64) 2^-24`` whatever the
order (L: the mode's contraction length).  Asserted with the project's factor 2.  A kernel that loses a lo term errs by 2^-9."""
import numpy as np
import pytest
import torch

from conftest import record
from test_gpu_ntf import U, dev, host, planted, problem
from test_gpu_ntf_hals import SHAPES, loss64, reference
from torchnmf_amd import _capi, hals, ntf
from torchnmf_amd.constants import eps

pytestmark = pytest.mark.gpu
X3 = {'precision': 'bf16x3'}


def bound(L):
    return 2 * (3 * 2.0 ** -18 * (1 + 2.0 ** -8) + (3 * L + 64) * U)


@pytest.mark.parametrize('mode', (0, 1, 2))
@pytest.mark.parametrize('nsplit', (1, 3))
@pytest.mark.parametrize('R', (3, 100, 200))
@pytest.mark.parametrize('shape', SHAPES)
def test_mttkrp_x3_against_float64(shape, R, nsplit, mode):
    fs, V = problem(shape, R)[:2]
    T, dfs, ref = ntf.NtfTarget(dev(V)), [dev(f) for f in fs], reference(shape, R)[mode]
    b = bound(V.size // shape[mode])
    got, worst = {}, {}
    for tile in ('wide', 'short'):
        g = ntf._mttkrp_call(T, dfs, mode, nsplit=nsplit, tile=tile, _fill=float('nan'), **X3)
        again = ntf._mttkrp_call(T, dfs, mode, nsplit=nsplit, tile=tile, _fill=7.0, **X3)
        assert torch.equal(g, again), 'a repeated call is bitwise identical whatever the workspace and the output held'
        g = host(g)
        assert g.shape == (shape[mode], _capi.load().nmfmu_pad_rank(R)) and (g[:, R:] == 0).all(), 'padded rank columns'
        got[tile] = g[:, :R]
        worst[tile] = float((np.abs(got[tile] - ref) / (b * ref)).max())
        print(shape, R, nsplit, mode, tile, worst[tile])
        assert worst[tile] <= 1, (tile, worst[tile])
    assert (np.abs(got['wide'] - got['short']) <= 2 * b * ref).all()
    record('ntf_mttkrp_x3', shape=shape, R=R, nsplit=nsplit, mode=mode, **worst)


@pytest.mark.parametrize('case', ('dense', 'frozen'))
def test_one_iteration_is_the_chain_of_public_pieces(case):
    V, _, start = planted(False)
    Vd = dev(V)
    train = (True, False, True) if case == 'frozen' else (True, True, True)
    alpha, l1_ratio = 0.07, 0.3
    m = ntf.NTF(factors=[torch.from_numpy(s) for s in start], trainable=train).cuda()
    assert m.fit(Vd, beta=2, tol=-1e9, max_iter=1, solver='hals', alpha=alpha, l1_ratio=l1_ratio, **X3) == 1
    fs, lib, R = [dev(s) for s in start], _capi.load(), start[0].shape[1]
    numerator = lambda n: ntf.ntf_mttkrp(Vd, fs, n, **X3)      # noqa: E731
    g = [ntf._gram(lib, f).double() for f in fs]
    a = float((numerator(0)[:, :R].double() * fs[0].double()).sum().item()) / float((g[0] * g[1] * g[2]).sum().item())
    assert a > 0
    for f, on in zip(fs, train):
        if on:
            f.mul_(a ** (1.0 / sum(train))).clamp_(min=eps)
    for n in range(3):
        if train[n]:
            pa, pb = (f for k, f in enumerate(fs) if k != n)
            hals.hals_sweep(fs[n], numerator(n), (ntf._gram(lib, pa) * ntf._gram(lib, pb)).view(R, R), alpha * l1_ratio,
                            alpha * (1 - l1_ratio))
    assert all(torch.equal(f.data, c) for f, c in zip(m.factors, fs))
    assert not all(torch.equal(numerator(n), ntf.ntf_mttkrp(Vd, fs, n)) for n in range(3)), 'the fp32 kernel answered'


def test_objective_never_increases_and_loss_matches():
    """Ten iterations, one ``fit`` each: the float64 loss on the host never rises by more than ``bound * 1/2 |V|^2`` (a perturbed
    coordinate step can raise it only in second order of the bound).  The loss ``fit`` tracks is ``1/2 |V|^2 - <V, Y> + 1/2 <Y, Y>``
    with ``<V, Y>`` from the bf16x3 numerator of mode 0: within ``bound * <V, Y>_64`` of the float64 loss at the two points where
    test_gpu_ntf_hals asserts its premise (the residual exceeds a tenth of 1/2 |V|^2).  ``bound`` at mode 0's contraction length,
    the longest of the three."""
    V, _, start = planted(False)
    Vd, b = dev(V), bound(V.size // min(V.shape))
    half_v2 = 0.5 * float((V.astype(np.float64) ** 2).sum())
    m = ntf.NTF(factors=[torch.from_numpy(s) for s in start]).cuda()
    trace = []
    for _ in range(10):
        assert m.fit(Vd, beta=2, tol=-1e9, max_iter=1, solver='hals', **X3) == 1
        trace.append(loss64(V, [f.data for f in m.factors]))
    worst_rise = float(np.diff(trace).max()) / half_v2
    print('worst rise / half_v2', worst_rise, 'bound', b)
    assert worst_rise <= b, trace
    fs = [dev(s) for s in start]
    eng = ntf._HalsNtf(ntf.NtfTarget(Vd), fs, (True, True, True), 0.0, 0.0, precision='bf16x3')
    errs = []
    for half_step in (None, 0):
        if half_step is not None:
            eng.half_step(half_step)
        got, ref = eng.divergence(), loss64(V, fs)
        vy = float(np.einsum('ijk,ir,jr,kr->', V.astype(np.float64), *[host(f) for f in fs]))
        assert ref > 0.1 * half_v2, 'the premise of the tolerance'
        errs.append(abs(got - ref) / vy)
        print('loss deviation / <V, Y>', errs[-1], 'bound', b)
        assert errs[-1] <= b, (got, ref)
    record('ntf_hals_x3_objective', worst_rise_over_half_v2=worst_rise, loss_deviation_over_vy=errs, bound=b)
