"""The float64 reference of PLCA on sparse targets (tests/sparse_plca_emulation.py) checked on the CPU:

1. its numerators are the dense ones (``plca_emulation.dense_numerators`` on the densified target) and its regrouped loss is the
   dense loss -- the iteration is exactly sparse;
2. a float64 ``fit`` built from it lands on the reference's recorded runs (golden g21) within 1e-9: two float64
   implementations of the same iterations (measured: 9e-16 at worst);
3. the bounds are what the module says they are (counts read off the pattern, zero where nothing is stored).
"""
import numpy as np
import pytest

import masked_emulation as M
import plca_emulation as P
import sparse_plca_emulation as S
from conftest import load_golden, rel_err

N, C = 37, 29
G21 = load_golden('g21_sparse_plca')
CASES = {'plain': {}, 'prior': dict(alphas=(1.02, 0.99, 1.01)), 'frozenZ': dict(train=(True, True, False)),
         'frozenW': dict(train=(False, True, True)), 'stop': dict(tol=1e-3, max_iter=200)}
NO_STOP = -1e9


@pytest.mark.parametrize('R', [3, 33, 100, 200])
@pytest.mark.parametrize('axis', [0, 1])
def test_sparse_numerators_and_loss_are_the_dense_ones(R, axis):
    idx, vn, W, H, Z = S.make_problem(N, C, R, axis)
    assert abs(float(vn.sum(dtype=np.float64)) - 1) < 1e-6 and np.allclose(W.sum(0), 1, atol=1e-5)
    t = S.estep(idx, vn, (N, C), H, W, Z)
    Vn, Mk = S.dense(idx, vn, (N, C))
    numW, numH = P.dense_numerators(Vn, W, H, Z)
    assert np.abs(t['num_w'] - numW).max() <= 1e-13 * np.abs(numW).max()
    assert np.abs(t['num_h'] - numH).max() <= 1e-13 * np.abs(numH).max()
    # the gather from the float64 g is the same plane
    nw, _, count = S.gather(idx, t['g'], (N, C), H)
    assert np.abs(nw - numW).max() <= 1e-13 * np.abs(numW).max() and np.array_equal(count, Mk.sum(0))
    # nothing stored: value and bound exactly 0
    for num, b, cnt in ((t['num_h'], t['num_h_bound'], t['count_h']), (t['num_w'], t['num_w_bound'], t['count_w'])):
        assert (cnt == 0).any() and np.all(num[cnt == 0] == 0) and np.all(b[cnt == 0] == 0) and np.all(b[cnt > 0] > 0)
    got, bound = S.loss(idx, vn, (N, C), H, W, Z)
    want = S.dense_loss(idx, vn, (N, C), H, W, Z)
    assert abs(got - want) <= 1e-12 * max(abs(want), 1.0) and 0 < bound < 1e-4 * abs(want)


def test_bound_counts_come_from_the_pattern():
    idx, vn, W, H, Z = S.make_problem(N, C, 200, 0)
    assert S.g_ops(3) == 11 and S.g_ops(33) == 11 and S.g_ops(100) == 12 and S.g_ops(200) == 14
    whole, split = S.estep(idx, vn, (N, C), H, W, Z, 512), S.estep(idx, vn, (N, C), H, W, Z, 8)
    cnt = whole['count_h']
    assert sorted(set(cnt.tolist())) == sorted(M.COUNTS)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = split['num_h_bound'] / whole['num_h_bound']
    segs = S.segments(cnt, 8)
    want = (cnt + segs + 14) / (cnt + 1 + 14)
    assert np.allclose(ratio[cnt > 0], np.broadcast_to(want[:, None], ratio.shape)[cnt > 0])
    assert np.array_equal(segs[cnt == 20], np.full((cnt == 20).sum(), 3)) and np.all(segs[cnt == 8] == 1)
    # g: relative, per entry
    assert np.allclose(whole['g_bound'], S.SECOND * 14 * S.U * whole['g'])
    # the gather's own bound leaves the roundings of g out
    _, b, c = S.gather(idx, whole['g'], (N, C), H, 8)
    k_full = c + S.segments(c, 8) + 14
    k_own = c + S.segments(c, 8)
    sel = c > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = b / split['num_w_bound']
    assert np.allclose(ratio[sel], np.broadcast_to((k_own / k_full)[:, None], b.shape)[sel])
    assert S.chain_rank_sums(37) == 16 and S.chain_rank_sums(1 << 14) == 19 and S.chain_rank_sums(65536) == 21


@pytest.mark.parametrize('name', list(CASES))
def test_float64_fit_meets_golden_g21(name):
    g = G21
    kw = dict(CASES[name])
    kw.setdefault('tol', NO_STOP)
    kw.setdefault('max_iter', 30)
    shape = tuple(int(x) for x in g['shape'])
    W, H, Z, n, norm, losses = S.fit(g['indices'], g['values'], shape, g['W_init'], g['H_init'], g['Z_init'], **kw)
    assert n == int(g[f'{name}_n']) and norm == float(g[f'{name}_norm'])
    errs = [rel_err(a, g[f'{name}_{k}']) for a, k in ((W, 'W'), (H, 'H'), (Z, 'Z'))]
    print(f'g21 {name}: float64 fit against the reference W {errs[0]:.1e} H {errs[1]:.1e} Z {errs[2]:.1e}')
    assert max(errs) < 1e-9, errs
    assert np.allclose(losses, g[f'{name}_losses'], rtol=1e-9, atol=0)
    if name == 'frozenW':
        assert np.array_equal(W, np.asarray(g['W_init'], dtype=np.float64))
