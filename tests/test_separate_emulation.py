"""tests/separate_emulation.py on the CPU: the float64 reference of ``separation.separate`` against golden g26 (the reference's
own fitted factors and per-group reconstructions), the identities a soft mask obeys, and the host tables."""
import numpy as np
import pytest

import forward_reference as FR
import separate_emulation as SE
from conftest import load_golden


@pytest.fixture(scope='module')
def g26():
    return load_golden('g26_separate')


def _mixture(g, name, kind):
    return {'none': None, 'real': g[f'{name}_Vreal'], 'complex': g[f'{name}_Vcomplex']}[kind]


@pytest.mark.parametrize('name', ['nmf', 'nmfd'])
def test_emulation_matches_golden(g26, name):
    H, W, groups = g26[f'{name}_H'], g26[f'{name}_W'], g26[f'{name}_groups'].tolist()
    assert float(g26['eps']) == SE.EPS
    Y, _, full, _ = SE.group_planes(H, W, groups)
    np.testing.assert_allclose(Y, g26[f'{name}_Y'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(full, g26[f'{name}_full'], rtol=1e-12, atol=1e-12)
    for i in range(int(g26[f'{name}_cases'])):
        want = g26[f'{name}_case{i}_out']
        out, bound = SE.emulate(H, W, _mixture(g26, name, str(g26[f'{name}_case{i}_mixture'])), groups,
                                float(g26[f'{name}_case{i}_power']), g26[f'{name}_case{i}_select'].tolist())
        assert out.shape == want.shape == bound.shape
        np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)
        assert np.all(bound[np.abs(want) > 0] > 0)


@pytest.mark.parametrize('power', [1.0, 2.0, 0.5, 1.7])
def test_masks_sum_to_d_over_d_plus_eps(power):
    H, W = FR.dense_factors((33, 130, 7))
    labels = [0, 1, 0, 2, 1, 2, 0]
    M, _ = SE.emulate(H.numpy(), W.numpy(), None, labels, power)
    Y, _, _, _ = SE.group_planes(H.numpy(), W.numpy(), labels)
    D = (Y ** float(np.float32(power))).sum(0)
    np.testing.assert_allclose(M.sum(0), D / (D + SE.EPS), rtol=1e-13)
    assert M.min() >= 0 and M.max() <= 1


def test_select_returns_the_same_planes():
    H, W = FR.dense_factors((33, 130, 7))
    V = np.random.default_rng(0).standard_normal((33, 130)).astype(np.float32)
    full, fb = SE.emulate(H.numpy(), W.numpy(), V, None, 2.0)
    part, pb = SE.emulate(H.numpy(), W.numpy(), V, None, 2.0, [2, 0, 2])
    assert np.array_equal(part, full[[2, 0, 2]]) and np.array_equal(pb, fb[[2, 0, 2]])


def test_empty_and_all_zero_groups():
    H, W = FR.dense_factors((33, 130, 7))
    H, W = H.numpy().copy(), W.numpy()
    base, _ = SE.emulate(H, W, None, [0, 0, 0, 1, 1, 1, 1], 2.0)
    # an empty label between the two groups: a zero plane, the others unchanged
    gap, gb = SE.emulate(H, W, None, [0, 0, 0, 2, 2, 2, 2], 2.0)
    assert gap.shape[0] == 3 and not gap[1].any() and not gb[1].any()
    assert np.array_equal(gap[[0, 2]], base)
    # a group whose components are all zero in H: a zero plane, and the others are what they are without it
    Hz = np.concatenate([H, np.zeros((33, 2), np.float32)], 1)
    Wz = np.concatenate([W, np.ones((130, 2), np.float32)], 1)
    zero, zb = SE.emulate(Hz, Wz, None, [0, 0, 0, 1, 1, 1, 1, 2, 2], 2.0)
    assert not zero[2].any() and not zb[2].any() and np.array_equal(zero[:2], base)
    # an element where every Y_g is zero: mask exactly 0, never NaN
    H[5] = 0
    M, b = SE.emulate(H, W, None, [0, 0, 0, 1, 1, 1, 1], 0.5)
    assert not M[:, 5].any() and not b[:, 5].any() and np.isfinite(M).all()


def test_tables_on_interleaved_labels():
    labels = SE.normalise([0, 1, 0, 2, 1], 5)
    G, members, cols, gstart = SE.tables(labels)
    assert (G, members, cols, gstart) == (3, [[0, 2], [1, 4], [3]], [0, 2, 1, 4, 3, -1], [0, 2, 4, 6])
    # an odd group in the middle and an empty one: padding keeps every boundary even
    G, members, cols, gstart = SE.tables([3, 0, 0, 0, 3])
    assert (G, members, cols, gstart) == (4, [[1, 2, 3], [], [], [0, 4]], [1, 2, 3, -1, 0, 4], [0, 4, 4, 4, 6])
    assert SE.tables(SE.normalise(None, 3))[2:] == ([0, -1, 1, -1, 2, -1], [0, 2, 4, 6])
    F = np.arange(10, dtype=np.float32).reshape(2, 5)
    P = SE.permuted(F, [0, 2, 1, 4, 3, -1])
    assert np.array_equal(P, np.array([[0, 2, 1, 4, 3, 0], [5, 7, 6, 9, 8, 0]], np.float32))
    assert SE.slots(3, None) == ([0, 1, 2], 3, [])
    assert SE.slots(3, [2, 0, 2]) == ([1, -1, 0], 3, [(2, 0)])


def test_tables_agree_with_the_library():
    from torchnmf_amd import separation as S
    rng = np.random.default_rng(3)
    for _ in range(50):
        R = int(rng.integers(1, 12))
        labels = rng.integers(0, 5, R).tolist()
        assert S.group_tables(S.normalise_groups(labels, R)) == SE.tables(SE.normalise(labels, R))
        G = max(labels) + 1
        sel = rng.integers(0, G, int(rng.integers(0, 6))).tolist()
        assert S.slot_table(G, sel) == SE.slots(G, sel)


def test_check_flags_one_bad_element():
    H, W = FR.dense_factors((33, 130, 7))
    out, bound = SE.emulate(H.numpy(), W.numpy(), None, None, 1.7)
    got = out.astype(np.float32)
    assert SE.check(got, out, bound, 'fp32 rounding of the reference') < 1.0
    bad = got.copy()
    bad[3, 7, 11] *= 1 + 2e-4
    with pytest.raises(AssertionError):
        SE.check(bad, out, bound, 'seeded fault')
    bad = got.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        SE.check(bad, out, bound, 'seeded NaN')
