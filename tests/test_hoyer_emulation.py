"""The float64 restatement of the Hoyer projection (tests/hoyer_emulation.py) against the reference's own results
(g15_hoyer_proj: s = |randn|, sigma in {0.2, 0.4, 0.8} x n in {2 .. 5000}), and the constraints it must meet on exit.

Bound per case: 4 x e_ref, the reference's own fp32 error against a float64 run of the same function, stored with the case
(the generator refuses a case whose e_ref is 0)."""
import numpy as np
import pytest

from conftest import load_golden
from hoyer_emulation import project, project_slice

G = load_golden('g15_hoyer_proj')
CASES = list(range(len(G['n'])))


@pytest.mark.parametrize('i', CASES)
def test_restatement_matches_reference(i):
    s, ref = G[f's_{i}'], G[f'p_{i}'].astype(np.float64)
    v, passes = project_slice(s, G['k1'][i], G['k2'][i])
    err = np.linalg.norm(v - ref) / np.linalg.norm(ref)
    bound = 4 * float(G['e_ref'][i])
    print(f"n={int(G['n'][i])} sigma={float(G['sigma'][i])} passes={passes} err={err:.2e} bound={bound:.2e}")
    assert err <= bound, (err, bound)
    assert np.array_equal(v == 0, ref == 0), 'zero pattern differs from the reference'
    assert 1 <= passes <= len(s)


@pytest.mark.parametrize('i', CASES)
def test_constraints_hold_on_exit(i):
    k1, k2 = float(G['k1'][i]), float(G['k2'][i])
    v, _ = project_slice(G[f's_{i}'], k1, k2)
    assert (v >= 0).all()
    assert abs(v.sum() - k1) <= 1e-12 * k1
    assert abs((v * v).sum() - k2) <= 1e-12 * k2
    n, sigma = len(v), float(G['sigma'][i])
    if n > 1:                   # Hoyer's sparseness of the result is the sigma the targets were built from (fp32-rounded)
        sp = (n ** 0.5 - v.sum() / np.sqrt((v * v).sum())) / (n ** 0.5 - 1)
        assert abs(sp - sigma) <= 1e-6


def test_batched_form_slices_along_dim():
    """project() walks any dim and gives each slice its own targets."""
    rng = np.random.default_rng(0)
    x = np.abs(rng.standard_normal((5, 3, 4)))
    nrm = np.sqrt((x * x).sum(axis=(0, 2)))
    k1, k2 = (20 ** 0.5 * 0.6 + 0.4) * nrm, nrm ** 2
    out, passes = project(x, k1, k2, dim=1)
    for j in range(3):
        v, p = project_slice(x[:, j, :].reshape(-1), k1[j], k2[j])
        assert np.array_equal(out[:, j, :].reshape(-1), v) and passes[j] == p


def test_degenerate_slices_return():
    """n = 1, an all-zero slice and k2 = 0 end (possibly in NaN), never loop."""
    for s, k1, k2 in (([3.0], 1.0, 1.0), (np.zeros(7), 2.0, 1.0), (np.ones(5), 1.0, 0.0)):
        v, passes = project_slice(s, k1, k2)
        assert v.shape == (len(s),) and 1 <= passes <= len(s)
