"""tests/trainer_emulation.py on the CPU: it is the oracle's algorithm, its bounds hold the honest fp32 computation, and a
seeded kernel mistake leaves them.

1. The float64 formulas agree with ``oracle.mu_oracle.betamu_terms`` / ``betamu_update`` / ``betamu_step`` /
   ``betamu_chain_step`` to float64 rounding and reproduce the g7 and g12 goldens at the tolerances of
   tests/test_oracle_golden.py.
2. A plain ``np.float32`` emulation of every kernel, in its operation order, stays inside every bound on the inputs the
   GPU tests use (tests/test_gpu_trainer_parity.py draws them from the same generators).  The worst error / bound ratio of
   each family is printed and must be <= 1; DESIGN.md section 9 quotes them.
3. Each mistake of ``UPDATE_FAULTS`` / ``MATMUL_FAULTS`` / ``gp_raw_kl``, applied to the emulation, leaves a bound or breaks
   the bit-equality of ``grad`` on at least one of those inputs.

The one-layer cases take their (neg, pos) from float64 products rounded to fp32 here; on the GPU they are the device's own
slab sums.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import mu_oracle as O
import trainer_emulation as T

t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
PEN = T.PENALTIES
F64_TOL = 1e-12       # float64 rounding of a few dozen operations (sums of up to 130 terms)


def _close(a, b, tol=F64_TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.abs(b), np.abs(b).max() * 1e-6 + 1e-300)
    return bool((np.abs(a - b) <= tol * scale).all())


# ---- 1. the oracle and the goldens ------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', T.TERMS_BETAS)
def test_terms_agree_with_oracle(beta):
    s, v = T.terms_problem(257)
    gn, gp = T.terms(s, v, beta)
    on, op = O.betamu_terms(t64(v), t64(s), beta)
    assert _close(gn, on.numpy()) and _close(gp, op.numpy())


def test_gamma_is_the_engines():
    from torchnmf_amd.engine import mu_gamma
    for beta in (-1, 0, 0.5, 1, 1.5, 2, 3):
        assert T.mu_gamma(beta) == T.f32(mu_gamma(float(beta))) and abs(T.mu_gamma(beta) - O.gamma_of(beta)) <= T.U


@pytest.mark.parametrize('pen', list(PEN))
@pytest.mark.parametrize('beta', T.UPDATE_BETAS)
def test_update_agrees_with_oracle(beta, pen):
    theta, neg, pos = T.update_problem(5, 257)
    gamma = O.gamma_of(beta)
    new, grad = T.update(theta, neg, pos, gamma, *PEN[pen])
    onew, ograd = O.betamu_update(t64(theta), t64(neg), t64(pos), gamma, *PEN[pen])
    # (the row of one large and many tiny values: rowsum - theta cancels nine digits, and the two float64 sums run in
    # different orders)
    assert _close(new, onew.numpy(), 1e-9 if PEN[pen][2] else F64_TOL) and np.array_equal(grad, ograd.numpy())


@pytest.mark.parametrize('pen', ['off', 'all'])
@pytest.mark.parametrize('beta', [0, 0.5, 1, 2, 3])
def test_one_layer_step_agrees_with_oracle(beta, pen):
    """One layer is a chain of length one: X0 = H, W1 = W."""
    V, W, H = T.fused_problem(T.FUSED_CASES[4])
    for which, name in ((1, 'W'), (0, 'H')):
        got = T.chain_step(V, H, [W], which, beta, *PEN[pen], gamma=O.gamma_of(beta))
        Wn, Hn, grads = O.betamu_step(t64(V), t64(W), t64(H), beta, *PEN[pen], params=(name,))
        assert _close(got['new'], (Wn if name == 'W' else Hn).numpy())
        assert _close(got['grad'], grads[name].numpy(), 1e-9)      # a difference: on the scale of the largest entry


@pytest.mark.parametrize('pen', T.CHAIN_PENS)
@pytest.mark.parametrize('beta', T.CHAIN_BETAS)
def test_chain_step_agrees_with_oracle(beta, pen):
    V, X0, Ws = T.chain_problem()
    for which, name in enumerate(('X0', 'W1', 'W2', 'W3')):
        got = T.chain_step(V, X0, Ws, which, beta, *PEN[pen], gamma=O.gamma_of(beta))
        X0n, Wsn, grads = O.betamu_chain_step(t64(V), t64(X0), [t64(W) for W in Ws], beta, *PEN[pen], order=[name])
        want = X0n if which == 0 else Wsn[which - 1]
        assert _close(got['new'], want.numpy()) and _close(got['grad'], grads[name].numpy(), 1e-9)


G7_PEN = {'plain': (0.0, 0.0, 0.0), 'pen': (1e-3, 1e-3, 1e-2)}


@pytest.mark.parametrize('case', [str(c) for c in load_golden('g7_betamu')['cases']])
def test_reproduces_g7(case):
    g = load_golden('g7_betamu')
    b, pen, which = case.split('_')
    beta = float(b[1:])
    params = ('W', 'H') if which == 'both' else (which,)
    V, W, H = (g[k].astype(np.float64) for k in ('V', 'W0', 'H0'))
    for it in range(1, 6):
        grads = {}
        for n in params:
            r = T.chain_step(V, H, [W], 1 if n == 'W' else 0, beta, *G7_PEN[pen])
            grads[n] = r['grad']
            if n == 'W':
                W = r['new']
            else:
                H = r['new']
        if it in (1, 5):
            assert rel_err(W, g[f'{case}_W{it}']) < 2e-6 and rel_err(H, g[f'{case}_H{it}']) < 2e-6
        if it == 1:
            for n in params:
                if f'{case}_grad{n}1' in g:
                    assert rel_err(grads[n], g[f'{case}_grad{n}1']) < 2e-6


@pytest.mark.parametrize('pen', ['plain', 'pen'])
@pytest.mark.parametrize('beta', [0.5, 1, 2])
def test_reproduces_g12(beta, pen):
    g = load_golden('g12_betamu_chain')
    V, X0 = g['V'].astype(np.float64), g['H1'].astype(np.float64)
    Ws = [g[k].astype(np.float64) for k in ('W1', 'W2', 'W3')]
    for it in range(1, 6):
        for which in (1, 0, 2, 3):                   # torch's parameter order: 0.W, 0.H, 1.W, 2.W
            r = T.chain_step(V, X0, Ws, which, beta, *G7_PEN[pen])
            if which == 0:
                X0 = r['new']
            else:
                Ws[which - 1] = r['new']
        if it in (1, 5):
            for pn, a in (('W1', Ws[0]), ('H1', X0), ('W2', Ws[1]), ('W3', Ws[2])):
                assert rel_err(a, g[f'b{beta}_{pen}_{pn}_{it}']) < 1e-4
    assert rel_err(r['grad'], g[f'b{beta}_{pen}_gradW3']) < 1e-3


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------
def _update_inputs():
    """(tag, theta, neg, pos, beta, pen) of every nmfmu_trainer_update case (70000 x 3 with two penalty sets only: the CPU
    suite stays quick; the GPU test runs them all)."""
    for rows, cols in T.UPDATE_SHAPES:
        theta, neg, pos = T.update_problem(rows, cols)
        for beta in T.UPDATE_BETAS:
            for pen in (PEN if rows < 1000 else ('off', 'all')):
                yield f'{rows}x{cols}-b{beta:g}-{pen}', theta, neg, pos, beta, pen


_fused_cache = {}


def _fused_inputs(case, which):
    """(theta, neg, pos) of one parameter of a one-layer case: float64 contractions rounded to fp32 (the GPU test reads
    the device's slab sums instead); beta == 1 takes the other factor's column sums, as the kernel does."""
    key = (case['id'], which)
    if key not in _fused_cache:
        V, W, H = (a.astype(np.float64) for a in T.fused_problem(case))
        gn, gp = T.terms(H @ W.T, V, case['beta'])
        own, other = (W, H) if which == 'W' else (H, W)
        G = (lambda x: x.T) if which == 'W' else (lambda x: x)
        neg = (G(gn) @ other).astype(T.F32)
        pos = other.sum(0).astype(T.F32) if case['beta'] == 1.0 else (G(gp) @ other).astype(T.F32)
        _fused_cache[key] = (own.astype(T.F32), neg, pos)
    return _fused_cache[key]


def _apply_f32(case, which, fault=None):
    theta, neg, pos = _fused_inputs(case, which)
    return T.update_f32(theta, neg, pos, T.mu_gamma(case['beta']), *PEN[case['pen']], rowsum_fn=T.rowsum_apply_f32,
                        fault=fault, pad=4, rs_pad=32 if case['R'] <= 32 else (64 if case['R'] <= 64 else (128 if case['R'] <= 128 else 256)))


def _apply_ratio(case, which, fault=None):
    theta, neg, pos = _fused_inputs(case, which)
    gamma, pen = T.mu_gamma(case['beta']), PEN[case['pen']]
    new, grad = _apply_f32(case, which, fault)
    ref, _ = T.update(theta, neg, pos, gamma, *pen)
    bound = T.update_bound(theta, neg, pos, gamma, *pen, c_rs=T.rowsum_ops_apply(case['R']))
    return T.worst_ratio(new, ref, bound), np.array_equal(grad, T.grad_f32(neg, pos), equal_nan=True)


def _update_ratio(theta, neg, pos, beta, pen, fault=None):
    gamma = T.mu_gamma(beta)
    new, grad = T.update_f32(theta, neg, pos, gamma, *PEN[pen], fault=fault)
    ref, _ = T.update(theta, neg, pos, gamma, *PEN[pen])
    bound = T.update_bound(theta, neg, pos, gamma, *PEN[pen], c_rs=T.rowsum_ops_update(theta.shape[1]))
    return T.worst_ratio(new, ref, bound), np.array_equal(grad, T.grad_f32(neg, pos), equal_nan=True)


# ---- 2. the honest fp32 computation stays inside the bounds ---------------------------------------------------------------
def test_fp32_update_within_bound():
    worst = 0.0
    for tag, theta, neg, pos, beta, pen in _update_inputs():
        ratio, grad_ok = _update_ratio(theta, neg, pos, beta, pen)
        assert ratio <= 1.0 and grad_ok, (tag, ratio, grad_ok)
        worst = max(worst, ratio)
    print(f'trainer_update fp32 emulation: worst error / bound = {worst:.3f}')
    assert worst <= 1.0


def test_fp32_apply_within_bound():
    worst = 0.0
    for case in T.FUSED_CASES:
        for which in ('W', 'H'):
            ratio, grad_ok = _apply_ratio(case, which)
            assert ratio <= 1.0 and grad_ok, (case['id'], which, ratio, grad_ok)
            worst = max(worst, ratio)
    print(f'trainer apply fp32 emulation: worst error / bound = {worst:.3f}')
    assert worst <= 1.0


def test_fp32_terms_within_bound():
    worst = 0.0
    for n in T.TERMS_SIZES:
        s, v = T.terms_problem(n)
        for beta in T.TERMS_BETAS:
            gn, gp = T.terms_f32(s, v, beta)
            rn, rp = T.terms(s, v, beta)
            bn, bp = T.terms_bound(s, v, beta)
            ratio = max(T.worst_ratio(gn, rn, bn), T.worst_ratio(gp, rp, bp))
            assert ratio <= 1.0, (n, beta, ratio)
            if beta == 2:
                assert np.array_equal(gn, v) and np.array_equal(gp, s)
            if beta == 1:
                assert bool((gp == 1.0).all())
            worst = max(worst, ratio)
    print(f'mu_terms fp32 emulation: worst error / bound = {worst:.3f}')
    assert worst <= 1.0


def test_fp32_matmul_within_bound():
    worst = 0.0
    for M, K in T.RECON_MK:
        for R in T.RECON_R:
            A, B = T.recon_problem(M, K, R)
            ratio = T.worst_ratio(T.matmul_f32(A, B), T.matmul(A, B), T.matmul_bound(A, B))
            assert ratio <= 1.0, (M, K, R, ratio)
            worst = max(worst, ratio)
            A, B = T.recon_problem(M, K, R, one_hot=True)
            assert np.array_equal(T.matmul_f32(A, B), B[:, T.one_hot_rank(M, K, R)].T)
    print(f'reconstruct fp32 emulation: worst error / bound = {worst:.3f}')
    assert worst <= 1.0


def test_fp32_chain_within_bound():
    V, X0, Ws = T.chain_problem()
    worst, worst_g = 0.0, 0.0
    for beta in T.CHAIN_BETAS:
        for pen in T.CHAIN_PENS:
            for which in range(4):
                ref = T.chain_step(V, X0, Ws, which, beta, *PEN[pen])
                new, grad = T.chain_step_f32(V, X0, Ws, which, beta, *PEN[pen])
                ratio, rg = T.worst_ratio(new, ref['new'], ref['bound']), T.worst_ratio(grad, ref['grad'], ref['grad_bound'])
                assert ratio <= 1.0 and rg <= 1.0, (beta, pen, which, ratio, rg)
                worst, worst_g = max(worst, ratio), max(worst_g, rg)
    print(f'chain step fp32 emulation: worst error / bound = {worst:.3f} (new), {worst_g:.3f} (grad)')
    assert worst <= 1.0 and worst_g <= 1.0


# ---- 3. seeded faults ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fault', T.UPDATE_FAULTS)
def test_update_fault_is_caught(fault):
    """On trainer_update_kernel's inputs and on the apply kernel's: each mistake leaves the bound or changes ``grad``."""
    caught_u = caught_a = False
    for tag, theta, neg, pos, beta, pen in _update_inputs():
        if theta.shape[0] > 1000:
            continue
        ratio, grad_ok = _update_ratio(theta, neg, pos, beta, pen, fault)
        if ratio > 1.0 or not grad_ok:
            caught_u = True
            break
    for case in T.FUSED_CASES:
        for which in ('W', 'H'):
            ratio, grad_ok = _apply_ratio(case, which, fault)
            caught_a = caught_a or ratio > 1.0 or not grad_ok
        if caught_a:
            break
    if fault == 'no_relu_neg':       # only nmfmu_trainer_update can be handed a negative numerator
        caught_a = True
    assert caught_u and caught_a, (fault, caught_u, caught_a)


def test_eps_on_the_closed_form_denominator_matters():
    """beta == 1, one layer: with a rank column of the other factor summing to ~1e-6, leaving eps off the closed-form
    denominator moves the update by more than 5 % -- on the case built for it, not only somewhere."""
    case = next(c for c in T.FUSED_CASES if c.get('tiny_col') is not None)
    theta, neg, pos = _fused_inputs(case, 'W')
    assert 5e-7 < float(pos[case['tiny_col']]) < 2e-6
    good, _ = _apply_f32(case, 'W')
    bad, _ = _apply_f32(case, 'W', 'no_final_eps')
    col = case['tiny_col']
    assert float(np.abs(bad[:, col] / good[:, col] - 1).min()) > 0.05
    assert _apply_ratio(case, 'W', 'no_final_eps')[0] > 1e4


def test_terms_fault_is_caught():
    s, v = T.terms_problem(257)
    _, gp = T.terms_f32(s, v, 1.0, fault='gp_raw_kl')
    assert not bool((gp == 1.0).all())


@pytest.mark.parametrize('beta', T.CHAIN_BETAS)
def test_chain_fault_is_caught(beta):
    """The chain's bound adds the worst case of every stage, and sums of up to 130 same-signed terms stay far inside it
    (``test_fp32_chain_within_bound``); it is still two orders of magnitude below one dropped rank step (of 5, 33 and 130)
    in the forward products, for every parameter."""
    V, X0, Ws = T.chain_problem()
    for which in range(4):
        ref = T.chain_step(V, X0, Ws, which, beta, *PEN['all'])
        new, grad = T.chain_step_f32(V, X0, Ws, which, beta, *PEN['all'], fault='last_step_dropped_chunk')
        assert T.worst_ratio(new, ref['new'], ref['bound']) > 1.0 and T.worst_ratio(grad, ref['grad'], ref['grad_bound']) > 1.0


@pytest.mark.parametrize('fault', T.MATMUL_FAULTS)
def test_matmul_fault_is_caught(fault):
    caught = set()
    for M, K in T.RECON_MK:
        for R in T.RECON_R:
            A, B = T.recon_problem(M, K, R)
            if T.worst_ratio(T.matmul_f32(A, B, fault), T.matmul(A, B), T.matmul_bound(A, B)) > 1.0:
                caught.add(R)
            A, B = T.recon_problem(M, K, R, one_hot=True)
            if not np.array_equal(T.matmul_f32(A, B, fault), B[:, T.one_hot_rank(M, K, R)].T):
                caught.add(('one_hot', R))
    if fault == 'last_step_dropped_odd':
        assert {1, 3, 31, 33, 65} <= caught, caught
    elif fault == 'last_step_dropped_chunk':
        assert {1, 2, 3, 4, 31, 33, 36, 65} <= caught, caught
    else:
        assert set(T.RECON_R) <= caught and all(('one_hot', R) in caught for R in T.RECON_R if R > 1), caught
