"""Float64 numpy model of ARD-NMF as ``torchnmf_amd.ard`` / ``csrc/nmfmu_ard.hip`` compute it (Tan & Fevotte 2013; conventions
of this code base: ``V ~ H W^T``, ``H [N, R]``, ``W [C, R]``): one half-step, the relevance update, the objective, and the loop
W half-step, H half-step, relevance.  TEST-ONLY; shared by tests/test_ard_emulation.py (no GPU) and tests/test_gpu_ard.py.

    Obj = D_beta(V | H W^T) / phi + sum_k [ (f(W[:, k]) + f(H[:, k]) + b) / lambda_k + c log lambda_k ]
    'l1': f = ||.||_1, c = N + C + a + 1, pos += pen[k];   'l2': f = 1/2 ||.||^2, c = (N + C) / 2 + a + 1, pos += pen[k] * f
    pen[k] = phi / lambda_k;  lambda_k = (f(W[:, k]) + f(H[:, k]) + b) / c

The eps conventions are the engine's (nmf.py:61-92 of the reference): eps inside the elementwise terms for beta != 2, relu + eps on
numerator and denominator, the closed-form denominator (column sums of the panel, no eps) at beta == 1.
"""
import math

import numpy as np

EPS = 1.1920928955078125e-07     # kEps (nmfmu_fused.h)
U32 = 2.0 ** -24                 # unit roundoff of fp32


def exponent(beta: float, prior: str) -> float:
    if prior == 'l1':
        return 1.0 / (2.0 - beta) if beta < 1 else (1.0 / (beta - 1.0) if beta > 2 else 1.0)
    return 1.0 / (3.0 - beta) if beta <= 2 else 1.0 / (beta - 1.0)


def c_of(N: int, C: int, a: float, prior: str) -> float:
    return N + C + a + 1.0 if prior == 'l1' else (N + C) / 2.0 + a + 1.0


def default_b(v_mean: float, R: int, a: float, prior: str) -> float:
    if prior == 'l1':
        return math.sqrt((a - 1.0) * (a - 2.0) * v_mean / R)
    return math.pi * (a - 1.0) * v_mean / (2.0 * R)


def norm(F, prior: str) -> np.ndarray:
    F = np.asarray(F, dtype=np.float64)
    return F.sum(0) if prior == 'l1' else 0.5 * (F * F).sum(0)


def mu_terms(X, S, beta: float):
    """(Gn, Gp) of nmf.py:61-74; Gp is None at beta == 1 (closed-form denominator)."""
    if beta == 2:
        return X, S
    if beta == 1:
        return X / (S + EPS), None
    Se = S + EPS
    return Se ** (beta - 2) * X, Se ** (beta - 1)


def beta_div(S, X, beta: float) -> float:
    if beta == 2:
        return float(0.5 * ((S - X) ** 2).sum())
    if beta == 1:
        return float((X * (np.log(X + EPS) - np.log(S + EPS))).sum() - X.sum() + S.sum())
    if beta == 0:
        q = (X + EPS) / (S + EPS)
        return float((q - np.log(q)).sum() - X.size)
    Se, Xf = S + EPS, (X + EPS if beta < 0 else X)
    return float(((Xf ** beta).sum() + (beta - 1) * (Se ** beta).sum() - beta * (Xf * Se ** (beta - 1)).sum()) / (beta * (beta - 1)))


def apply_stage(theta, num, den, kl_den, pen, prior: str, e: float) -> np.ndarray:
    """ard_apply_kernel on summed slabs: ``num`` / ``den`` [rows, R] (den None at beta == 1, then ``kl_den`` [R]), ``pen`` [R]."""
    theta = np.asarray(theta, dtype=np.float64)
    neg = np.maximum(num, 0.0) + EPS
    pos = np.broadcast_to(np.asarray(kl_den, dtype=np.float64), theta.shape) if den is None else np.maximum(den, 0.0) + EPS
    pen = np.asarray(pen, dtype=np.float64)
    pos = pos + (pen if prior == 'l1' else pen * theta)
    mult = neg / pos
    return theta * (mult if e == 1 else mult ** e)


def half_step(F, P, X, beta: float, prior: str, pen, e: float) -> np.ndarray:
    """Owner ``F [M, R]`` against the panel ``P [K, R]`` and the target ``X [M, K]`` (the W half-step passes V^T)."""
    gn, gp = mu_terms(X, F @ P.T, beta)
    return apply_stage(F, gn @ P, None if gp is None else gp @ P, P.sum(0), pen, prior, e)


def relevance(W, H, prior: str, b: float, c: float) -> np.ndarray:
    return (norm(W, prior) + norm(H, prior) + b) / c


def objective(H, W, V, lam, beta: float, prior: str, phi: float, a: float, b: float) -> float:
    c = c_of(H.shape[0], W.shape[0], a, prior)
    return beta_div(H @ W.T, V, beta) / phi + float(((norm(W, prior) + norm(H, prior) + b) / lam + c * np.log(lam)).sum())


def iterate(V, W, H, beta, prior, phi, a, b, n_iter, update_W=True, update_H=True, trace=None):
    """``n_iter`` iterations from (W, H) in float64; lambda starts from the initial factors.  Returns (W, H, lam).
    ``trace``: a list that receives the objective after every sub-step (W, H, relevance), after the initial value."""
    V, W, H = (np.array(t, dtype=np.float64) for t in (V, W, H))
    e, c = exponent(beta, prior), c_of(H.shape[0], W.shape[0], a, prior)
    lam = relevance(W, H, prior, b, c)
    obj = lambda: objective(H, W, V, lam, beta, prior, phi, a, b)
    if trace is not None:
        trace.append(obj())
    for _ in range(n_iter):
        pen = phi / lam
        if update_W:
            W = half_step(W, H, V.T, beta, prior, pen, e)
            if trace is not None:
                trace.append(obj())
        if update_H:
            H = half_step(H, W, V, beta, prior, pen, e)
            if trace is not None:
                trace.append(obj())
        lam = relevance(W, H, prior, b, c)
        if trace is not None:
            trace.append(obj())
    return W, H, lam


def relative_relevance(lam, b: float, c: float) -> np.ndarray:
    B = b / c
    return (np.asarray(lam, dtype=np.float64) - B) / B


# ---- the planted case: a 40 x 60 target of rank 3 with 2 % multiplicative noise, fitted at rank 8 ------------------------
PLANTED = dict(N=40, C=60, true_rank=3, R=8, beta=1.0, phi=0.1, a=5.0, n_iter=500, seed=2, noise=0.02)


def planted(seed=None):
    """(V, W0, H0) in float64: V = (Ht Wt^T) (1 + noise * normal), Ht / Wt uniform on [0, 1); the start is |normal|."""
    p = PLANTED
    rng = np.random.default_rng(p['seed'] if seed is None else seed)
    Ht, Wt = rng.random((p['N'], p['true_rank'])), rng.random((p['C'], p['true_rank']))
    V = (Ht @ Wt.T) * (1.0 + p['noise'] * rng.standard_normal((p['N'], p['C'])))
    V = np.maximum(V, 1e-3)
    W0, H0 = np.abs(rng.standard_normal((p['C'], p['R']))), np.abs(rng.standard_normal((p['N'], p['R'])))
    return V, W0, H0
