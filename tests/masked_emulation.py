"""Float64 reference of missing-data NMF (csrc/nmfmu_sparse_masked.hip, sparse_engine.MaskedMU), test-only: terms, step and
loss from DENSE masked formulas -- a mask M (1 at the stored entries), the target V (0 elsewhere), S = H W^T:

    Gn, Gp = M * output_neg(V, S), M * output_pos(S)      (nmf.py:61-74; beta == 1: Gp = M)
    H side: num = Gn W,   den = Gp W          W side: num = Gn^T H,   den = Gp^T H
    step  : f * ((relu(num) + eps) / (relu(den) + eps + l1 + l2 f))^gamma                     (nmf.py:78-92)
    loss  : metrics.beta_div(S[M], V[M], beta)                                                (metrics.py:22, 39, 57, 85-96)

Nothing on this path is rounded to 16 bits: what separates the kernel from this module is fp32 arithmetic alone, and every
element is held to the bound the standard model gives for the operations the kernel performs on it (Higham, Accuracy and
Stability of Numerical Algorithms, ch. 3-4: a sum of n terms, every term passing through at most k roundings, is within
k u sum |terms| of the exact one to first order; u = 2^-24).  No bound is taken from a run.  From the kernel source:

* s = <owner[row], panel[col]>: one multiply per product, at most RL additions into the lane's partial, six butterfly
  additions: RL + 7 roundings, every term >= 0, so s is relative (RL + 7) u; se = s + eps one more: S_OPS = RL + 8.
* g (``ops_g``): beta 2: gn = v exact, gp = s (RL + 7).  beta 1: gn = v / se (S_OPS + the divide), gp = 1 exact.  beta 0:
  r = 1 / se (S_OPS + 1), gp = r, gn = r r v (twice r's, two multiplies).  Otherwise p2 = exp2f(c log2f(se)), c = beta - 2:
  log2f and exp2f are 1-ulp = 2 u functions (ULP_FN, the explicit allowance for the pair); the relative error S_OPS u of se
  moves log2 by S_OPS u / ln 2, log2f adds ULP_FN u |L|, the product c L one rounding u |c L|; an absolute error d of the
  exponent moves exp2 by d ln 2 relative, exp2f adds ULP_FN u.  gn = p2 v: one multiply; gp = p2 se: se's S_OPS and one.
* every term g b is one multiply and joins its accumulator through at most ``count`` additions inside the segments (storage
  order) and ``segments - 1`` in the finishing kernel: k = count + segments + ops_g (the row's largest), bound
  k u sum |g panel|.
* the apply (``APPLY_OPS``): relu + eps twice, + l1, l2 f (two), the divide, powf (ULP_FN), the multiply by f -- relative
  to the result; the bounds of num and den reach it as d new / new = gamma (d neg / neg + d pos / pos)
  (``sparse_emulation.apply_allowance``'s rule, with the masked denominator for every beta).
* the loss: per stored entry one fp32 expression of s, widened to double and summed in double (n 2^-53 sum |terms|); the
  terms of v alone are float64 on the host.  ``loss`` lists the roundings of each branch beside the formula.
"""
from __future__ import annotations

import math

import numpy as np

import mu_emulation as E

EPS = E.EPS
U = 2.0 ** -24
ULP_FN = 2.0
LN2 = math.log(2.0)
APPLY_OPS = 9


def rank_slots(r_pad: int) -> int:
    return 1 if r_pad <= 64 else (2 if r_pad == 128 else 4)


def kind_of(beta: float) -> str:
    """nmfmu_beta_kind: the four branches of the masked kernels."""
    beta = float(np.float32(beta))
    return {1.0: 'kl', 2.0: 'euc', 0.0: 'is'}.get(beta, 'gen')


def gamma_of(beta: float) -> float:
    return 1.0 / (2.0 - beta) if beta < 1 else (1.0 / (beta - 1.0) if beta > 2 else 1.0)


def dense(idx, vals, shape):
    """(V, M) float64 / bool from coalesced COO entries."""
    V = np.zeros(shape)
    M = np.zeros(shape, dtype=bool)
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    V[idx[0], idx[1]] = np.asarray(vals, dtype=np.float64)
    M[idx[0], idx[1]] = True
    return V, M


def g_terms(V, S, beta: float):
    """(Gn, Gp) unmasked, float64."""
    kind = kind_of(beta)
    se = S + EPS
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if kind == 'euc':
            return V, S
        if kind == 'kl':
            return V / se, np.ones_like(S)
        if kind == 'is':
            return V / (se * se), 1.0 / se
        b = float(np.float32(beta))
        return V * np.power(se, b - 2.0), np.power(se, b - 1.0)


def ops_g(se, beta: float, RL: int):
    """(roundings behind gn, behind gp) per entry, in units of u (module docstring)."""
    kind = kind_of(beta)
    s_ops = RL + 8
    one = np.ones_like(se)
    if kind == 'euc':
        return 0 * one, (RL + 7) * one
    if kind == 'kl':
        return (s_ops + 1) * one, 0 * one
    if kind == 'is':
        r = s_ops + 1
        return (2 * r + 2) * one, r * one
    c = abs(float(np.float32(beta)) - 2.0)
    expo = c * s_ops / LN2 + c * np.abs(np.log2(se)) * (ULP_FN + 1)
    p2 = expo * LN2 + ULP_FN
    return p2 + 1, p2 + s_ops + 1


def segments(count, chunk: int):
    return np.maximum(-(-np.asarray(count) // int(chunk)), 1)


def terms(idx, vals, shape, H, W, beta: float, side: str, chunk: int = 512):
    """dict(num, den, num_bound, den_bound) of one side, [owner rows, R]."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    V, M = dense(idx, vals, shape)
    S = H @ W.T
    Gn, Gp = g_terms(V, S, beta)
    Gn, Gp = np.where(M, Gn, 0.0), np.where(M, Gp, 0.0)
    on, op = ops_g(S + EPS, beta, rank_slots(E.pad_rank(H.shape[1])))
    on, op = np.where(M, on, 0.0), np.where(M, op, 0.0)
    panel = W
    if side == 'w':
        Gn, Gp, on, op, M, panel = Gn.T, Gp.T, on.T, op.T, M.T, H
    count = M.sum(1)
    k0 = count + segments(count, chunk)
    pa = np.abs(panel)
    return dict(num=Gn @ panel, den=Gp @ panel, count=count,
                num_bound=((k0 + on.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gn) @ pa),
                den_bound=((k0 + op.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gp) @ pa))


def apply(f, num, den, gamma: float, l1=0.0, l2=0.0):
    f = np.asarray(f, np.float64)
    neg = np.maximum(num, 0.0) + EPS
    pos = np.maximum(den, 0.0) + EPS + (l1 if l1 > 0 else 0.0) + (l2 * f if l2 > 0 else 0.0)
    return f * np.power(neg / pos, gamma)


def step(idx, vals, shape, H, W, beta: float, side: str, l1=0.0, l2=0.0, chunk: int = 512):
    """(new owner, bound) of one half-step."""
    t = terms(idx, vals, shape, H, W, beta, side, chunk)
    f = np.asarray(H if side == 'h' else W, np.float64)
    gamma = gamma_of(beta)
    new = apply(f, t['num'], t['den'], gamma, l1, l2)
    neg = np.maximum(t['num'], 0.0) + EPS
    pos = np.maximum(t['den'], 0.0) + EPS + (l1 if l1 > 0 else 0.0) + (l2 * f if l2 > 0 else 0.0)
    bound = np.abs(new) * (gamma * (t['num_bound'] / neg + t['den_bound'] / pos) + APPLY_OPS * U)
    return new, bound, t


def v_term(vals, beta: float) -> float:
    v = np.asarray(vals, np.float64)
    kind = kind_of(beta)
    if kind == 'euc':
        return 0.0
    if kind == 'kl':
        return float(v @ np.log(v + EPS) - v.sum())
    if kind == 'is':
        return float(-np.log(v + EPS).sum() - len(v))
    return float(np.power(v + EPS if beta < 0 else v, beta).sum())


def loss(idx, vals, H, W, beta: float):
    """(metrics.beta_div over the stored entries, its bound)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    v = np.asarray(vals, np.float64)
    s = np.einsum('pr,pr->p', H[idx[0]], W[idx[1]]) if len(v) else np.zeros(0)
    se = s + EPS
    e_s = rank_slots(E.pad_rank(H.shape[1])) + 8.0          # roundings of se (of s: one fewer)
    kind = kind_of(beta)
    if kind == 'euc':        # d = s - v (s's error, the subtraction), squared in double
        d = s - v
        t, b, mul = d * d, 2 * np.abs(d) * (e_s * np.abs(s) + np.abs(d)), 0.5
    elif kind == 'kl':       # s widened; v logf(se): se's error through the log, logf's ulp, the multiply
        lg = np.log(se)
        t, b, mul = s - v * lg, e_s * s + v * (e_s + (ULP_FN + 1) * np.abs(lg)), 1.0
    elif kind == 'is':       # (v + eps) / se: the addition, se, the divide; logf(se)
        q, lg = (v + EPS) / se, np.log(se)
        t, b, mul = q + lg, q * (e_s + 2) + e_s + ULP_FN * np.abs(lg), 1.0
    else:                    # pb1 = exp2f(c log2f(se)), c = beta - 1, times (c se - beta v') in double
        bt = float(np.float32(beta))
        c = bt - 1.0
        vt = v + EPS if bt < 0 else v
        pb1 = np.power(se, c)
        ep = (abs(c) * e_s / LN2 + abs(c) * np.abs(np.log2(se)) * (ULP_FN + 1)) * LN2 + ULP_FN
        t = pb1 * (c * se - bt * vt)
        b = pb1 * (ep * (abs(c) * se + abs(bt) * vt) + abs(c) * se * e_s + abs(bt) * vt)
        mul = 1.0 / (bt * c)
    vt_ = v_term(v, beta)
    total = (vt_ + t.sum()) * mul
    bound = (b.sum() * U + (len(v) + 8) * 2.0 ** -53 * (np.abs(t).sum() + abs(vt_))) * abs(mul)
    return float(total), float(bound) + 1e-300


def dense_loss(idx, vals, H, W, beta: float) -> float:
    """metrics.py:60-96 restated on the gathered vectors (the check of ``loss``'s regrouping)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    y = np.asarray(vals, np.float64)
    x = np.einsum('pr,pr->p', H[idx[0]], W[idx[1]])
    if beta == 2:
        return float(0.5 * ((x - y) ** 2).sum())
    if beta == 1:
        return float(y @ (np.log(y + EPS) - np.log(x + EPS)) - y.sum() + x.sum())
    if beta == 0:
        return float(((y + EPS) / (x + EPS)).sum() - np.log(y + EPS).sum() + np.log(x + EPS).sum() - len(y))
    x = x + EPS
    if beta < 0:
        y = y + EPS
    return float(((y ** beta).sum() + (beta - 1) * (x ** beta).sum() - beta * (y @ x ** (beta - 1))) / (beta * (beta - 1)))


def bound_err(got, ref, bound):
    """Per element |got - ref| / bound; where the bound is 0 (nothing is rounded) any difference is inf; inf where ``got`` is
    not finite."""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), e, np.inf)


# ---- the problems of tests/test_gpu_masked.py -----------------------------------------------------------------------------
COUNTS = (0, 1, 4, 5, 8, 9, 20)     # unroll tails (1, 5, 9), whole trips (4, 8, 20), chunk 8: exact (8) and split (9, 20)


def make_problem(N: int, C: int, R: int, axis: int = 0, seed: int = 0):
    """(idx [2, nnz] sorted by (row, col), vals fp32, W0, H0): owner ``axis`` (0: rows of V, 1: columns) cycles through
    COUNTS; index 3 of the other axis holds no entry.  Factors uniform in [0.1, 1), values uniform in [0.1, 2)."""
    g = np.random.default_rng(1000 * seed + 7 * N + 3 * C + R + axis)
    n, c = (C, N) if axis else (N, C)
    allowed = np.delete(np.arange(c), 3)
    counts = [COUNTS[i % len(COUNTS)] for i in range(n)]
    own = np.repeat(np.arange(n), counts)
    oth = np.concatenate([np.sort(g.choice(allowed, size=k, replace=False)) for k in counts])
    rows, cols = (oth, own) if axis else (own, oth)
    order = np.lexsort((cols, rows))
    idx = np.stack([rows[order], cols[order]]).astype(np.int64)
    vals = (g.random(idx.shape[1]) * 1.9 + 0.1).astype(np.float32)
    W0 = (g.random((C, R)) * 0.9 + 0.1).astype(np.float32)
    H0 = (g.random((N, R)) * 0.9 + 0.1).astype(np.float32)
    return idx, vals, W0, H0
