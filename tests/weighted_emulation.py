"""Float64 reference of weighted NMF on a dense target (csrc/nmfmu_wmu.hip, wmu.WeightedMU), test-only: terms, step and loss
from the DENSE weighted formulas -- weights M >= 0, target V (anything where M == 0), Y = H W^T:

    Gn, Gp = M * output_neg(V, Y), M * output_pos(Y)      (nmf.py:61-74; beta == 1: Gp = M); 0 where M == 0, by selection
    H side: num = Gn W,   den = Gp W          W side: num = Gn^T H,   den = Gp^T H
    step  : f * ((relu(num) + eps) / (relu(den) + eps + l1 + l2 f))^gamma                     (nmf.py:78-92)
    loss  : sum M * (the term of metrics.beta_div(Y, V, beta) at the entry)                   (metrics.py:22, 39, 57, 85-96)

What separates the kernel from this module is fp32 arithmetic alone; every element is held to the bound the standard model
gives for the operations the kernel performs on it (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3-4: a sum of
n terms, every term passing through at most k roundings, is within k u sum |terms| of the exact one to first order;
u = 2^-24).  No bound is taken from a run.  From the kernel source:

* y = <owner[row], panel[col]> is ONE MFMA accumulator fed the full padded rank in ascending order: bitwise a chain of r_pad
  fmaf (v_mfma_f32_32x32x2_f32), one rounding per term, every term >= 0, so y is relative r_pad u; se = y + eps one more:
  S_OPS = r_pad + 1.
* g (``ops_g``), as masked_emulation counts it with that S_OPS -- beta 2: gn = v exact, gp = y (r_pad).  beta 1: gn = v / se
  (S_OPS + the divide), gp = 1 exact.  beta 0: r = 1 / se (S_OPS + 1), gp = r, gn = r r v (twice r's, two multiplies).
  Otherwise p2 = exp2f(c log2f(se)), c = beta - 2: log2f and exp2f are 1-ulp = 2 u functions (ULP_FN); the relative error of
  se moves log2 by S_OPS u / ln 2, log2f adds ULP_FN u |L|, the product c L one rounding; an absolute error d of the exponent
  moves exp2 by d ln 2 relative, exp2f adds ULP_FN u; gn = p2 v: one multiply; gp = p2 se: se's S_OPS and one.  Then the
  weight: one multiply (``m * g``) for either seed.
* a term (m g) panel enters its accumulator by an fmaf (the product is not rounded on its own) and then rides the chain to the
  end of its part: a stage is 32 chained fmaf per accumulator element, a part ``stages-in-part`` of them, so at most
  32 * stages-in-part roundings (fewer in the part that holds the tail: min with the contraction length); the finishing kernel
  adds the parts in part order, ``parts - 1`` more.  k = steps-in-part + parts - 1 + ops_g + 1 (the largest of the row), bound
  k u sum |m g panel|.
* the apply (``APPLY_OPS``) and the way the bounds of num and den reach the result: masked_emulation's.
* the loss: per weighted entry one fp32 expression of y, widened to double, times m in double and summed in double
  (n 2^-53 sum |terms|); the terms of v alone are float64 on the host.
"""
from __future__ import annotations

import numpy as np

import masked_emulation as ME
import mu_emulation as E

EPS = E.EPS
U = ME.U
ULP_FN = ME.ULP_FN
LN2 = ME.LN2
APPLY_OPS = ME.APPLY_OPS
BK = 32                  # kWmBK
TILE_ROWS = 128          # kWmRows
TARGET_WGS, MIN_STAGES, MAX_SPLIT = 512, 4, 64

kind_of, gamma_of, bound_err, apply = ME.kind_of, ME.gamma_of, ME.bound_err, ME.apply


# ---- the split rule of include/nmfmu.h (nmfmu_wmu_nsplit / nmfmu_wmu_ws) -----------------------------------------------------
def stages(contraction: int) -> int:
    return -(-contraction // BK)


def parts_for(contraction: int, nsplit: int) -> int:
    """Parts for a wanted split count >= 1: no empty part, only the last one short."""
    st = stages(contraction)
    n = max(1, min(nsplit, st))
    per = -(-st // n)
    return -(-st // per)


def auto_split(tiles: int, contraction: int) -> int:
    want = -(-TARGET_WGS // tiles)
    cap = max(1, stages(contraction) // MIN_STAGES)
    return parts_for(contraction, min(want, cap, MAX_SPLIT))


def split(rows: int, contraction: int, r_pad: int, nsplit: int = 0) -> int:
    if nsplit > 0:
        return parts_for(contraction, nsplit)
    return auto_split(-(-rows // TILE_ROWS) * -(-r_pad // 128), contraction)


def part_len(contraction: int, parts: int) -> int:
    return -(-stages(contraction) // parts) * BK


def workspace_floats(rows: int, contraction: int, r_pad: int, nsplit: int = 0) -> int:
    return split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad


def loss_parts(n: int, c: int) -> int:
    return -(-n // TILE_ROWS) * auto_split(-(-n // TILE_ROWS), c)


# ---- terms ------------------------------------------------------------------------------------------------------------------
def clean(V, M):
    """(V with 1 where M == 0 -- nothing there may reach a result --, M, the boolean selection)."""
    V, M = np.asarray(V, np.float64), np.asarray(M, np.float64)
    sel = M > 0
    return np.where(sel, V, 1.0), M, sel


def ops_g(se, beta: float, r_pad: int):
    """(roundings behind m * gn, behind m * gp) per entry, in units of u (module docstring)."""
    kind = kind_of(beta)
    s_ops = r_pad + 1
    one = np.ones_like(se)
    if kind == 'euc':
        on, op = 0 * one, r_pad * one
    elif kind == 'kl':
        on, op = (s_ops + 1) * one, 0 * one
    elif kind == 'is':
        r = s_ops + 1
        on, op = (2 * r + 2) * one, r * one
    else:
        c = abs(float(np.float32(beta)) - 2.0)
        expo = c * s_ops / LN2 + c * np.abs(np.log2(se)) * (ULP_FN + 1)
        p2 = expo * LN2 + ULP_FN
        on, op = p2 + 1, p2 + s_ops + 1
    return on + 1, op + 1


def terms(V, M, H, W, beta: float, side: str, nsplit: int = 0):
    """dict(num, den, num_bound, den_bound) of one side, [owner rows, R]."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    V, M, sel = clean(V, M)
    r_pad = E.pad_rank(H.shape[1])
    Y = H @ W.T
    Gn, Gp = ME.g_terms(V, Y, beta)
    Gn, Gp = np.where(sel, M * Gn, 0.0), np.where(sel, M * Gp, 0.0)
    on, op = ops_g(Y + EPS, beta, r_pad)
    on, op = np.where(sel, on, 0.0), np.where(sel, op, 0.0)
    panel = W
    if side == 'w':
        Gn, Gp, on, op, panel = Gn.T, Gp.T, on.T, op.T, H
    rows, contraction = Gn.shape
    parts = split(rows, contraction, r_pad, nsplit)
    k0 = min(part_len(contraction, parts), contraction) + parts - 1
    pa = np.abs(panel)
    return dict(num=Gn @ panel, den=Gp @ panel, parts=parts,
                num_bound=((k0 + on.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gn) @ pa),
                den_bound=((k0 + op.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gp) @ pa))


def step(V, M, H, W, beta: float, side: str, l1=0.0, l2=0.0, nsplit: int = 0):
    """(new owner, bound, terms) of one half-step."""
    t = terms(V, M, H, W, beta, side, nsplit)
    f = np.asarray(H if side == 'h' else W, np.float64)
    gamma = gamma_of(beta)
    new = apply(f, t['num'], t['den'], gamma, l1, l2)
    neg = np.maximum(t['num'], 0.0) + EPS
    pos = np.maximum(t['den'], 0.0) + EPS + (l1 if l1 > 0 else 0.0) + (l2 * f if l2 > 0 else 0.0)
    bound = np.abs(new) * (gamma * (t['num_bound'] / neg + t['den_bound'] / pos) + APPLY_OPS * U)
    return new, bound, t


def iterate(V, M, W, H, beta: float, n_iter: int, l1=0.0, l2=0.0, update_W=True, update_H=True):
    """``n_iter`` iterations of fit's loop (W half-step, then H with the new W), float64."""
    W, H = np.asarray(W, np.float64).copy(), np.asarray(H, np.float64).copy()
    for _ in range(n_iter):
        if update_W:
            W = step(V, M, H, W, beta, 'w', l1, l2)[0]
        if update_H:
            H = step(V, M, H, W, beta, 'h', l1, l2)[0]
    return W, H


# ---- loss -------------------------------------------------------------------------------------------------------------------
def v_term(V, M, beta: float) -> float:
    """sum m * (the terms of metrics.beta_div that hold v alone) over the weighted entries."""
    V, M, sel = clean(V, M)
    v, m = V[sel], M[sel]
    kind = kind_of(beta)
    if kind == 'euc':
        return 0.0
    if kind == 'kl':
        return float(m @ (v * np.log(v + EPS) - v))
    if kind == 'is':
        return float(m @ (-np.log(v + EPS) - 1.0))
    return float(m @ np.power(v + EPS if beta < 0 else v, beta))


def loss(V, M, H, W, beta: float):
    """(the weighted loss, its bound)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    V, M, sel = clean(V, M)
    v, m, s = V[sel], M[sel], (H @ W.T)[sel]
    se = s + EPS
    e_s = E.pad_rank(H.shape[1]) + 1.0                     # roundings of se (of y: one fewer)
    kind = kind_of(beta)
    if kind == 'euc':        # d = y - v (y's error, the subtraction), squared in double
        d = s - v
        t, b, mul = d * d, 2 * np.abs(d) * (e_s * np.abs(s) + np.abs(d)), 0.5
    elif kind == 'kl':       # y widened; v logf(se): se's error through the log, logf's ulp, the multiply
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
    vt_ = v_term(V, M, beta)
    total = (vt_ + m @ t) * mul
    bound = ((m @ b) * U + (len(v) + 8) * 2.0 ** -53 * (m @ np.abs(t) + abs(vt_))) * abs(mul)
    return float(total), float(bound) + 1e-300


def dense_loss(V, M, H, W, beta: float) -> float:
    """sum M * d_beta(V | Y) entry by entry, metrics.py:60-96 restated (the check of ``loss``'s regrouping)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    V, M, sel = clean(V, M)
    y, m, x = V[sel], M[sel], (H @ W.T)[sel]
    if beta == 2:
        return float(0.5 * (m @ (x - y) ** 2))
    if beta == 1:
        return float(m @ (y * (np.log(y + EPS) - np.log(x + EPS)) - y + x))
    if beta == 0:
        return float(m @ ((y + EPS) / (x + EPS) - np.log(y + EPS) + np.log(x + EPS) - 1.0))
    x = x + EPS
    if beta < 0:
        y = y + EPS
    return float(m @ (y ** beta + (beta - 1) * x ** beta - beta * y * x ** (beta - 1)) / (beta * (beta - 1)))


# ---- the problems of tests/test_gpu_weighted.py ----------------------------------------------------------------------------
def make_problem(N: int, C: int, R: int, seed: int = 0):
    """(V, M, W0, H0) fp32: weights real in [0.25, 4) with about 30 % exact zeros, row 5 and column 3 weightless; the target
    uniform in [0.1, 2) where weighted and NaN, Inf, -1 or 1000 where not; factors uniform in [0.1, 1)."""
    g = np.random.default_rng(1000 * seed + 7 * N + 3 * C + R)
    M = (g.random((N, C)) * 3.75 + 0.25).astype(np.float32)
    M[g.random((N, C)) < 0.3] = 0.0
    M[5, :] = 0.0
    M[:, 3] = 0.0
    V = (g.random((N, C)) * 1.9 + 0.1).astype(np.float32)
    junk = np.array([np.nan, np.inf, -1.0, 1000.0], np.float32)[g.integers(0, 4, (N, C))]
    V = np.where(M > 0, V, junk).astype(np.float32)
    W0 = (g.random((C, R)) * 0.9 + 0.1).astype(np.float32)
    H0 = (g.random((N, R)) * 0.9 + 0.1).astype(np.float32)
    return V, M, W0, H0
