"""Float64 reference of the fold-in kernel (csrc/nmfmu_fold_in.hip, torchnmf_amd/fold_in.py), test-only: one iteration and
``k`` iterations of the H half-step on every new row with W fixed, for both readings of the unstored entries, plus the
per-row stop rule.  Dense formulas on a mask M (1 at the stored entries), V (0 elsewhere), S = H W^T:

    missing       : num = (M * g_neg(V, S)) W,  den' = relu((M * g_pos(S)) W) + eps       (masked_emulation.g_terms)
    zero, beta 1  : num = (M * V / (S + eps)) W, den' = colsum(W)            -- no relu, no eps (nmf.py:128-131)
    zero, beta 2  : num = (M * V) W,             den' = relu(H (W^T W)) + eps
    new = h * ((relu(num) + eps) / (den' + l1 + l2 h))^gamma                                (nmf.py:78-92)

What separates the kernel from this module is fp32 arithmetic alone.  Every element of ONE iteration is held to the bound the
standard model gives for the operations the kernel performs on it (masked_emulation's docstring; u = 2^-24); no bound is
taken from a run.  From the kernel source:

* s_j = <h, W[j]>: an r-ordered chain of R fmaf, one rounding each, every term >= 0: relative R u (gamma_R); se = s + eps
  one more.  ``masked_emulation.ops_g`` counts se as RL + 8 roundings for its butterfly; it is called with RL = R - 7, so
  that its count is R + 1, and forms g per branch exactly as for the masked kernel (fold_g is masked_g, line for line).
  zero, beta 1 is the 'kl' branch (the divide); zero, beta 2 has g_neg = v, exact.
* num / den: every term g W[j][r] joins its accumulator by one fmaf (one rounding for the multiply and the add) and passes
  at most count - 1 later ones; a long row (count > long_rows; default ``default_block``, the kernel's largest block of
  the rank) is cut over four waves and its four partials are added in
  wave order, three more.  k = count + waves + ops_g (the row's largest), bound k u sum |g W| -- the masked kernel's rule
  with waves for segments.  The block size does not enter: the chains run on across the blocks.
* zero, beta 1: colsum(W) is nmfmu_rank_sums(W, C, R, 1): up to C <= 2^14 one kernel, 1024 threads with four strided
  partial sums each (ceil(C / 4096) additions), (s0 + s1) + (s2 + s3), a 10-level tree; above, 128 chunks: 256 threads with
  four partial sums each, two, an 8-level tree, then a 7-level tree over the chunks (``colsum_ops``).  All terms >= 0:
  relative.
* zero, beta 2: G = W^T W is nmfmu_gram: 64 chunks of ceil(C / 64) rows, four strided partial sums of products (a multiply
  and ceil(rows / 4) additions, or as many fmaf), two, then 64 additions in chunk order (``gram_ops``); den = sum_q h[q]
  G[q][r], a q-ordered chain of R fmaf.  All terms >= 0: relative (R + gram_ops) u.
* the apply: ``masked_emulation.APPLY_OPS`` roundings of its own; the bounds of num and den reach it as
  d new / new = gamma (d neg / neg + d pos / pos).
* the stop rule is evaluated by the kernel in fp32 exactly as written (one subtraction, one multiply, two maxima);
  ``stop_counts`` restates it in fp32 numpy on a list of states.
"""
from __future__ import annotations

import numpy as np

import masked_emulation as M

EPS = M.EPS
U = M.U
WAVES = 4


def default_block(R: int) -> int:
    """csrc/nmfmu_fold_in.hip: fold_block_cap -- the largest block the workgroup's 64 KiB of LDS hold at rank R, and the
    default long-row threshold."""
    rl = 1 if R <= 64 else (2 if R <= 128 else 4)
    per = (16384 - WAVES * 2 * 64 * rl) // WAVES - 64 * rl - 4
    return max(1, min(64, per // ((R | 1) + 2)))


def colsum_ops(C: int) -> int:
    if C <= (1 << 14):
        return -(-C // 4096) + 2 + 10
    per = -(-C // 128)
    return -(-per // 1024) + 2 + 8 + 7


def gram_ops(C: int) -> int:
    per = -(-C // 64)
    return 1 + -(-per // 4) + 2 + 64


def iteration(idx, vals, shape, H, W, beta: float, mode: str, l1=0.0, l2=0.0, long_rows: int = None):
    """(new H, bound, terms) of one iteration on every row; float64."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    C, R = W.shape
    long_rows = default_block(R) if long_rows is None else long_rows
    V, Mk = M.dense(idx, vals, shape)
    S = H @ W.T
    se = S + EPS
    count = Mk.sum(1)
    k0 = count + np.where(count > long_rows, WAVES, 1)
    pa = np.abs(W)
    gamma = M.gamma_of(beta)
    reg = (l1 if l1 > 0 else 0.0) + (l2 * H if l2 > 0 else 0.0)
    if mode == 'missing':
        Gn, Gp = M.g_terms(V, S, beta)
        on, op = M.ops_g(se, beta, R - 7)
        Gn, Gp, on, op = (np.where(Mk, x, 0.0) for x in (Gn, Gp, on, op))
        den = Gp @ W
        den_bound = ((k0 + op.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gp) @ pa)
        pos = np.maximum(den, 0.0) + EPS + reg
    else:
        kind = M.kind_of(beta)
        assert kind in ('kl', 'euc'), "unstored='zero': beta in {1, 2}"
        if kind == 'kl':
            Gn, on = np.where(Mk, V / se, 0.0), np.where(Mk, R + 2.0, 0.0)
            den = np.broadcast_to(W.sum(0), H.shape)
            den_bound = colsum_ops(C) * U * np.broadcast_to(pa.sum(0), H.shape)
            pos = den + reg
        else:
            Gn, on = np.where(Mk, V, 0.0), np.zeros_like(V)
            G = W.T @ W
            den = H @ G
            den_bound = (R + gram_ops(C)) * U * (np.abs(H) @ np.abs(G))
            pos = np.maximum(den, 0.0) + EPS + reg
    num = Gn @ W
    num_bound = ((k0 + on.max(1, initial=0.0)) * U)[:, None] * (np.abs(Gn) @ pa)
    neg = np.maximum(num, 0.0) + EPS
    new = H * np.power(neg / pos, gamma)
    bound = np.abs(new) * (gamma * (num_bound / neg + den_bound / np.abs(pos)) + M.APPLY_OPS * U)
    return new, bound, dict(num=num, den=den, num_bound=num_bound, den_bound=den_bound, count=count)


def states(idx, vals, shape, H0, W, beta: float, mode: str, k: int, l1=0.0, l2=0.0):
    """[H_0, H_1, .., H_k]: k iterations on every row, none stopped; float64."""
    out = [np.asarray(H0, np.float64)]
    for _ in range(k):
        out.append(iteration(idx, vals, shape, out[-1], W, beta, mode, l1, l2)[0])
    return out


def stop_counts(sts, tol: float):
    """Per row the first k >= 1 with max_r |h_k - h_(k-1)| <= tol * max_r h_k, evaluated in fp32 as the kernel does (one
    subtraction, one multiply, two maxima); len(sts) - 1 where it never holds or tol == 0."""
    sts = [np.asarray(s, np.float32) for s in sts]
    n, last = sts[0].shape[0], len(sts) - 1
    out = np.full(n, last, dtype=np.int32)
    if not tol > 0:
        return out
    open_ = np.ones(n, dtype=bool)
    t = np.float32(tol)
    for k in range(1, last + 1):
        d = np.abs(sts[k] - sts[k - 1]).max(1) if sts[k].shape[1] else np.zeros(n, np.float32)
        m = sts[k].max(1)
        hit = open_ & (d <= t * m)
        out[hit] = k
        open_ &= ~hit
    return out


def run(idx, vals, shape, H0, W, beta: float, mode: str, max_iter: int, tol: float = 0.0, l1=0.0, l2=0.0):
    """(H, counts): every row at the state its own count names (the rows are independent: a stopped row's later states are
    simply not taken)."""
    sts = states(idx, vals, shape, H0, W, beta, mode, max_iter, l1, l2)
    cnt = stop_counts(sts, tol)
    H = np.stack([sts[int(c)][i] for i, c in enumerate(cnt)]) if len(cnt) else sts[0]
    return H, cnt


def check(got, ref, bound, got_counts=None, ref_counts=None):
    """(worst |got - ref| / bound over every element, ok): ok needs every element within its bound and, when counts are
    given, every count equal."""
    e = M.bound_err(got, ref, bound)
    worst = float(e.max()) if e.size else 0.0
    ok = worst <= 1.0
    if ref_counts is not None:
        ok = ok and got_counts is not None and np.array_equal(np.asarray(got_counts, np.int64),
                                                              np.asarray(ref_counts, np.int64))
    return worst, bool(ok)


# ---- the problems of tests/test_gpu_fold_in.py --------------------------------------------------------------------------------
WIDE_COUNTS = (0, 1, 63, 64, 65, 130, 300, 513, 700)    # block edges (63, 64, 65), rows of up to four blocks, longer ones


def make_wide(R: int, C: int = 700, seed: int = 0):
    """(idx, vals, W0, H0) of the 9 x C target whose rows hold WIDE_COUNTS stored entries."""
    g = np.random.default_rng(5000 + 31 * seed + R)
    rows = np.repeat(np.arange(len(WIDE_COUNTS)), WIDE_COUNTS)
    cols = np.concatenate([np.sort(g.choice(C, size=k, replace=False)) for k in WIDE_COUNTS]).astype(np.int64)
    idx = np.stack([rows, cols]).astype(np.int64)
    vals = (g.random(idx.shape[1]) * 1.9 + 0.1).astype(np.float32)
    W0 = (g.random((C, R)) * 0.9 + 0.1).astype(np.float32)
    H0 = (g.random((len(WIDE_COUNTS), R)) * 0.9 + 0.1).astype(np.float32)
    return idx, vals, W0, H0
