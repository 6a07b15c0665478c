"""Float64 formulas and first-order error bounds of the ``trainer.BetaMu`` paths (test-only, numpy, no GPU).

Everything here is read off the kernel sources (pytorch-nmf_amd/csrc) the way tests/mu_emulation.py and
tests/sparse_autograd_reference.py do; no constant is fitted to device output.  u = 2^-24 (``U``); one unit in the last
place of an fp32 value is at most 2 u of that value (``ULP``).

* ``update`` / ``update_bound``: trainer.py:93-112 as ``trainer_update_kernel`` (nmfmu_aux.hip:656-684) and the trainer mode of
  ``apply_kernel`` (nmfmu_aux.hip:144-162, :219-236) do it.  Both kernels run the same chain on the element:
  relu of neg and pos (:674-675 / :215, :221), ``grad = ps - ng`` (:676 / :224), ``+ l1`` (:677 / :225), ``+ l2 * theta``
  (:678 / :226), ``+ ortho * (rowsum - theta)`` (:679 / :228), ``+ eps`` on both terms (:680 / :222, :229), IEEE division
  (:680 / :231), ``powf`` when gamma != 1 (:681 / :232), the product with theta (:682 / :233).  They differ in the row sum
  only: per-thread strided partial sums and an eight-level tree (:663-670, ``rowsum_ops_update``), or a serial loop over
  the rank (:157, ``rowsum_ops_apply``).  The bound counts one rounding (u of the result) per add and per multiply; a
  multiply-add the compiler contracts rounds once, so counting two covers either code.  ``powf``: ROCm's HIP math API
  table with the ULP figures is not among the documents available to this suite, so ``POW_ULPS`` is 4, the CUDA
  programming guide's figure for the same API.
* ``grad_f32``: ``grad`` is ONE correctly rounded fp32 subtraction of two fp32 values -- checked bit for bit.
* ``terms`` / ``terms_bound``: ``mu_terms_kernel`` (nmfmu_aux.hip:591-600) = ``mu_elem`` (nmfmu_fused.h:276-299) on ``s + eps``
  (``s`` itself at beta == 2), launched with ``nmfmu_beta_kind`` (nmfmu_capi.hip:212-217): beta 1, 2 and 0 have their own
  branches, every other beta takes the generic ``v_log_f32`` / ``v_exp_f32`` one.  ``v_rcp_f32``, ``v_log_f32`` and ``v_exp_f32``
  are good to one ulp; the logarithm's error is amplified by ``|(beta - 1) log2 s|`` (the comment above
  ``beta_div_grad_kernel``, ``AMBIGUITY`` in mu_emulation.py).  Near s = 1 the logarithm is close to zero and one ulp of it
  is finer than one ulp of its argument resolves, so the bound also carries one argument-ulp's worth, 2 u / ln 2.
* ``matmul_bound``: ``reconstruct_kernel`` (nmfmu_aux.hip:727-796), fp32 MFMA accumulation in rank order:
  (R + 2) u (|A| |B|^T) per element, the figure of sparse_autograd_reference.py -- it holds for any summation order.
* ``chain_step``: ``BetaMu._chain_step`` (trainer.py of the package, :281-310): forward products, seeds, back-propagated
  products, update; every quantity is non-negative, so the stages' errors add (carried as absolute per-element errors).

The ``*_f32`` functions are plain ``np.float32`` emulations in the kernels' operation order; ``fault=`` seeds one of the
mistakes tests/test_trainer_emulation.py must see caught.  The case generators at the end give the CPU and the GPU tests
the same arrays.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
ULP = 2.0 * U
EPS = 1.1920928955078125e-07      # kEps (nmfmu_fused.h:75)
LN2 = float(np.log(2.0))
POW_ULPS = 4                      # powf: the CUDA guide's figure (see the module docstring)
F32 = np.float32


def f32(x) -> float:
    """The value a C ``float`` argument receives."""
    return float(np.float32(x))


def mu_gamma(beta: float) -> float:
    """engine.mu_gamma (nmf.py:341-346) as ``nmfmu_trainer_update`` receives it: rounded to fp32."""
    beta = float(beta)
    g = 1.0 / (2.0 - beta) if beta < 1 else (1.0 / (beta - 1.0) if beta > 2 else 1.0)
    return f32(g)


def beta_kind(beta: float) -> str:
    """nmfmu_beta_kind (nmfmu_capi.hip:212-217)."""
    return {1.0: 'kl', 2.0: 'euc', 0.0: 'is'}.get(f32(beta), 'gen')


# ---- the update ------------------------------------------------------------------------------------------------------
def rowsum_ops_update(cols: int) -> int:
    """Roundings behind one row sum of trainer_update_kernel: a thread adds ceil(cols / 256) elements to 0.f (the first
    addition is exact), then eight levels of the shared-memory tree."""
    return max(-(-cols // 256) - 1, 0) + 8


def rowsum_ops_apply(rank: int) -> int:
    """apply_kernel: one thread adds the ``rank`` staged values to 0.f in order."""
    return max(rank - 1, 0)


def _rows(theta, rowsum):
    return theta.sum(1, keepdims=True) if rowsum is None else np.asarray(rowsum, dtype=np.float64)


def update(theta, neg_raw, pos_raw, gamma, l1=0.0, l2=0.0, ortho=0.0, rowsum=None):
    """(new, grad) in float64.  ``gamma``, ``l1``, ``l2``, ``ortho``: the values the kernel holds (``f32`` of what the caller
    passed to the C entry).  ``rowsum``: sum over axis 1 of theta (default), broadcastable to theta."""
    theta = np.asarray(theta, dtype=np.float64)
    ng = np.maximum(np.asarray(neg_raw, dtype=np.float64), 0.0)
    ps = np.maximum(np.broadcast_to(np.asarray(pos_raw, dtype=np.float64), theta.shape), 0.0)
    grad = ps - ng
    p = ps
    if l1 > 0:
        p = p + l1
    if l2 > 0:
        p = p + l2 * theta
    if ortho > 0:
        p = p + ortho * (_rows(theta, rowsum) - theta)
    mult = (ng + EPS) / (p + EPS)
    if gamma != 1:
        mult = np.power(mult, gamma)
    return theta * mult, grad


def update_bound(theta, neg_raw, pos_raw, gamma, l1=0.0, l2=0.0, ortho=0.0, c_rs=0, rowsum=None, rowabs=None,
                 neg_err=0.0, pos_err=0.0):
    """First-order bound of |new_fp32 - new_float64| per element.  ``c_rs``: roundings of the fp32 row sum
    (``rowsum_ops_*``); ``rowabs``: sum |theta| over the same axis; ``neg_err`` / ``pos_err``: absolute errors the raw inputs
    already carry (0 when they are the kernel's own inputs)."""
    theta = np.asarray(theta, dtype=np.float64)
    ng = np.maximum(np.asarray(neg_raw, dtype=np.float64), 0.0)
    p = np.maximum(np.broadcast_to(np.asarray(pos_raw, dtype=np.float64), theta.shape), 0.0)
    dp = np.zeros_like(theta) + pos_err                 # absolute error of the running denominator
    if l1 > 0:
        p = p + l1
        dp = dp + U * np.abs(p)                         # one add
    if l2 > 0:
        t = l2 * theta
        p = p + t
        dp = dp + U * np.abs(t) + U * np.abs(p)         # multiply, add
    if ortho > 0:
        rs = _rows(theta, rowsum)
        ra = np.abs(theta).sum(1, keepdims=True) if rowabs is None else np.asarray(rowabs, dtype=np.float64)
        d = rs - theta
        dd = c_rs * U * ra + U * np.abs(d)              # the fp32 row sum, the subtraction
        t = ortho * d
        p = p + t
        dp = dp + ortho * dd + U * np.abs(t) + U * np.abs(p)   # multiply, add
    p = p + EPS
    dp = dp + U * np.abs(p)                             # + eps
    n = ng + EPS
    dn = neg_err + U * n                                # + eps
    rel = dn / n + dp / np.abs(p) + U                   # IEEE division
    new = theta * np.power(n / p, gamma) if gamma != 1 else theta * (n / p)
    if gamma != 1:
        rel = gamma * rel + POW_ULPS * ULP
    return np.abs(new) * (rel + U)                      # the product with theta


def grad_f32(neg_raw, pos_raw):
    """``relu(pos) - relu(neg)`` as one fp32 subtraction (bit-exact reference of ``grad``)."""
    ng = np.maximum(np.asarray(neg_raw, dtype=F32), F32(0))
    ps = np.maximum(np.asarray(pos_raw, dtype=F32), F32(0))
    return (ps - ng).astype(F32)


def rowsum_update_f32(theta):
    """trainer_update_kernel's row sum in its own order (2-D fp32 array -> [rows, 1])."""
    theta = np.asarray(theta, dtype=F32)
    rows, cols = theta.shape
    red = np.zeros((rows, 256), dtype=F32)
    for c0 in range(0, cols, 256):
        w = min(256, cols - c0)
        red[:, :w] = red[:, :w] + theta[:, c0:c0 + w]
    o = 128
    while o > 0:
        red[:, :o] = red[:, :o] + red[:, o:2 * o]
        o >>= 1
    return red[:, :1].copy()


def rowsum_apply_f32(theta):
    """apply_kernel's: serial over the rank."""
    theta = np.asarray(theta, dtype=F32)
    s = np.zeros((theta.shape[0], 1), dtype=F32)
    for r in range(theta.shape[1]):
        s = s + theta[:, r:r + 1]
    return s


UPDATE_FAULTS = ('no_final_eps', 'eps_twice', 'rowsum_updated', 'rowsum_padded', 'no_minus_theta', 'grad_after_l1',
                 'no_relu_neg', 'gamma_ignored', 'tail_skipped')


def update_f32(theta, neg_raw, pos_raw, gamma, l1=0.0, l2=0.0, ortho=0.0, rowsum_fn=rowsum_update_f32, fault=None, pad=256,
               rs_pad=None):
    """(new, grad) of the kernels in np.float32, operation by operation.  ``pad``: the group 'tail_skipped' leaves a
    remainder of (256, trainer_update_kernel's column stride; 4, apply_kernel's rank group); ``rs_pad``: the multiple
    'rowsum_padded' reads up to (default ``pad``; the padded rank for apply_kernel)."""
    th = np.asarray(theta, dtype=F32)
    neg = np.asarray(neg_raw, dtype=F32)
    pos = np.broadcast_to(np.asarray(pos_raw, dtype=F32), th.shape)
    eps, gam = F32(EPS), F32(gamma)
    l1f, l2f, orf = F32(l1), F32(l2), F32(ortho)
    with np.errstate(invalid='ignore', divide='ignore'):
        ng = neg if fault == 'no_relu_neg' else np.maximum(neg, F32(0))
        ps = np.maximum(pos, F32(0))
        if fault == 'eps_twice':
            ps = ps + eps
        grad = ps - ng
        if l1 > 0:
            ps = ps + l1f
            if fault == 'grad_after_l1':
                grad = ps - ng
        if l2 > 0:
            ps = ps + l2f * th
        if ortho > 0:
            src = th
            if fault == 'rowsum_updated':
                src = update_f32(theta, neg_raw, pos_raw, gamma, l1, l2, ortho, rowsum_fn)[0]
            if fault == 'rowsum_padded':      # the neighbours up to the next multiple of ``pad``, holding 1.0
                fill = np.ones(th.shape[:1] + (-th.shape[1] % (rs_pad or pad),) + th.shape[2:], dtype=F32)
                src = np.concatenate([th, fill], axis=1)
            rs = rowsum_fn(src)
            ps = ps + orf * (rs if fault == 'no_minus_theta' else rs - th)
        if fault != 'no_final_eps':
            ps = ps + eps
        mult = (ng + eps) / ps
        if gamma != 1 and fault != 'gamma_ignored':
            mult = np.power(mult, gam)
        new = (th * mult).astype(F32)
    if fault == 'tail_skipped':
        tail = th.shape[1] % pad
        if tail:
            new[:, -tail:] = th[:, -tail:]
    return new, grad.astype(F32)


# ---- the seeds ---------------------------------------------------------------------------------------------------------
def terms(s, v, beta):
    """(gn, gp) of mu_terms_kernel in float64; ``s`` WITHOUT eps (the kernel adds it)."""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    kind = beta_kind(beta)
    if kind == 'euc':
        return v.copy(), s.copy()
    se = s + EPS
    if kind == 'kl':
        return v / se, np.ones_like(se)
    if kind == 'is':
        return v / (se * se), 1.0 / se
    gp = np.power(se, f32(beta) - 1.0)
    return gp / se * v, gp


def terms_bound(s, v, beta, s_err=0.0):
    """(bound of gn, bound of gp), absolute.  ``s_err``: the absolute error ``s`` already carries."""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    gn, gp = terms(s, v, beta)
    kind = beta_kind(beta)
    b = f32(beta)
    if kind == 'euc':
        return np.zeros_like(gn), np.zeros_like(gp) + s_err        # gn = v, gp = s: copies
    se = s + EPS
    rs = s_err / se + U                                             # relative error of s + eps (one add)
    if kind == 'kl':
        return np.abs(gn) * (rs + ULP + U), np.zeros_like(gp)       # v_rcp_f32, one multiply; gp = 1.0f
    if kind == 'is':
        rp = rs + ULP                                               # v_rcp_f32
        return np.abs(gn) * (2 * rp + 2 * U), np.abs(gp) * rp       # gp * gp * v
    a = abs(b - 1.0)
    lg = np.abs(np.log2(se))
    dlg = ULP * lg + ULP / LN2 + rs / LN2                           # v_log_f32 (see the module docstring), s's own error
    dt = a * dlg + U * a * lg                                       # (beta - 1) * lg
    rp = LN2 * dt + ULP                                             # v_exp_f32
    rn = rp + (rs + ULP) + 2 * U                                    # gp * v_rcp_f32(s) * v
    return np.abs(gn) * rn, np.abs(gp) * rp


def terms_f32(s, v, beta, fault=None):
    s, v = np.asarray(s, dtype=F32), np.asarray(v, dtype=F32)
    kind = beta_kind(beta)
    if kind == 'euc':
        return v.copy(), s.copy()
    with np.errstate(over='ignore', divide='ignore'):
        se = s + F32(EPS)
        rcp = F32(1) / se
        if kind == 'kl':
            gp = np.zeros_like(se) if fault == 'gp_raw_kl' else np.ones_like(se)   # mu_elem<kKL> leaves gp = 0.f
            return v * rcp, gp
        if kind == 'is':
            return rcp * rcp * v, rcp
        gp = np.exp2((F32(beta) - F32(1)) * np.log2(se)).astype(F32)
        return (gp * rcp * v).astype(F32), gp


# ---- the products ------------------------------------------------------------------------------------------------------
def matmul(A, B):
    """A @ B^T in float64 (nmfmu_reconstruct's operand convention)."""
    return np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T


def matmul_bound(A, B, err_a=None, err_b=None):
    A, B = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(B, dtype=np.float64))
    out = (A.shape[1] + 2) * U * (A @ B.T)
    if err_a is not None:
        out = out + np.asarray(err_a) @ B.T
    if err_b is not None:
        out = out + A @ np.asarray(err_b).T
    return out


MATMUL_FAULTS = ('rows_swapped', 'last_step_dropped_odd', 'last_step_dropped_chunk')


def matmul_f32(A, B, fault=None):
    """fp32 accumulation in rank order.  Faults: two output rows of a 32-row block exchanged; the last rank step left
    out where R is odd (the MFMA takes two steps at a time) / where R is no multiple of the 32-column staging chunk."""
    A, B = np.asarray(A, dtype=F32), np.asarray(B, dtype=F32)
    R = A.shape[1]
    stop = R
    if (fault == 'last_step_dropped_odd' and R % 2 == 1) or (fault == 'last_step_dropped_chunk' and R % 32 != 0):
        stop = R - 1
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=F32)
    for r in range(stop):
        acc = acc + A[:, r:r + 1] * B[:, r][None, :]
    if fault == 'rows_swapped' and A.shape[0] >= 6:
        m0 = 32 * ((A.shape[0] - 6) // 32)
        acc[[m0 + 1, m0 + 5]] = acc[[m0 + 5, m0 + 1]]
    return acc


# ---- the chain ---------------------------------------------------------------------------------------------------------
def chain_step(V, X0, Ws, which, beta, l1=0.0, l2=0.0, ortho=0.0, gamma=None):
    """``BetaMu._chain_step`` for parameter ``which`` (0 = X0, k = W_k) of prediction = X0 W1^T ... Wn^T.
    Returns dict(new, grad, bound, grad_bound, neg, pos)."""
    X0 = np.asarray(X0, dtype=np.float64)
    Ws = [np.asarray(W, dtype=np.float64) for W in Ws]
    gamma = mu_gamma(beta) if gamma is None else gamma
    xs, ex = [X0], [np.zeros_like(X0)]
    for W in Ws:                                        # forward products
        ex.append(matmul_bound(xs[-1], W, err_a=ex[-1]))
        xs.append(matmul(xs[-1], W))
    gn, gp = terms(xs[-1], V, beta)                     # seeds
    bn, bp = terms_bound(xs[-1], V, beta, s_err=ex[-1])

    def back(G, eG):                                    # back-propagated products
        k = len(Ws)
        while True:
            if which == k:                              # dW_k = G_k^T X_{k-1}
                return matmul(G.T, xs[k - 1].T), matmul_bound(G.T, xs[k - 1].T, err_a=eG.T, err_b=ex[k - 1].T)
            G, eG = matmul(G, Ws[k - 1].T), matmul_bound(G, Ws[k - 1].T, err_a=eG)
            k -= 1
            if k == 0:
                return G, eG
    neg, eneg = back(gn, bn)
    pos, epos = back(gp, bp)
    theta = X0 if which == 0 else Ws[which - 1]
    new, grad = update(theta, neg, pos, gamma, l1, l2, ortho)
    bound = update_bound(theta, neg, pos, gamma, l1, l2, ortho, c_rs=rowsum_ops_update(theta.shape[1]),
                         neg_err=eneg, pos_err=epos)
    return dict(new=new, grad=grad, bound=bound, grad_bound=eneg + epos + U * np.abs(grad), neg=neg, pos=pos)


def chain_step_f32(V, X0, Ws, which, beta, l1=0.0, l2=0.0, ortho=0.0, fault=None):
    """The same step with every stage in np.float32 (``matmul_f32``, ``terms_f32``, ``update_f32``).  ``fault``: a
    ``MATMUL_FAULTS`` mistake in the forward products."""
    xs = [np.asarray(X0, dtype=F32)]
    Ws = [np.asarray(W, dtype=F32) for W in Ws]
    for W in Ws:
        xs.append(matmul_f32(xs[-1], W, fault))
    gn, gp = terms_f32(xs[-1], V, beta)

    def back(G):
        k = len(Ws)
        while True:
            if which == k:
                return matmul_f32(np.ascontiguousarray(G.T), np.ascontiguousarray(xs[k - 1].T))
            G = matmul_f32(G, np.ascontiguousarray(Ws[k - 1].T))
            k -= 1
            if k == 0:
                return G
    theta = xs[0] if which == 0 else Ws[which - 1]
    return update_f32(theta, back(gn), back(gp), mu_gamma(beta), l1, l2, ortho)


# ---- shared case generators (CPU and GPU tests see the same arrays) -----------------------------------------------------
PENALTIES = {'off': (0.0, 0.0, 0.0), 'l1': (f32(1e-3), 0.0, 0.0), 'l2': (0.0, f32(1e-3), 0.0), 'ortho': (0.0, 0.0, f32(1e-2)),
             'all': (f32(1e-3), f32(1e-3), f32(1e-2))}
UPDATE_SHAPES = [(1, 1), (3, 255), (2, 256), (5, 257), (4, 1000), (70000, 3)]
UPDATE_BETAS = (1.0, 0.0, 0.5, 3.0)          # gamma 1, 1/2, 2/3, 1/2


def update_problem(rows: int, cols: int):
    """(theta, neg, pos) fp32: positive theta; neg / pos of order 1 with negative entries (the relu branch), exact zeros
    (alone and in both at once: eps / eps) and, where the row has more than one element, one row made of one large value
    and many tiny ones (rowsum - theta cancels)."""
    g = np.random.default_rng(rows * 1009 + cols)
    theta = (np.abs(g.standard_normal((rows, cols))) + 0.05).astype(F32)
    neg = (g.random((rows, cols)) * 2).astype(F32)
    pos = (g.random((rows, cols)) * 2 + 0.05).astype(F32)
    sel = g.random((rows, cols))
    neg[sel < 0.06] *= F32(-1)
    pos[(sel > 0.04) & (sel < 0.10)] *= F32(-1)
    neg[(sel > 0.20) & (sel < 0.26)] = 0
    pos[(sel > 0.24) & (sel < 0.30)] = 0
    if rows * cols > 1:
        pos.flat[1], neg.flat[1] = 0, 0                 # one certain 0 / 0
        neg.flat[0] = -abs(neg.flat[0]) - F32(0.5)      # one certain negative numerator
    if cols > 1:
        theta[rows - 1] = (g.random(cols) * 1e-4 + 1e-6).astype(F32)
        theta[rows - 1, cols // 2] = F32(1e4)
    return theta, neg, pos


TERMS_BETAS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
TERMS_SIZES = (1, 255, 257, 4096 * 256 + 257)


def terms_problem(n: int):
    """(s, v) fp32: s among exact 0 (-> eps), ~1e-6, order 1 and ~1e4; v in [0, 1) with exact zeros."""
    g = np.random.default_rng(n)
    band = g.integers(0, 4, n) if n > 1 else np.array([2])
    base = g.random(n) * 0.9 + 0.1
    s = np.choose(band, [np.zeros(n), base * 1e-6, base * 3.0, base * 1e4]).astype(F32)
    v = g.random(n)
    v[g.random(n) < 0.1] = 0.0
    if n > 4:
        s[:4] = [0.0, 1e-6, 1.0, 1e4]
        v[4] = 0.0
    return s, v.astype(F32)


RECON_MK = [(1, 1), (31, 33), (33, 127), (127, 128), (128, 129), (129, 257), (257, 31)]
RECON_R = (1, 2, 3, 4, 31, 32, 33, 36, 65)


def recon_problem(M: int, K: int, R: int, one_hot=False):
    """(A [M, R], B [K, R]) fp32: signed normal values, or a one-hot A (row m selects rank ``one_hot_rank(M, K, R)[m]``)."""
    g = np.random.default_rng((M * 263 + K) * 67 + R)
    B = g.standard_normal((K, R)).astype(F32)
    if one_hot:
        A = np.zeros((M, R), dtype=F32)
        A[np.arange(M), one_hot_rank(M, K, R)] = 1
    else:
        A = g.standard_normal((M, R)).astype(F32)
    return A, B


def one_hot_rank(M: int, K: int, R: int):
    """A drawn map, not a linear one: rows 4, 8 or 32 apart (the strides of the MFMA output lane map) must not share a rank
    by construction, which (a m + b) mod R does for every R dividing 4 a."""
    return np.random.default_rng((M * 263 + K) * 67 + R + 1).integers(0, R, M)


# One-layer (fused) cases: N x C target, rank, operand mode, beta, penalties, forced contraction split (None = the
# library's own), what the case is there for.
FUSED_CASES = [
    dict(id='r5-b1-ns25', N=50, C=6200, R=5, prec='bf16x3', beta=1.0, pen='off', nsplit=25,
         why='25 contraction splits in the H step: rounds of 16, of 8 and single slabs; 50 rows (no multiple of 16)'),
    dict(id='r5-b1-pen-tall', N=32600, C=40, R=5, prec='bf16x3', beta=1.0, pen='all', nsplit=None,
         why='H has 32768 padded rows = 512 stripes of 64: the 64-row instance, penalties on'),
    dict(id='r5-b1-tiny-colsum', N=90, C=70, R=5, prec='bf16x3', beta=1.0, pen='off', nsplit=1, tiny_col=2,
         why='rank column 2 of H sums to ~1e-6: eps is 10 % of the closed-form denominator of the W step'),
    dict(id='r33-b2-pen-ns3', N=130, C=1100, R=33, prec='bf16x3', beta=2.0, pen='all', nsplit=3, why='three slabs'),
    dict(id='r33-b0.5-ns1', N=77, C=203, R=33, prec='bf16x3', beta=0.5, pen='off', nsplit=1, why='one slab, powf(., 2/3)'),
    dict(id='r33-b3-ortho', N=61, C=300, R=33, prec='bf16x3', beta=3.0, pen='ortho', nsplit=None, why='ortho alone'),
    dict(id='r100-b0-ortho', N=200, C=330, R=100, prec='bf16x3', beta=0.0, pen='ortho', nsplit=None, why='ortho alone'),
    dict(id='r100-b3-pen-ns3', N=300, C=1100, R=100, prec='bf16x3', beta=3.0, pen='all', nsplit=3, why='three slabs'),
    dict(id='r128-b1-pen', N=257, C=520, R=128, prec='bf16x3', beta=1.0, pen='all', nsplit=None, why='full rank tile'),
    dict(id='r128-b0.5-ortho-ns3', N=130, C=1100, R=128, prec='bf16x3', beta=0.5, pen='ortho', nsplit=3, why='three slabs'),
    dict(id='r128-b2-ns1', N=200, C=300, R=128, prec='bf16x3', beta=2.0, pen='off', nsplit=1, why='one slab'),
    dict(id='r200-f16-b2-pen', N=300, C=640, R=200, prec='f16', beta=2.0, pen='all', nsplit=2, why='padded rank 256, fp16'),
]


def fused_problem(case):
    """(V, W0, H0) fp32 numpy."""
    N, C, R = case['N'], case['C'], case['R']
    g = np.random.default_rng(N * 7 + C * 3 + R)
    V = g.random((N, C)).astype(F32)
    if case['beta'] <= 0:
        V = V + F32(2.0 ** -7)
    W0 = (np.abs(g.standard_normal((C, R))) + 0.05).astype(F32)
    H0 = (np.abs(g.standard_normal((N, R))) + 0.05).astype(F32)
    if case.get('tiny_col') is not None:
        H0[:, case['tiny_col']] = (g.random(N) * 2e-6 / N).astype(F32)
    return V, W0, H0


CHAIN_SHAPES = dict(X0=(37, 5), W1=(33, 5), W2=(130, 33), W3=(70, 130))
CHAIN_BETAS = (1.0, 0.5, 2.0)
CHAIN_PENS = ('off', 'all')


def chain_problem():
    """(V, X0, [W1, W2, W3]) fp32 numpy: ranks 5, 33 and 130, no size a multiple of the 128-tile."""
    g = np.random.default_rng(12)
    mk = lambda shape: (np.abs(g.standard_normal(shape)) * 0.5 + 0.05).astype(F32)
    X0 = mk(CHAIN_SHAPES['X0'])
    Ws = [mk(CHAIN_SHAPES[k]) for k in ('W1', 'W2', 'W3')]
    V = (g.random((37, 70)) * 50).astype(F32)
    return V, X0, Ws


CONV_BETAS = (1.0, 0.5)
CONV_ORTHO = f32(1e-2)


def conv_problem():
    """(V 2x40x96, W0 40x5x8, H0 2x5x89) fp32 numpy."""
    g = np.random.default_rng(14)
    V = g.random((2, 40, 96)).astype(F32)
    W0 = np.abs(g.standard_normal((40, 5, 8))).astype(F32)
    H0 = np.abs(g.standard_normal((2, 5, 89))).astype(F32)
    return V, W0, H0


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; 0 / 0 counts as 0, a non-finite ``got`` or an error over a zero bound as inf."""
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isfinite(got), ratio, np.inf).max())
