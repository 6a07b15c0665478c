"""Float64 reference of ``sparse_beta_div`` (csrc/nmfmu_sparse_autograd.hip, torchnmf_amd/sparse_autograd.py), test-only:
the value ``V_norm + pos - neg``, both gradients, and the per-element bound the standard model of fp32 arithmetic gives for
the operations the kernels perform (the style and the helpers of tests/sparse_emulation.py; u = 2^-24).

Constants, read off the kernel sources (never tuned to a measurement):

* ``sp_div_forward_kernel``: s = <owner[row], panel[col]> is the dot product of ``sp_partial_kernel``: one multiply, at most RL
  additions into the lane's partial, six butterfly additions -- relative (RL + 7) u, all terms >= 0.  The data term is
  ``sparse_emulation.loss_neg``'s (logf at 2 u, + eps, the multiply by v; the sum itself runs in float64).
* ``sp_div_backward_kernel``: g = v / (s + eps) from the SAVED s: (RL + 7) for s, + eps, the divide -- ``sparse_emulation.ops_g``
  (the first-order effect of s's error on g); beta == 2: g = v, exact.  Every term g * panel[col][r] is one multiply and
  joins its segment's accumulator through at most min(count, chunk) additions (storage order); a split row's partials are
  added in ``sp_div_finish_kernel`` through (segments - 1) more; one more rounding in the subtraction pos - acc (on a
  result of magnitude <= |pos| + sum |g panel|) and one in the multiplication by up.  So
      |got - ref| <= |up| (bound_pos + u (2 |pos| + (min(count, chunk) + segments + 1 + ops_g + 2) sum |g panel|))
  which is ABSOLUTE: the gradient is a difference and may cancel.
* pos, beta == 1: the panel's column sums from ``nmfmu_rank_sums`` (``colsum_ops`` below counts its additions); beta == 2: the
  plane ``nmfmu_rowmat`` makes of the owner and ``nmfmu_gram`` of the panel (``sparse_emulation.rowmat``'s bound).
* the value: ``sparse_emulation.v_norm_bound`` (float64 on the host) + the two column sums / Gram matrices behind pos
  (their dot product runs in float64) + ``loss_neg``'s bound + the rounding of the result to fp32.
"""
from __future__ import annotations

import numpy as np

import mu_emulation as E
import sparse_emulation as S

U = S.U
EPS = S.EPS
RANK_CHUNKS = 128      # kRankChunks


def colsum_ops(rows: int) -> int:
    """Additions behind one column sum of ``nmfmu_rank_sums`` (inner = 1).  Up to 2^14 rows: one workgroup of 1024 threads,
    four accumulators per thread (the remainder loop feeds the first: at most ceil(rows / 4096) + 3 additions), two to
    combine them, a ten-level tree.  Above: 128 ranges of ceil(rows / 128), 256 threads (ceil(per / 1024) + 3, two, an
    eight-level tree), then a seven-level tree over the ranges."""
    if rows <= (1 << 14):
        return -(-rows // 4096) + 3 + 2 + 10
    per = -(-rows // RANK_CHUNKS)
    return -(-per // 1024) + 3 + 2 + 8 + 7


def segments(count, chunk: int):
    count = np.asarray(count, dtype=np.int64)
    return np.maximum(1, -(-count // chunk))


def side(csr_, owner, panel, beta: float, up: float, chunk: int):
    """(grad float64 [rows, R], bound) of one factor: ``owner`` is the factor differentiated, ``csr_`` the target stored
    over its rows."""
    owner = np.asarray(owner, dtype=np.float64)
    panel = np.asarray(panel, dtype=np.float64)
    em = S.numerator(csr_, owner, panel, beta)
    if beta == 1:
        cs = S.colsum(panel)
        pos = np.broadcast_to(cs, owner.shape)
        bpos = np.broadcast_to(colsum_ops(len(panel)) * U * np.abs(panel).sum(0), owner.shape)
    else:
        g, _ = S.gram(panel)
        pos, bpos = S.rowmat(owner, g, len(panel))
    count = em['count']
    k_acc = np.minimum(count, chunk) + segments(count, chunk) + 1 + em['g_ops'] + 2
    grad = up * (pos - em['num'])
    bound = abs(up) * (bpos + U * (2 * np.abs(pos) + k_acc[:, None] * em['abs_sum']))
    return grad, bound


def value(csr_h, H, W, beta: float):
    """(V_norm + pos - neg in float64, its bound)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    vals = csr_h[2]
    vn, bvn = S.v_norm(vals, beta), S.v_norm_bound(vals, beta)
    if beta == 1:
        pos = float(W.sum(0) @ H.sum(0))
        bpos = (colsum_ops(len(H)) + colsum_ops(len(W)) + 1) * U * float(np.abs(W).sum(0) @ np.abs(H).sum(0))
    else:
        pos, bpos = S.loss_pos(H, W, 2)
    neg, bneg = S.loss_neg(csr_h, H, W, beta)
    loss = vn + pos - neg
    return loss, bvn + bpos + bneg + U * abs(loss) + 2.0 ** -50 * (abs(vn) + abs(pos) + abs(neg))


def evaluate(idx, vals, shape, H, W, beta: float, up: float = 1.0, chunk: int = 512):
    """Everything for one problem; ``idx`` / ``vals`` are the COALESCED entries ([2, nnz] int64, fp32)."""
    N, C = shape
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    csr_h = S.csr(idx[0], idx[1], vals, N)
    csr_w = S.csr(idx[1], idx[0], vals, C)
    loss, bloss = value(csr_h, H, W, beta)
    gH, bH = side(csr_h, H, W, beta, up, chunk)
    gW, bW = side(csr_w, W, H, beta, up, chunk)
    return dict(loss=loss, loss_bound=bloss, gH=gH, gH_bound=bH, gW=gW, gW_bound=bW)


def dense_value_bound(H, W, Vd, beta: float) -> float:
    """Bound of ``beta_div(reconstruct(H, W), Vd, beta)`` (``beta_div_kernel`` / ``loss_elem``) against float64, to first
    order: the fp32 reconstruction S is a dot product of length R ((R + 2) u S), the elementwise term is evaluated in
    fp32 and summed in float64, the result is rounded to fp32.
      beta 2: d = S - x: (R + 2) u S + u |d|;  1/2 d d: |d| err(d) + u d^2 / 2
      beta 1: A = x (log2(x + eps) - log2(S + eps)) ln 2 with v_log_f32 at 2 u each, the subtraction, the two multiplies and
              the rounded constant; then A - x and + ((S + eps) - eps), one rounding each on top of S's own error."""
    H, W, Vd = np.asarray(H, np.float64), np.asarray(W, np.float64), np.asarray(Vd, np.float64)
    R = H.shape[1]
    Sx = H @ W.T
    if beta == 2:
        d = Sx - Vd
        ed = (R + 2) * U * Sx + U * np.abs(d)
        b = np.abs(d) * ed + U * 0.5 * d * d
        total = float((0.5 * d * d).sum())
    else:
        se = Sx + EPS
        lx, ls = np.log2(Vd + EPS), np.log2(se)
        A = Vd * (lx - ls) * S.LN2
        eA = Vd * S.LN2 * (S.ULP_FN * U * (np.abs(lx) + np.abs(ls)) + (R + 3) * U / S.LN2 + U * np.abs(lx - ls)) + 3 * U * np.abs(A)
        es = (R + 4) * U * se
        t = A - Vd + Sx
        b = eA + U * np.abs(A - Vd) + es + U * np.abs(t)
        total = float(t.sum())
    return float(b.sum()) + U * abs(total)


def known_log_eps_term(vals) -> float:
    """dense - sparse at beta == 1: the dense divergence has v log(v + eps) where the sparse V_norm has v log v."""
    v = np.asarray(vals, dtype=np.float64)
    return float(np.sum(v * (np.log(v + EPS) - np.log(v))))


def pad_rank(R: int) -> int:
    return E.pad_rank(R)
