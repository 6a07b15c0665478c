"""Float64 reference of PLCA on a sparse-COO target (csrc/nmfmu_sparse_plca.hip, plca._SparsePlcaEM), test-only: g, both
numerator planes and the tracked loss from DENSE formulas -- the normalised target Vn (0 where nothing is stored), its mask M:

    S = H diag(Z) W^T,   G = Vn / (S + eps)         (reference plca.py:252-253; G = 0 wherever Vn is)
    H side: num_H = G W        W side: num_W = G^T H
    loss  : sum over ALL N x C of x (log(x + eps) - log(s + eps)) - x + s          (metrics.py:22 on the densified target)

and a float64 ``fit`` built from them and from ``plca_emulation.em_step`` (the M-step, plca.py:253-290).

Nothing on this path is rounded to 16 bits: what separates the kernels from this module is fp32 arithmetic alone, and every
element is held to the bound the standard model gives for the operations the kernel performs on it (the rule of
tests/masked_emulation.py: a sum of n terms, every term passing through at most k roundings, is within k u sum |terms| of the
exact one to first order; u = 2^-24; times ``SECOND`` = 1 + 2^-10 for the neglected products of errors, as in
tests/plca_emulation.py -- the largest k here is below 64).  No bound is taken from a run.  From the kernel source:

* sp_plca_estep_kernel, the roundings behind g (``g_ops``): the owner row is scaled by z once per segment (one multiply), one
  multiply per product, at most RL additions into the lane's partial, six butterfly additions, ``+ eps``, the divide:
  1 + 1 + RL + 6 + 1 + 1 = RL + 10.  Every term of s is >= 0, so these are relative: |dg| <= (RL + 10) u g.  (A product and
  its addition contracted into one fma: fewer roundings, same bound.)
* every term g b of a numerator is one multiply and joins its accumulator through at most ``count`` additions inside the
  segments (storage order) and ``segments - 1`` in the finishing kernel: k = count + segments + g_ops, bound
  k u sum |g panel| -- ``estep`` (num_H) and ``estep``'s num_W, both against the float64 g.
* sp_plca_gather_kernel reads g back: it holds only the one multiply per term.  ``gather`` takes g as GIVEN (the device's own
  fp32 plane, exact input): k = count + segments.
* the loss (``loss``): H * Z is one fp32 multiply (torch), ``nmfmu_sp_div_forward`` forms s from it with one multiply per
  product, RL additions and six butterfly additions, ``+ eps``: se is relative (RL + 9) u; logf is a 1-ulp = 2 u function
  (ULP_FN); v * logf one multiply; the terms are widened and summed in double.  sum_all s = sum_r Z_r colsum(H)_r
  colsum(W)_r with the fp32 column sums of ``nmfmu_rank_sums`` (``chain_rank_sums``: a thread's strided partial, the
  combination of its four partials, the LDS trees) multiplied and summed in double.  The terms of vn alone are float64 on
  the host.
"""
from __future__ import annotations

import numpy as np

import masked_emulation as M
import mu_emulation as E
import plca_emulation as P

EPS = E.EPS
U = 2.0 ** -24
SECOND = P.SECOND
ULP_FN = M.ULP_FN
rank_slots = M.rank_slots
segments = M.segments
bound_err = M.bound_err
dense = M.dense


def g_ops(R: int) -> int:
    """Roundings behind one g of sp_plca_estep_kernel (module docstring)."""
    return rank_slots(E.pad_rank(R)) + 10


def normalise(idx, vals, W, H, Z):
    """(vals_n, W, H, Z) fp32 as ``PLCA`` and its ``fit`` normalise them: the factors over everything but the rank axis,
    the stored values by their fp32 total."""
    f32 = np.float32
    vals, W, H, Z = (np.asarray(a, dtype=f32) for a in (vals, W, H, Z))
    return ((vals / vals.sum(dtype=f32)).astype(f32), (W / W.sum(0, dtype=f32)).astype(f32),
            (H / H.sum(0, dtype=f32)).astype(f32), (Z / Z.sum(dtype=f32)).astype(f32))


def _side_bound(Gabs, panel, M_, k_extra, chunk):
    count = M_.sum(1)
    k = count + segments(count, chunk) + k_extra
    return count, SECOND * (k * U)[:, None] * (Gabs @ np.abs(panel))


def estep(idx, vals_n, shape, H, W, Z, chunk: int = 512):
    """dict(g, g_bound [nnz] in CSR order; num_h, num_h_bound, count_h [N ...]; num_w, num_w_bound, count_w [C ...])."""
    H, W, Z = (np.asarray(a, np.float64) for a in (H, W, Z))
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    Vn, Mk = dense(idx, vals_n, shape)
    S = H @ (W * Z).T
    G = np.where(Mk, Vn / (S + EPS), 0.0)
    ops = g_ops(H.shape[1])
    g = G[idx[0], idx[1]]
    count_h, bh = _side_bound(G, W, Mk, ops, chunk)
    count_w, bw = _side_bound(G.T, H, Mk.T, ops, chunk)
    return dict(g=g, g_bound=SECOND * ops * U * np.abs(g), G=G, num_h=G @ W, num_h_bound=bh, count_h=count_h,
                num_w=G.T @ H, num_w_bound=bw, count_w=count_w)


def gather(idx, g, shape, H, chunk: int = 512):
    """(num_w, bound, count) of the W side from a GIVEN g (CSR order; exact input): one multiply per term."""
    H = np.asarray(H, np.float64)
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    G, Mk = dense(idx, g, shape)
    count, b = _side_bound(np.abs(G.T), H, Mk.T, 0, chunk)
    return G.T @ H, b, count


def chain_rank_sums(rows: int) -> int:
    """Longest chain of fp32 additions behind one column sum of nmfmu_rank_sums (inner == 1).  Up to 2^14 rows: one block
    of 1024 threads, four strided partials per thread (the tail loop adds onto the first), their combination, a 10-level
    LDS tree.  Above: 128 chunks of 256 threads (8 levels) and a 7-level tree over the chunk partials."""
    if rows <= 1 << 14:
        return -(-rows // 4096) + 3 + 2 + 10
    per = -(-rows // 128)
    return -(-per // 1024) + 3 + 2 + 8 + 7


def dense_loss(idx, vals_n, shape, H, W, Z) -> float:
    """metrics.py:22 on the densified target, every entry."""
    H, W, Z = (np.asarray(a, np.float64) for a in (H, W, Z))
    Vn, _ = dense(idx, vals_n, shape)
    S = H @ (W * Z).T
    return float((Vn * (np.log(Vn + EPS) - np.log(S + EPS)) - Vn + S).sum())


def loss(idx, vals_n, shape, H, W, Z):
    """(the same quantity regrouped as the device forms it, its bound)."""
    H, W, Z = (np.asarray(a, np.float64) for a in (H, W, Z))
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    v = np.asarray(vals_n, np.float64)
    s = np.einsum('pr,pr->p', H[idx[0]] * Z, W[idx[1]]) if len(v) else np.zeros(0)
    lg = np.log(s + EPS)
    e_se = rank_slots(E.pad_rank(H.shape[1])) + 9.0
    v_term = float(v @ np.log(v + EPS) - v.sum())
    neg = v * lg
    neg_b = U * v * (e_se + (ULP_FN + 1) * np.abs(lg))
    csh, csw = H.sum(0), W.sum(0)
    pos_t = Z * csh * csw
    pos_b = U * (chain_rank_sums(H.shape[0]) + chain_rank_sums(W.shape[0])) * pos_t
    total = v_term + pos_t.sum() - neg.sum()
    bound = SECOND * (neg_b.sum() + pos_b.sum()) + (len(v) + len(Z) + 8) * 2.0 ** -53 * (np.abs(neg).sum() + pos_t.sum()
                                                                                        + abs(v_term))
    return float(total), float(bound) + 1e-300


def fit(idx, vals, shape, W_init, H_init, Z_init, tol=1e-4, max_iter=200, alphas=(1.0, 1.0, 1.0), train=(True, True, True)):
    """The reference's fit (plca.py:236-304) in float64 over the stored entries: (W, H, Z, n_iter, norm, tracked losses).
    ``*_init``: the factors as the constructor normalised them.  The prior constant stays a double, as in a float64 run of
    the reference."""
    vals = np.asarray(vals, np.float64)
    norm = float(vals.sum())
    vn = vals / norm
    W, H, Z = (np.asarray(a, np.float64) for a in (W_init, H_init, Z_init))
    V, _ = dense(idx, vals, shape)

    def track():      # plca.py:245-247, 293-295: kl_div(WZH * norm, V * norm) -- eps beside the UNnormalised arguments
        Sn = (H @ (W * Z).T) * norm
        return float(np.sqrt(2.0 * (V * (np.log(V + EPS) - np.log(Sn + EPS)) - V + Sn).sum()))
    losses = [track()]
    prev, n_iter = losses[0], -1
    for n_iter in range(max_iter):
        t = estep(idx, vn, shape, H, W, Z)
        r = P.em_step(W, H, Z, t['num_w'], t['num_h'], train, alphas, u=2.0 ** -53, rounding=False)
        W, H, Z = r['W'].v, r['H'].v, r['Z'].v
        if n_iter % 10 == 9:
            losses.append(track())
            if (prev - losses[-1]) / losses[0] < tol:
                break
            prev = losses[-1]
    return W, H, Z, n_iter, norm, losses


# ---- the problems of tests/test_gpu_sparse_plca.py ---------------------------------------------------------------------------
def make_problem(N: int, C: int, R: int, axis: int = 0):
    """(idx, vals_n, W, H, Z) fp32: the pattern of ``masked_emulation.make_problem`` (the owner ``axis`` cycles through 0, 1, 4,
    5, 8, 9 and 20 stored entries; index 3 of the other axis holds none), the factors normalised as PLCA normalises them,
    the values summing to 1."""
    idx, vals, W0, H0 = M.make_problem(N, C, R, axis)
    g = np.random.default_rng(31 * R + axis)
    Z0 = (g.random(R) * 0.9 + 0.1).astype(np.float32)
    return (idx,) + normalise(idx, vals, W0, H0, Z0)
