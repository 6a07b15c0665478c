"""float64 numpy model of ``NMF.fit(solver='hals')`` (torchnmf_amd/hals.py, csrc/nmfmu_hals.hip) and the per-element check of
the sweep kernel.  No torch, no GPU: the CPU tests exercise it on its own, the GPU tests compare the device against it.

Conventions as in the package: ``V (N, C) ~ H (N, R) @ W (C, R)^T``; an iteration is the W half-step, then the H half-step
with the new W; ``eps = 2^-23``.
"""
import numpy as np

EPS = 2.0 ** -23
U = 2.0 ** -24          # unit roundoff of fp32


def sweep(F, A, G, l1=0.0, l2=0.0, floor=EPS, den_eps=EPS):
    """One Gauss-Seidel pass over the rank on a copy of ``F [rows, R]``: for r = 0 .. R-1, every row on its own,
    ``F[:, r] = max(floor, (A[:, r] - l1 - sum_{j != r} F[:, j] G[j, r]) / (G[r, r] + l2 + den_eps))``."""
    F = np.array(F, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    for r in range(F.shape[1]):
        s = F @ G[:, r] - F[:, r] * G[r, r]
        F[:, r] = np.maximum(floor, (A[:, r] - l1 - s) / (G[r, r] + l2 + den_eps))
    return F


def half_step(X_owner, F, P, l1=0.0, l2=0.0, floor=EPS, den_eps=EPS):
    """The sweep of the owner ``F`` against the panel ``P``: ``A = X_owner @ P`` (V^T H for W, V W for H), ``G = P^T P``."""
    P = np.asarray(P, dtype=np.float64)
    return sweep(F, np.asarray(X_owner, dtype=np.float64) @ P, P.T @ P, l1, l2, floor, den_eps)


def divergence(V, W, H):
    """1/2 |V - H W^T|^2: the loss ``fit`` tracks (no regularisation terms)."""
    return 0.5 * float(((V - H @ W.T) ** 2).sum())


def objective(V, W, H, l1=0.0, l2=0.0):
    """What the sweeps descend on: the divergence plus l1 (sum W + sum H) + l2 / 2 (|W|^2 + |H|^2)."""
    return divergence(V, W, H) + l1 * (W.sum() + H.sum()) + 0.5 * l2 * ((W ** 2).sum() + (H ** 2).sum())


def optimal_scale(V, W, H):
    """argmin_a |V - a H W^T|^2 = <V W, H> / <H^T H, W^T W>."""
    return float(((V @ W) * H).sum() / ((H.T @ H) * (W.T @ W)).sum())


def init_scale(V, W, H, train_W=True, train_H=True):
    """The step before the first iteration: both factors trainable -> each times sqrt(a); one -> that one times a; skipped
    when a is not finite or <= 0; the trainable factors clamped to >= eps afterwards.  Returns new (W, H)."""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    a = optimal_scale(V, W, H)
    if np.isfinite(a) and a > 0:
        if train_W and train_H:
            W, H = W * a ** 0.5, H * a ** 0.5
        elif train_W:
            W = W * a
        elif train_H:
            H = H * a
    if train_W:
        W = np.maximum(W, EPS)
    if train_H:
        H = np.maximum(H, EPS)
    return W, H


def fit(V, W, H, max_iter, tol=-1e300, l1=0.0, l2=0.0, train_W=True, train_H=True, trace=None):
    """``NMF.fit(V, beta=2, tol, max_iter, solver='hals')`` in float64 -> (W, H, n_iter).  ``trace``: a list that receives the
    objective after the initial scaling and after every half-step."""
    V = np.asarray(V, dtype=np.float64)
    W, H = init_scale(V, W, H, train_W, train_H)
    if trace is not None:
        trace.append(objective(V, W, H, l1, l2))
    loss_init = previous = (2.0 * divergence(V, W, H)) ** 0.5
    n_iter = -1
    for n_iter in range(max_iter):
        if train_W:
            W = half_step(V.T, W, H, l1, l2)
            if trace is not None:
                trace.append(objective(V, W, H, l1, l2))
        if train_H:
            H = half_step(V, H, W, l1, l2)
            if trace is not None:
                trace.append(objective(V, W, H, l1, l2))
        if n_iter % 10 == 9:
            loss = (2.0 * divergence(V, W, H)) ** 0.5
            if (previous - loss) / loss_init < tol:
                break
            previous = loss
    return W, H, n_iter + 1


def mu_fit(V, W, H, n_iter):
    """float64 multiplicative update for beta = 2 (nmf.py:78-92 with l1 = l2 = 0, gamma = 1), from the factors as given."""
    V = np.asarray(V, dtype=np.float64)
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    for _ in range(n_iter):
        W = W * ((V.T @ H + EPS) / (W @ (H.T @ H) + EPS))
        H = H * ((V @ W + EPS) / (H @ (W.T @ W) + EPS))
    return W, H


# ---- the per-element check of nmfmu_hals_sweep -------------------------------------------------------------------------
def bound_c(rank):
    """c(R) of the running-error bound, counted on the kernel's accumulation scheme (csrc/nmfmu_hals.hip): term j of the dot
    product goes to accumulator j mod 4 by fused multiply-add -- at most ceil(R / 4) roundings on a term -- and the four are
    combined as (acc0 + acc1) + (acc2 + acc3): 2 more.  (a - l1) and (.. - s) round once each: 2.  The denominator
    (g_rr + l2) + eps is a sum of non-negative terms rounded twice; its relative error moves the quotient by at most that
    fraction of |numerator| / den <= (|a| + l1 + sum |f g|) / den: 2.  One more for the second-order terms, which
    (1 + u)^(c) - 1 <= (c + 1) u covers for c u < 0.01."""
    return (rank + 3) // 4 + 2 + 2 + 2 + 1


def sweep_check(got, old, A, G, l1=0.0, l2=0.0):
    """The Gauss-Seidel fixed point, per element, from the device's OWN output: for every (row, r), in float64,
        want = max(eps, (A - l1 - sum_{j<r} got[j] G[j, r] - sum_{j>r} old[j] G[j, r]) / (G[r, r] + l2 + eps))
    with l1, l2 rounded to fp32 first (what the C entry receives), and
        bound = c(R) u (|A| + l1 + sum |f G|) / den + 2 u |want|
    (2 u |want|: the division's own rounding, and slack for the fp32 representation of the result).  max(eps, .) is
    1-Lipschitz, so |got - want| <= bound holds on either side of the clamp whenever the unclamped values are within bound.
    Returns (err, bound), both [rows, R] float64."""
    got, old = np.asarray(got, dtype=np.float64), np.asarray(old, dtype=np.float64)
    A, G = np.asarray(A, dtype=np.float64), np.asarray(G, dtype=np.float64)
    l1, l2 = float(np.float32(l1)), float(np.float32(l2))
    rows, R = got.shape
    err, bound = np.empty((rows, R)), np.empty((rows, R))
    c = bound_c(R)
    for r in range(R):
        mix = np.concatenate([got[:, :r], np.zeros((rows, 1)), old[:, r + 1:]], axis=1)
        s = mix @ G[:, r]
        mag = np.abs(mix) @ np.abs(G[:, r])
        den = G[r, r] + l2 + EPS
        want = np.maximum(EPS, (A[:, r] - l1 - s) / den)
        err[:, r] = np.abs(got[:, r] - want)
        bound[:, r] = c * U * (np.abs(A[:, r]) + l1 + mag) / den + 2 * U * np.abs(want)
    return err, bound


def sweep_case(rows, rank, seed=0):
    """Inputs of the sweep test, fp32: (F [rows, rank], A [rows, rank], G [rank, rank] symmetric).  The panel behind G has one
    all-floor column (G[r, r] ~ 0; not at rank 1), A = X @ panel for a noisy target X whose exact factor has 30 % zeros, so that some coordinates clamp and others do
    not, and one row of A is all zero."""
    rng = np.random.default_rng(seed + 1000 * rows + rank)
    n = 40
    P = np.abs(rng.standard_normal((n, rank)))
    if rank > 1:                      # (at rank 1 it would be the only column: every row would sit on the floor)
        P[:, rank // 2] = EPS
    F_true = np.abs(rng.standard_normal((rows, rank))) * (rng.random((rows, rank)) < 0.7)
    X = (F_true @ P.T) * (0.5 + rng.random((rows, n)))
    A = X @ P
    A[rows // 2] = 0.0
    F = np.maximum(np.abs(rng.standard_normal((rows, rank))) * 0.3, EPS)
    G = (P.T @ P).astype(np.float32)
    G = np.maximum(G, G.T)            # (bitwise symmetric after the rounding, as nmfmu_gram's output is)
    return F.astype(np.float32), A.astype(np.float32), G


def fit_case(name):
    """The two targets of the convergence tests: (V, W0, H0) in float64, values exactly representable in fp32."""
    if name == 'dense':
        rng = np.random.default_rng(3)
        n, c, r = 200, 130, 33
        V = rng.random((n, c))
    else:
        rng = np.random.default_rng(7)
        n, c, r = 300, 257, 64
        V = rng.random((n, c)) * (rng.random((n, c)) < 0.05)
    W0 = np.abs(rng.standard_normal((c, r)))
    H0 = np.abs(rng.standard_normal((n, r)))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return f32(V), f32(W0), f32(H0)
