"""float64 numpy model of ``NMF.fit(solver='ccd', unstored=omega)`` (torchnmf_amd/wccd.py, csrc/nmfmu_sparse_wccd.hip): the
recurrence, a dense brute force on an explicit weight matrix, the whole procedure, an fp32 model of the kernel's own arithmetic
and the per-element check of the sweep kernel.  No torch, no GPU: the CPU tests exercise it on its own, the GPU tests compare
the device against it.

Conventions as in tests/ccd_emulation.py (whose work lists, cases and helpers it uses): ``V (N, C) ~ H (N, R) @ W (C, R)^T``;
stored entries carry weight 1, every unstored entry is a zero of weight ``omega``, 0 < omega < 1 (the recurrence itself is
defined for 0 <= omega <= 1: the CPU tests use the end points); ``c = 1 - omega``; ``eps = 2^-23``.
"""
import numpy as np

import ccd_emulation as CE

EPS, U, LIMIT, WG_WAVES = CE.EPS, CE.U, CE.LIMIT, CE.WG_WAVES
side_list, sweep_case, zero_row, fit_case, fraction, scores = (CE.side_list, CE.sweep_case, CE.zero_row, CE.fit_case,
                                                               CE.fraction, CE.scores)
Q_SLOTS = 4             # owner coordinates a lane holds: the length of its chain of q


def minimiser(f, d, n, q, gkk, omega, l1, l2):
    D = (1.0 - omega) * d + omega * gkk
    return np.maximum(EPS, (n - omega * q + f * D - l1) / (D + l2 + EPS))


def sweep(F, P, ptr, cols, vals, omega, l1=0.0, l2=0.0, G=None):
    """One pass over the rank on a copy of ``F``, float64: the recurrence of csrc/nmfmu_sparse_wccd.hip with the maintained
    residual ``t_e = v_e - c <F[i], P[j_e]>``, every owner row on its own -- one without entries too.  ``G``: the Gram matrix
    to use (None: ``P^T P``)."""
    F = np.array(F, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    G = P.T @ P if G is None else np.asarray(G, dtype=np.float64)
    c = 1.0 - omega
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        Pi = P[cols[a:b]]
        t = np.asarray(vals[a:b], dtype=np.float64) - c * (Pi @ F[i])
        for k in range(F.shape[1]):
            p = Pi[:, k]
            fn = minimiser(F[i, k], p @ p, t @ p, F[i] @ G[k], G[k, k], omega, l1, l2)
            t -= c * (fn - F[i, k]) * p
            F[i, k] = fn
    return F


# ---- the dense brute force -----------------------------------------------------------------------------------------------------
def dense(ptr, cols, vals, n_panel, omega):
    """(X, Wt) [rows, n_panel] of one side's work list: the target with its unstored entries as zeros, and the weights -- 1
    on a stored entry (a stored zero too), omega elsewhere."""
    rows = len(ptr) - 1
    X, Wt = np.zeros((rows, n_panel)), np.full((rows, n_panel), float(omega))
    own = np.repeat(np.arange(rows), np.diff(ptr))
    X[own, cols] = vals
    Wt[own, cols] = 1.0
    return X, Wt


def row_objective(f, P, x, wt, l1=0.0, l2=0.0):
    """1/2 sum_j wt_j (x_j - <f, P[j]>)^2 + l1 sum f + l2/2 |f|^2 over ALL panel rows j."""
    r = x - P @ f
    return 0.5 * float(wt @ (r * r)) + l1 * f.sum() + 0.5 * l2 * float(f @ f)


def brute_minimiser(f, k, P, x, wt, l1=0.0, l2=0.0):
    """argmin over f[k] of ``row_objective`` with the other coordinates fixed, from the weight matrix alone (the kernel's eps
    in the denominator and its floor applied)."""
    p = P[:, k]
    rest = x - P @ f + f[k] * p
    return max(EPS, (float((wt * p) @ rest) - l1) / (float((wt * p) @ p) + l2 + EPS))


# ---- the whole procedure ---------------------------------------------------------------------------------------------------
def divergence(idx, vals, W, H, omega):
    """The weighted loss ``fit`` tracks, by the identity: 1/2 sum_stored [(v - y)^2 - omega y^2] + 1/2 omega <H^T H, W^T W>."""
    s = scores(idx, W, H)
    d = np.asarray(vals, dtype=np.float64) - s
    return 0.5 * float(d @ d - omega * (s @ s)) + 0.5 * omega * float(((H.T @ H) * (W.T @ W)).sum())


def dense_divergence(idx, vals, shape, W, H, omega):
    """The same loss as the dense weighted sum 1/2 sum_ij wt_ij (x_ij - y_ij)^2."""
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    X, Wt = np.zeros(shape), np.full(shape, float(omega))
    X[idx[0], idx[1]] = vals
    Wt[idx[0], idx[1]] = 1.0
    return 0.5 * float((Wt * (X - H @ W.T) ** 2).sum())


def objective(idx, vals, W, H, omega, l1=0.0, l2=0.0):
    """What the sweeps descend on: the divergence plus l1 (sum W + sum H) + l2 / 2 (|W|^2 + |H|^2)."""
    return divergence(idx, vals, W, H, omega) + l1 * (W.sum() + H.sum()) + 0.5 * l2 * ((W ** 2).sum() + (H ** 2).sum())


def init_scale(idx, vals, W, H, omega, train_W=True, train_H=True):
    """a = sum_e v_e s_e / (c sum_e s_e^2 + omega <H^T H, W^T W>), the scalar that minimises the weighted loss of a H W^T;
    both factors trainable -> each times sqrt(a); one -> that one times a; skipped unless a is finite and positive; the
    trainable factors clamped to >= eps afterwards."""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    s = scores(idx, W, H)
    den = (1.0 - omega) * float(s @ s) + omega * float(((H.T @ H) * (W.T @ W)).sum())
    a = float(np.asarray(vals, dtype=np.float64) @ s) / den if den != 0 else float('nan')
    if (train_W or train_H) and np.isfinite(a) and a > 0:
        if train_W and train_H:
            W, H = W * a ** 0.5, H * a ** 0.5
        elif train_W:
            W = W * a
        else:
            H = H * a
    if train_W:
        W = np.maximum(W, EPS)
    if train_H:
        H = np.maximum(H, EPS)
    return W, H


def fit(idx, vals, shape, W, H, omega, max_iter, tol=-1e300, l1=0.0, l2=0.0, train_W=True, train_H=True, trace=None,
        losses=None):
    """``NMF.fit(V, beta=2, tol, max_iter, solver='ccd', unstored=omega)`` in float64 -> (W, H, n_iter).  ``trace``: a list that
    receives the objective after the initial scaling and after every half-step; ``losses``: the divergence at the same
    points."""
    vals = np.asarray(vals, dtype=np.float64)
    lw, lh = side_list(idx, vals, shape, 'w'), side_list(idx, vals, shape, 'h')
    W, H = init_scale(idx, vals, W, H, omega, train_W, train_H)

    def note():
        if trace is not None:
            trace.append(objective(idx, vals, W, H, omega, l1, l2))
        if losses is not None:
            losses.append(divergence(idx, vals, W, H, omega))
    note()
    loss_init = previous = (2.0 * divergence(idx, vals, W, H, omega)) ** 0.5
    n_iter = -1
    for n_iter in range(max_iter):
        if train_W:
            W = sweep(W, H, *lw, omega, l1, l2)
            note()
        if train_H:
            H = sweep(H, W, *lh, omega, l1, l2)
            note()
        if n_iter % 10 == 9:
            loss = (2.0 * divergence(idx, vals, W, H, omega)) ** 0.5
            if (previous - loss) / loss_init < tol:
                break
            previous = loss
    return W, H, n_iter + 1


# ---- the kernel's own arithmetic in fp32 (a model, not bit-exact: fma is float32(float64 product + float64 addend)) ------------
_fma, _butterfly = CE._fma, CE._butterfly


def _fma1(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def gram_f32(P):
    """A symmetric fp32 Gram matrix of the panel, as ``nmfmu_gram`` hands one to the sweep (its own rounding is not the
    sweep's: the check takes G as an input)."""
    P = np.asarray(P, dtype=np.float64)
    G = (P.T @ P).astype(np.float32)
    return np.maximum(G, G.T)


def sweep_f32(F, P, ptr, cols, vals, omega, l1=0.0, l2=0.0, G=None, wg_rows=LIMIT):
    """The kernel's operations in its order with numpy float32 (the header of csrc/nmfmu_sparse_wccd.hip): c = 1.0f - omega;
    t_e = fma(-c, s_e, v_e); d and n as in ``ccd_emulation.sweep_f32``; q: lane l's chain over the coordinates l + 64 m,
    m = 0 .. 3, then the butterfly; D = fma(c, d, omega * G[k][k]); num = fma(f, D, fma(-omega, q, n)) - l1;
    den = (D + l2) + eps; t_e = fma(-(c * (f' - f)), p, t_e)."""
    F = np.array(F, dtype=np.float32)
    P = np.asarray(P, dtype=np.float32)
    G = gram_f32(P) if G is None else np.asarray(G, dtype=np.float32)
    omega, l1, l2, eps = np.float32(omega), np.float32(l1), np.float32(l2), np.float32(EPS)
    c = np.float32(np.float32(1.0) - omega)
    R = F.shape[1]
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        cnt = b - a
        NW = WG_WAVES if cnt > wg_rows else 1
        T = -(-cnt // (64 * NW))
        Pi = np.zeros((T * NW * 64, R), dtype=np.float32)
        Pi[:cnt] = P[cols[a:b]]
        v = np.zeros(T * NW * 64, dtype=np.float32)
        v[:cnt] = vals[a:b]
        s = np.zeros_like(v)
        for k in range(R):
            s = _fma(np.full_like(s, F[i, k]), Pi[:, k], s)
        t = _fma(np.full_like(s, -c), s, v)
        own = np.zeros(64 * Q_SLOTS, dtype=np.float32)       # coordinate j in lane j mod 64, slot j / 64
        own[:R] = F[i]
        for k in range(R):
            p = Pi[:, k].reshape(T, NW, 64)
            tt = t.reshape(T, NW, 64)
            d, n = np.zeros((NW, 64), dtype=np.float32), np.zeros((NW, 64), dtype=np.float32)
            for m in range(T):
                d = _fma(p[m], p[m], d)
                n = _fma(tt[m], p[m], n)
            dw, nw = [_butterfly(x) for x in d], [_butterfly(x) for x in n]
            d, n = dw[0], nw[0]
            for w in range(1, NW):
                d, n = np.float32(d + dw[w]), np.float32(n + nw[w])
            gk = np.zeros(64 * Q_SLOTS, dtype=np.float32)
            gk[:R] = G[k]
            q = np.zeros(64, dtype=np.float32)
            for m in range(Q_SLOTS):                          # (beyond the rank both operands are +0: the chain is unchanged)
                q = _fma(own[64 * m:64 * m + 64], gk[64 * m:64 * m + 64], q)
            q = _butterfly(q)
            f = F[i, k]
            D = _fma1(c, d, np.float32(omega * G[k, k]))
            num = np.float32(_fma1(f, D, _fma1(-omega, q, n)) - l1)
            den = np.float32(np.float32(D + l2) + eps)
            fn = np.maximum(eps, np.float32(num / den))
            back = np.float32(-np.float32(c * np.float32(fn - f)))
            t = _fma(np.full_like(t, back), Pi[:, k], t)
            F[i, k] = fn
            own[k] = fn
    return F


# ---- the per-element check of nmfmu_sp_wccd_sweep -----------------------------------------------------------------------------
def bound_terms(rank, k, count, wg_rows=LIMIT):
    """(c_res, S, S_q) of the running-error bound, counted on the kernel's operations (csrc/nmfmu_sparse_wccd.hip).  The
    premise, as for ``ccd_emulation.bound_terms``: owner, panel, values and G are >= 0.  c is taken as 1 - fp32(omega) exactly
    and the rounding of the kernel's c = 1.0f - omega (relative u) is charged wherever c is a factor.

    The residual the kernel holds when it updates coordinate k.  With M_e = v_e + c sum_j max(old_j, new_j) p_ej, which bounds
    |t_e| at every moment of the sweep and c sum_j |f'_j - f_j| p_ej (|f' - f| <= max(f', f) for non-negative values):
      * s_e is a chain of R fused multiply-adds: at most R roundings on a term; times c: <= R u M_e;
      * the rounding of c in c s_e: 1;   fma(-c, s_e, v_e): 1 rounding of a value <= M_e;
      * the earlier coordinates j < k: f'_j - f_j rounds once, c times it rounds once, c's own rounding: 3 roundings on
        c |delta_j| p_ej, which sum over j to <= M_e: 3;   the fused update rounds t_e once per coordinate: k;
      c_res = R + 1 + 1 + 3 + k, error of t_e <= c_res u M_e.
    The sums over the entries, n and d: with NW waves on the row (1, or WG_WAVES above ``wg_rows`` entries) a lane's chain
    over T = ceil(count / (64 NW)) slots, six butterfly additions and NW - 1 additions of the waves' totals:
      S = T + 6 + NW - 1 roundings on a term (a row without entries has no terms at all).
    q: a lane's chain of at most four fused multiply-adds and six butterfly additions: S_q = 10."""
    NW = WG_WAVES if count > wg_rows else 1
    T = -(-count // (64 * NW))
    return rank + 5 + k, T + 6 + NW - 1, Q_SLOTS + 6


def sweep_check(got, old, P, G, ptr, cols, vals, omega, l1=0.0, l2=0.0, wg_rows=LIMIT):
    """The coordinate fixed point, per element, from the device's OWN output: for every owner row (one without entries too) and
    every k, in float64, the state as it stood when coordinate k was updated (mix: coordinates < k new, >= k old),
        rho_e = v_e - c sum_j mix_j p_ej,   q = sum_j mix_j G[k][j],   want = minimiser(old[k], sum p^2, sum rho p, q, G[k][k])
    with omega, l1, l2 rounded to fp32 first (what the C entry receives) and ``G`` as the kernel read it (an input: its own
    rounding is ``nmfmu_gram``'s).  With A = sum_e |rho_e| p_ek, B = omega sum_j mix_j G[k][j], C = old[k] D, mag = A + B + C +
    l1 >= |num| and (c_res, S, S_q) of ``bound_terms``, the numerator's error is at most u times
        c_res sum_e M_e p_ek          the residuals in n
      + S A + S_q B                   the sums n and q
      + (S + 2) C                     D = fma(c, d, omega G_kk): d's sum (S), c's rounding, the product's, the fma's: <= (S + 2) u D
      + (A + B) + (A + B + C) + mag   the roundings of fma(-omega, q, n), fma(f, D, .) and the subtraction of l1
    and the denominator (D + l2) + eps carries D's (S + 2) u and two roundings of non-negative sums, which move the quotient by
    (S + 4) u mag / den; one more u mag / den covers the second-order terms ((1 + u)^c - 1 <= (c + 1) u for c u < 0.01):
        bound = u (c_res sum M p + (S + 3) A + (S_q + 3) B + (S + 4) C + l1 + (S + 5) mag) / den + 2 u |want|
    (2 u |want|: the division's own rounding and the fp32 representation of the result).  max(eps, .) is 1-Lipschitz, so the
    bound holds on either side of the clamp.  Returns (err, bound), both [rows, R] float64."""
    got, old = np.asarray(got, dtype=np.float64), np.asarray(old, dtype=np.float64)
    P, G = np.asarray(P, dtype=np.float64), np.asarray(G, dtype=np.float64)
    omega, l1, l2 = float(np.float32(omega)), float(np.float32(l1)), float(np.float32(l2))
    c = 1.0 - omega
    rows, R = got.shape
    err, bound = np.zeros((rows, R)), np.zeros((rows, R))
    for i in range(rows):
        a, b = ptr[i], ptr[i + 1]
        Pi = P[cols[a:b]]
        v = np.asarray(vals[a:b], dtype=np.float64)
        M = v + c * (Pi @ np.maximum(got[i], old[i]))
        mix = old[i].copy()
        rho = v - c * (Pi @ mix)              # float64 throughout: its own rounding is 2^-29 of fp32's
        for k in range(R):
            p = Pi[:, k]
            d = p @ p
            q = mix @ G[k]
            D = c * d + omega * G[k, k]
            den = D + l2 + EPS
            want = minimiser(old[i, k], d, rho @ p, q, G[k, k], omega, l1, l2)
            c_res, S, S_q = bound_terms(R, k, b - a, wg_rows)
            A, B, C = np.abs(rho) @ p, omega * (mix @ np.abs(G[k])), old[i, k] * D
            mag = A + B + C + l1
            err[i, k] = abs(got[i, k] - want)
            bound[i, k] = U * (c_res * (M @ p) + (S + 3) * A + (S_q + 3) * B + (S + 4) * C + l1 + (S + 5) * mag) / den \
                + 2 * U * abs(want)
            rho -= c * (got[i, k] - old[i, k]) * p
            mix[k] = got[i, k]
    return err, bound
