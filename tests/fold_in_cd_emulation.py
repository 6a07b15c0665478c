"""float64 numpy model of fold-in by coordinate descent (``fold_in_cd(solver='ccd' | 'hals')``, torchnmf_amd/fold_in.py,
csrc/nmfmu_fold_in_cd.hip), test-only: the iterated sweep with the per-row stop rule, an fp32 model of
the kernel's own operation order, a running-error bound counted on those operations, and the per-element check that
recomputes every coordinate's minimiser in float64 from the device's own new and old row.  No torch, no GPU.

Conventions: ``V_new (n, C) ~ H (n, R) @ W (C, R)^T`` with ``W`` fixed; the rows as a CSR work list ``(ptr, cols, vals)``
(``ccd_emulation.side_list(idx, vals, shape, 'h')``); the objective of a row has one parameter ``omega`` in [0, 1] -- 0:
'missing', 1: 'zero' (HALS on the row), between: the confidence of the unstored zeros; ``c = 1 - omega``; ``eps = 2^-23``.

What the kernel does, from its source: with NW waves on a row (1, or WAVES = 4 above ``long_rows`` entries) wave w owns
the entries [w per, (w + 1) per), per = ceil(count / NW); local entry i on lane i mod 64 as slot i / 64.  d_k, n (and, for
omega = 1, the constant n_k): per-lane fused multiply-add chains over the slots in ascending order, an xor butterfly
32 .. 1 per wave, the waves' totals added in wave order.  q: lane l's chain over the coordinates l + 64 m, m = 0 .. 3, then
the butterfly.  The residuals t_e = fma(-c, s_e, v_e) are formed anew from h at the start of every iteration (s_e a chain of
R fused multiply-adds, k ascending) and maintained inside it: t_e = fma(-(c * (h' - h)), p, t_e).  d_k and
D_k = fma(c, d_k, omega * G[k][k]) are formed once per row by the same chain every iteration would run.  A row whose share
exceeds the wave's LDS (``avail``) keeps no residuals and forms t_e from h as it stands for every coordinate: fewer
roundings on the same value, inside the same bound.
"""
import numpy as np

import ccd_emulation as CE
import fold_in_emulation as FE
import wccd_emulation as WE

EPS, U = CE.EPS, CE.U
WAVES = 4
Q_SLOTS = 4
PER_WAVE = ((10240 - 4 * WAVES) // WAVES) & ~3        # floats of LDS a wave owns: a workgroup has 40 KiB


def omega_of(mode):
    """'missing' -> 0, 'zero' -> 1, a number -> itself."""
    return {'missing': 0.0, 'zero': 1.0}.get(mode, mode) if isinstance(mode, str) else float(mode)


def avail(R: int) -> int:
    """csrc/nmfmu_fold_in_cd.hip: fcd_avail -- what a wave has for residuals and staged W rows."""
    return PER_WAVE - 3 * ((R + 63) & ~63)


def default_block(R: int) -> int:
    """fcd_block_cap: the largest share whose residuals and W rows fit the wave's LDS."""
    return (avail(R) - 3) // ((R | 1) + 1)


def default_long_rows(R: int) -> int:
    """nmfmu_fold_in_cd_long_rows: the count above which a row takes the workgroup by default."""
    return min(default_block(R), 128)


# ---- float64: the iterated sweep -----------------------------------------------------------------------------------------
def sweep(H, W, ptr, cols, vals, omega, l1=0.0, l2=0.0, G=None):
    """One iteration on every row: ``ccd_emulation.sweep`` for omega = 0 (a row without entries is returned as it came),
    ``wccd_emulation.sweep`` otherwise (every row is swept)."""
    if omega == 0:
        return CE.sweep(H, W, ptr, cols, vals, l1, l2)
    return WE.sweep(H, W, ptr, cols, vals, omega, l1, l2, G)


def states(H0, W, ptr, cols, vals, omega, k, l1=0.0, l2=0.0, G=None):
    """[H_0, .., H_k]: k iterations on every row, none stopped; float64.  No initial scaling: H0 as it is."""
    out = [np.asarray(H0, np.float64)]
    for _ in range(k):
        out.append(sweep(out[-1], W, ptr, cols, vals, omega, l1, l2, G))
    return out


def run(H0, W, ptr, cols, vals, omega, max_iter, tol=0.0, l1=0.0, l2=0.0, G=None):
    """(H, counts): every row at the state its own count names -- the first k >= 1 with
    max_r |h_k - h_(k-1)| <= tol * max_r h_k (``fold_in_emulation.stop_counts``: evaluated in fp32; an unchanged row stops
    at 1), max_iter where it never holds or tol == 0."""
    sts = states(H0, W, ptr, cols, vals, omega, max_iter, l1, l2, G)
    cnt = FE.stop_counts(sts, tol)
    H = np.stack([sts[int(c)][i] for i, c in enumerate(cnt)]) if len(cnt) else sts[0]
    return H, cnt


def objectives(H, W, ptr, cols, vals, omega, l1=0.0, l2=0.0):
    """Per row, ``wccd_emulation.row_objective`` on the explicit weight matrix (1 on a stored entry, omega elsewhere)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    X, Wt = WE.dense(ptr, cols, vals, W.shape[0], omega)
    return np.array([WE.row_objective(H[i], W, X[i], Wt[i], l1, l2) for i in range(H.shape[0])])


# ---- the kernel's own arithmetic in fp32 (a model, not bit-exact: fma is float32(float64 product + float64 addend)) ------------
_fma, _fma1, _butterfly = CE._fma, WE._fma1, CE._butterfly


def _row_sum(x, p, NW, T):
    """sum_e x_e p_e in the kernel's order: [NW, T, 64] operands, a chain over the slots per lane, the butterfly per wave,
    the waves' totals in wave order."""
    acc = np.zeros((NW, 64), dtype=np.float32)
    for t in range(T):
        acc = _fma(x[:, t], p[:, t], acc)
    tot = [_butterfly(a) for a in acc]
    out = tot[0]
    for w in range(1, NW):
        out = np.float32(out + tot[w])
    return out


def sweep_f32(H, W, ptr, cols, vals, omega, l1=0.0, l2=0.0, G=None, long_rows=None):
    """One iteration in the kernel's operation order with numpy float32 (see the module docstring and the header of
    csrc/nmfmu_fold_in_cd.hip); the rows whose residuals live in LDS.  ``G``: the fp32 Gram matrix as the kernel reads it
    (None: ``wccd_emulation.gram_f32``; not read for omega = 0)."""
    H = np.array(H, dtype=np.float32)
    W = np.asarray(W, dtype=np.float32)
    R = H.shape[1]
    long_rows = default_long_rows(R) if long_rows is None else long_rows
    if omega == 0:
        G = np.zeros((R, R), dtype=np.float32)
    else:
        G = WE.gram_f32(W) if G is None else np.asarray(G, dtype=np.float32)
    omega, l1, l2, eps = np.float32(omega), np.float32(l1), np.float32(l2), np.float32(EPS)
    c = np.float32(np.float32(1.0) - omega)
    for i in range(H.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        cnt = b - a
        if cnt == 0 and omega == 0:
            continue
        NW = WAVES if cnt > long_rows else 1
        per = -(-cnt // NW)
        T = -(-per // 64)
        Pi = np.zeros((NW, T * 64, R), dtype=np.float32)
        v = np.zeros((NW, T * 64), dtype=np.float32)
        for w in range(NW):
            lo, hi = min(cnt, w * per), min(cnt, (w + 1) * per)
            Pi[w, :hi - lo] = W[cols[a + lo:a + hi]]
            v[w, :hi - lo] = vals[a + lo:a + hi]
        Pi = Pi.reshape(NW, T, 64, R)
        v = v.reshape(NW, T, 64)
        s = np.zeros_like(v)
        for k in range(R):
            s = _fma(np.full_like(s, H[i, k]), Pi[..., k], s)
        t = _fma(np.full_like(s, -c), s, v)
        own = np.zeros(64 * Q_SLOTS, dtype=np.float32)       # coordinate j in lane j mod 64, slot j / 64
        own[:R] = H[i]
        for k in range(R):
            p = Pi[..., k]
            d = _row_sum(p, p, NW, T)
            n = _row_sum(t, p, NW, T)
            f = H[i, k]
            if omega == 0:
                D = d
                num = np.float32(_fma1(f, D, n) - l1)
            else:
                gk = np.zeros(64 * Q_SLOTS, dtype=np.float32)
                gk[:R] = G[k]
                q = np.zeros(64, dtype=np.float32)
                for m in range(Q_SLOTS):                      # (beyond the rank both operands are +0: the chain is unchanged)
                    q = _fma(own[64 * m:64 * m + 64], gk[64 * m:64 * m + 64], q)
                q = _butterfly(q)
                D = _fma1(c, d, np.float32(omega * G[k, k]))
                num = np.float32(_fma1(f, D, _fma1(-omega, q, n)) - l1)
            den = np.float32(np.float32(D + l2) + eps)
            fn = np.maximum(eps, np.float32(num / den))
            back = np.float32(-np.float32(c * np.float32(fn - f)))
            t = _fma(np.full_like(t, back), p, t)
            H[i, k] = fn
            own[k] = fn
    return H


# ---- the per-element check of one iteration of nmfmu_fold_in_cd ---------------------------------------------------------------
def bound_terms(rank, k, count, long_rows):
    """(c_res, S, S_q) of the running-error bound, counted on the kernel's operations exactly as
    ``wccd_emulation.bound_terms`` counts them for the sweep kernel (the recurrence is the same; the premise too: H, W, values
    and G are >= 0), with this kernel's work split:
      c_res = R + 5 + k   the residual t_e when coordinate k is updated: the chain s_e (R), the rounding of c in c s_e (1),
                          fma(-c, s_e, v_e) (1), the earlier coordinates' c (h' - h) (3 for all together) and one fused update
                          per earlier coordinate (k) -- each a rounding of a value <= M_e.  A row that keeps no residuals forms
                          t_e with R + 2 of them.
      S = T + 6 + NW - 1  a sum over the entries (d_k, n, the constant n_k): a lane's chain over T = ceil(per / 64) slots,
                          per = ceil(count / NW), six butterfly additions, NW - 1 additions of the waves' totals.  Forming d_k
                          once per row runs the same chain: the count does not change.
      S_q = 4 + 6         q: a lane's chain of at most four fused multiply-adds, six butterfly additions."""
    NW = WAVES if count > long_rows else 1
    per = -(-count // NW)
    T = -(-per // 64)
    return rank + 5 + k, T + 6 + NW - 1, Q_SLOTS + 6


def sweep_check(got, old, W, G, ptr, cols, vals, omega, l1=0.0, l2=0.0, long_rows=None):
    """One iteration, per element, from the device's OWN output: for every row and every k, in float64, the state as it stood
    when coordinate k was updated (mix: coordinates < k from ``got``, >= k from ``old``),
        rho_e = v_e - c sum_j mix_j p_ej,   q = sum_j mix_j G[k][j],   want = minimiser(old[k], sum p^2, sum rho p, q, G[k][k])
    (``wccd_emulation.minimiser``; omega, l1, l2 rounded to fp32 first; ``G`` as the kernel read it, None for omega = 0), and
    the bound of ``wccd_emulation.sweep_check`` with ``bound_terms`` of this kernel:
        bound = u (c_res sum M p + (S + 3) A + (S_q + 3) B + (S + 4) C + l1 + (S + 5) mag) / den + 2 u |want|
    with M_e = v_e + c sum_j max(old_j, got_j) p_ej, A = sum_e |rho_e| p_ek, B = omega sum_j mix_j |G[k][j]|, C = old[k] D,
    mag = A + B + C + l1 -- derived there; it holds at the end points too (omega = 0: B = 0, D = d, and c is exact; omega = 1:
    c = 0, the residual is the value itself and n its constant sum).  A row without entries under omega = 0 must come back
    as it went: err = |got - old|, bound = 0.  Returns (err, bound), both [rows, R] float64."""
    got, old = np.asarray(got, dtype=np.float64), np.asarray(old, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    rows, R = got.shape
    long_rows = default_long_rows(R) if long_rows is None else long_rows
    omega, l1, l2 = float(np.float32(omega)), float(np.float32(l1)), float(np.float32(l2))
    G = np.zeros((R, R)) if omega == 0 else np.asarray(G, dtype=np.float64)
    c = 1.0 - omega
    err, bound = np.zeros((rows, R)), np.zeros((rows, R))
    for i in range(rows):
        a, b = ptr[i], ptr[i + 1]
        if b == a and omega == 0:
            err[i] = np.abs(got[i] - old[i])
            continue
        Pi = W[cols[a:b]]
        v = np.asarray(vals[a:b], dtype=np.float64)
        M = v + c * (Pi @ np.maximum(got[i], old[i]))
        mix = old[i].copy()
        rho = v - c * (Pi @ mix)
        for k in range(R):
            p = Pi[:, k]
            d = p @ p
            q = mix @ G[k]
            D = c * d + omega * G[k, k]
            den = D + l2 + EPS
            want = WE.minimiser(old[i, k], d, rho @ p, q, G[k, k], omega, l1, l2)
            c_res, S, S_q = bound_terms(R, k, b - a, long_rows)
            A, B, C = np.abs(rho) @ p, omega * (mix @ np.abs(G[k])), old[i, k] * D
            mag = A + B + C + l1
            err[i, k] = abs(got[i, k] - want)
            bound[i, k] = U * (c_res * (M @ p) + (S + 3) * A + (S_q + 3) * B + (S + 4) * C + l1 + (S + 5) * mag) / den \
                + 2 * U * abs(want)
            rho -= c * (got[i, k] - old[i, k]) * p
            mix[k] = got[i, k]
    return err, bound


fraction = CE.fraction


def work_list(idx, vals, shape):
    """The CSR work list of the new rows from COO entries."""
    return CE.side_list(idx, vals, shape, 'h')
