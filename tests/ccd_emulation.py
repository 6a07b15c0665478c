"""float64 numpy model of ``NMF.fit(solver='ccd', unstored='missing')`` (torchnmf_amd/ccd.py, csrc/nmfmu_sparse_ccd.hip), an
fp32 model of the kernel's own arithmetic, and the per-element check of the sweep kernel.  No torch, no GPU: the CPU tests
exercise it on its own, the GPU tests compare the device against it.

Conventions as in the package: ``V (N, C) ~ H (N, R) @ W (C, R)^T`` over the STORED entries only; an iteration is the W
half-step, then the H half-step with the new W; ``eps = 2^-23``.  A side's work list is ``(ptr, cols, vals)``: owner row
``i`` stores the entries ``ptr[i] .. ptr[i + 1]`` with panel rows ``cols`` and values ``vals`` (CSR for H, CSC for W).
"""
import numpy as np

EPS = 2.0 ** -23
U = 2.0 ** -24          # unit roundoff of fp32
LIMIT = 512             # ccd.RESIDENT_LIMIT: residuals per wave in registers, and the default workgroup threshold
WG_WAVES = 16           # ccd.WG_WAVES
FULL_ITERS = 10         # iterations of the fully stored comparison with solver='hals'


def side_list(idx, vals, shape, side):
    """(ptr, cols, vals) of one side from COO entries ``idx [2, nnz]`` (any order): 'h' -- owner rows are rows of V, 'w' --
    columns of V.  Entries of an owner row are sorted by panel row, as the package's CSR / CSC arrays are."""
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    own, oth = (idx[0], idx[1]) if side == 'h' else (idx[1], idx[0])
    n = shape[0] if side == 'h' else shape[1]
    o = np.lexsort((oth, own))
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(own, minlength=n))
    return ptr, oth[o], np.asarray(vals)[o]


def minimiser(f, d, n, l1, l2):
    return np.maximum(EPS, (n + f * d - l1) / (d + l2 + EPS))


def sweep(F, P, ptr, cols, vals, l1=0.0, l2=0.0):
    """One pass over the rank on a copy of ``F``, float64: the recurrence of csrc/nmfmu_sparse_ccd.hip with the maintained
    residual, every owner row on its own; a row without entries is returned as it came."""
    F = np.array(F, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        if b == a:
            continue
        Pi = P[cols[a:b]]
        r = np.asarray(vals[a:b], dtype=np.float64) - Pi @ F[i]
        for k in range(F.shape[1]):
            p = Pi[:, k]
            fn = minimiser(F[i, k], p @ p, r @ p, l1, l2)
            r -= (fn - F[i, k]) * p
            F[i, k] = fn
    return F


def gram_sweep(F, P, ptr, cols, vals, l1=0.0, l2=0.0):
    """The same pass written as Gauss-Seidel on the row's own normal equations: ``G_i = P_i^T P_i`` and ``A_i = v_i P_i`` over
    the row's stored entries, ``f_k = max(eps, (A_i[k] - l1 - sum_{j != k} f_j G_i[j, k]) / (G_i[k, k] + l2 + eps))``."""
    F = np.array(F, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        if b == a:
            continue
        Pi = P[cols[a:b]]
        G, A = Pi.T @ Pi, np.asarray(vals[a:b], dtype=np.float64) @ Pi
        for k in range(F.shape[1]):
            s = F[i] @ G[:, k] - F[i, k] * G[k, k]
            F[i, k] = max(EPS, (A[k] - l1 - s) / (G[k, k] + l2 + EPS))
    return F


# ---- the kernel's own arithmetic in fp32 (a model, not bit-exact: fma is float32(float64 product + float64 addend)) ------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _butterfly(x):
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[lanes ^ o]).astype(np.float32)
    return x[0]


def sweep_f32(F, P, ptr, cols, vals, l1=0.0, l2=0.0, wg_rows=LIMIT):
    """The kernel's operations in its order with numpy float32.  NW = 1 waves on a row of at most ``wg_rows`` entries,
    WG_WAVES on a longer one: entry e on lane e mod 64 of wave (e / 64) mod NW, per-lane chains over the slots, xor butterfly
    32 .. 1 per wave, the waves' totals added in wave order, ``fma(f, d, n) - l1`` over ``(d + l2) + eps``."""
    F = np.array(F, dtype=np.float32)
    P = np.asarray(P, dtype=np.float32)
    l1, l2, eps = np.float32(l1), np.float32(l2), np.float32(EPS)
    R = F.shape[1]
    for i in range(F.shape[0]):
        a, b = ptr[i], ptr[i + 1]
        cnt = b - a
        if cnt == 0:
            continue
        NW = WG_WAVES if cnt > wg_rows else 1
        T = -(-cnt // (64 * NW))
        Pi = np.zeros((T * NW * 64, R), dtype=np.float32)
        Pi[:cnt] = P[cols[a:b]]
        v = np.zeros(T * NW * 64, dtype=np.float32)
        v[:cnt] = vals[a:b]
        s = np.zeros_like(v)
        for k in range(R):
            s = _fma(np.full_like(s, F[i, k]), Pi[:, k], s)
        r = (v - s).astype(np.float32)
        for k in range(R):
            p = Pi[:, k].reshape(T, NW, 64)
            rr = r.reshape(T, NW, 64)
            d, n = np.zeros((NW, 64), dtype=np.float32), np.zeros((NW, 64), dtype=np.float32)
            for t in range(T):
                d = _fma(p[t], p[t], d)
                n = _fma(rr[t], p[t], n)
            dw, nw = [_butterfly(x) for x in d], [_butterfly(x) for x in n]
            d, n = dw[0], nw[0]
            for w in range(1, NW):
                d, n = np.float32(d + dw[w]), np.float32(n + nw[w])
            f = F[i, k]
            num = np.float32(np.float32(np.float64(f) * np.float64(d) + np.float64(n)) - l1)
            den = np.float32(np.float32(d + l2) + eps)
            fn = np.maximum(eps, np.float32(num / den))
            back = np.float32(-(fn - f))
            r = _fma(np.full_like(r, back), Pi[:, k], r)
            F[i, k] = fn
    return F


# ---- the whole procedure ---------------------------------------------------------------------------------------------------
def scores(idx, W, H):
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    return np.einsum('pr,pr->p', H[idx[0]], W[idx[1]])


def divergence(idx, vals, W, H):
    """1/2 sum over the stored entries of (v - <H[i], W[j]>)^2: the loss ``fit`` tracks (no regularisation terms)."""
    d = np.asarray(vals, dtype=np.float64) - scores(idx, W, H)
    return 0.5 * float(d @ d)


def objective(idx, vals, W, H, l1=0.0, l2=0.0):
    """What the sweeps descend on: the divergence plus l1 (sum W + sum H) + l2 / 2 (|W|^2 + |H|^2)."""
    return divergence(idx, vals, W, H) + l1 * (W.sum() + H.sum()) + 0.5 * l2 * ((W ** 2).sum() + (H ** 2).sum())


def init_scale(idx, vals, W, H, train_W=True, train_H=True):
    """a = sum_e v_e s_e / sum_e s_e^2 over the stored entries; both factors trainable -> each times sqrt(a); one -> that one
    times a; skipped unless a is finite and positive; the trainable factors clamped to >= eps afterwards."""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    s = scores(idx, W, H)
    ss = float(s @ s)
    a = float(np.asarray(vals, dtype=np.float64) @ s) / ss if ss != 0 else float('nan')
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


def fit(idx, vals, shape, W, H, max_iter, tol=-1e300, l1=0.0, l2=0.0, train_W=True, train_H=True, trace=None, losses=None):
    """``NMF.fit(V, beta=2, tol, max_iter, solver='ccd', unstored='missing')`` in float64 -> (W, H, n_iter).  ``trace``: a
    list that receives the objective after the initial scaling and after every half-step; ``losses``: the divergence at the
    same points."""
    vals = np.asarray(vals, dtype=np.float64)
    lw, lh = side_list(idx, vals, shape, 'w'), side_list(idx, vals, shape, 'h')
    W, H = init_scale(idx, vals, W, H, train_W, train_H)

    def note():
        if trace is not None:
            trace.append(objective(idx, vals, W, H, l1, l2))
        if losses is not None:
            losses.append(divergence(idx, vals, W, H))
    note()
    loss_init = previous = (2.0 * divergence(idx, vals, W, H)) ** 0.5
    n_iter = -1
    for n_iter in range(max_iter):
        if train_W:
            W = sweep(W, H, *lw, l1, l2)
            note()
        if train_H:
            H = sweep(H, W, *lh, l1, l2)
            note()
        if n_iter % 10 == 9:
            loss = (2.0 * divergence(idx, vals, W, H)) ** 0.5
            if (previous - loss) / loss_init < tol:
                break
            previous = loss
    return W, H, n_iter + 1


def masked_mu_fit(idx, vals, shape, W, H, n_iter):
    """float64 masked multiplicative update for beta = 2 (``masked_emulation.step``), from the factors as given."""
    import masked_emulation as M
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    for _ in range(n_iter):
        W = M.step(idx, vals, shape, H, W, 2.0, 'w')[0]
        H = M.step(idx, vals, shape, H, W, 2.0, 'h')[0]
    return W, H


# ---- the per-element check of nmfmu_sp_ccd_sweep ------------------------------------------------------------------------------
def bound_terms(rank, k, count, wg_rows=LIMIT):
    """(c_res, c_sum) of the running-error bound, counted on the kernel's operations (csrc/nmfmu_sparse_ccd.hip).

    The residual the kernel holds when it updates coordinate k.  With M_e = v_e + sum_j max(old_j, new_j) p_ej, which bounds
    |r_e| at every moment of the sweep (all terms are >= 0) and every |f'_j - f_j| p_ej:
      * s_e is a chain of R fused multiply-adds: at most R roundings on a term, error <= R u sum_j old_j p_ej <= R u M_e;
      * v_e - s_e: 1 rounding of a value <= M_e;
      * each earlier coordinate j < k: f'_j - f_j rounds once (times p_ej: <= u M_e in r_e; counted once for all j together
        it would be sum_j |delta_j| p_ej <= 2 M_e: 2), and the fused update rounds r_e once: k roundings of values <= M_e.
      c_res = R + 1 + 2 + k, error of r_e <= c_res u M_e, so n is off by at most c_res u sum_e M_e p_ek before its own sum.
    The sums.  With NW waves on the row (1, or WG_WAVES above ``wg_rows`` entries) a lane's chain over T = ceil(count / (64
    NW)) slots, six butterfly additions and NW - 1 additions of the waves' totals put at most S = T + 6 + NW - 1 roundings
    on a term: n is within S u sum_e |r_e| p_ek, d within S u d.  d enters the quotient three times -- in f d of the
    numerator, and in the denominator, whose relative error moves the quotient by that fraction of |num| / den: with
    mag = sum_e |r_e| p_ek + f_k d + l1 >= |num| that is 3 S u mag / den for the three sums.  fma(f, d, n) and the
    subtraction of l1 round once each: 2; (d + l2) + eps rounds twice, non-negative terms: 2; one more covers the
    second-order terms ((1 + u)^c - 1 <= (c + 1) u for c u < 0.01).
      c_sum = 3 S + 2 + 2 + 1."""
    NW = WG_WAVES if count > wg_rows else 1
    T = -(-count // (64 * NW))
    return rank + 3 + k, 3 * (T + 6 + NW - 1) + 5


def sweep_check(got, old, P, ptr, cols, vals, l1=0.0, l2=0.0, wg_rows=LIMIT):
    """The coordinate fixed point, per element, from the device's OWN output: for every owner row with entries and every k, in
    float64, the residual as it stood when coordinate k was updated (coordinates < k new, >= k old),
        rho_e = v_e - sum_{j<k} got[j] p_ej - sum_{j>=k} old[j] p_ej,    want = minimiser(old[k], sum p^2, sum rho p)
    with l1, l2 rounded to fp32 first (what the C entry receives), and
        bound = u (c_res sum_e M_e p_ek + c_sum mag) / den + 2 u |want|
    (``bound_terms``; 2 u |want|: the division's own rounding and the fp32 representation of the result).  max(eps, .) is
    1-Lipschitz, so the bound holds on either side of the clamp.  Rows without entries: err = |got - old|, bound = 0.
    Returns (err, bound), both [rows, R] float64."""
    got, old = np.asarray(got, dtype=np.float64), np.asarray(old, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    l1, l2 = float(np.float32(l1)), float(np.float32(l2))
    rows, R = got.shape
    err, bound = np.zeros((rows, R)), np.zeros((rows, R))
    for i in range(rows):
        a, b = ptr[i], ptr[i + 1]
        if b == a:
            err[i] = np.abs(got[i] - old[i])
            continue
        Pi = P[cols[a:b]]
        v = np.asarray(vals[a:b], dtype=np.float64)
        M = v + Pi @ np.maximum(got[i], old[i])
        rho = v - Pi @ old[i]             # float64 throughout: its own rounding is 2^-29 of fp32's
        for k in range(R):
            p = Pi[:, k]
            d = p @ p
            den = d + l2 + EPS
            want = minimiser(old[i, k], d, rho @ p, l1, l2)
            c_res, c_sum = bound_terms(R, k, b - a, wg_rows)
            mag = np.abs(rho) @ p + old[i, k] * d + l1
            err[i, k] = abs(got[i, k] - want)
            bound[i, k] = U * (c_res * (M @ p) + c_sum * mag) / den + 2 * U * abs(want)
            rho -= (got[i, k] - old[i, k]) * p
    return err, bound


def fraction(err, bound):
    """Per element err / bound; where the bound is 0 (an untouched row) any difference is inf."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


ZERO_ROW_SCALE = 2.0 ** -10


def sweep_case(counts, n_panel, rank, seed=0):
    """Inputs of the sweep test, fp32: (F [rows, rank], P [n_panel, rank], ptr, cols, vals) with ``counts[i]`` stored entries
    in owner row i, panel rows drawn without repeats and sorted.  P > 0 with one all-floor column (not at rank 1).  The
    values are a noisy product of a factor with 30 % zeros, so that some coordinates clamp and others do not; every fifth
    value is a stored zero.  The row ``zero_row(counts)`` (if any) stores zeros only: its exact
    minimiser is the floor in every coordinate.  The maintained residual of that row carries the rounding of every update
    before it (about u R |r| each), while what keeps the last coordinate's numerator negative is only the floor's own share
    eps sum_j p_ej = 2 u sum_j p_ej of the residual: the row therefore starts from ZERO_ROW_SCALE times a normal start,
    which puts the accumulated rounding (<= u (R + 3 + k) M_e, M_e <= 2^-10 R) two orders below that share at rank 256.
    (``sweep_f32`` ends on the floor from an unscaled start too on the cases of the tests, but nothing guarantees it: the
    worst-case rounding of a residual near R exceeds the floor's share from rank 33 on.)"""
    counts = np.asarray(counts, dtype=np.int64)
    rows = len(counts)
    assert counts.max(initial=0) <= n_panel
    rng = np.random.default_rng(seed + 1000 * rows + 7 * rank + n_panel)
    P = np.abs(rng.standard_normal((n_panel, rank))) + 0.05
    if rank > 1:
        P[:, rank // 2] = EPS
    ptr = np.zeros(rows + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(counts)
    cols = np.concatenate([np.sort(rng.choice(n_panel, size=c, replace=False)) for c in counts] + [np.zeros(0, dtype=np.int64)])
    F_true = np.abs(rng.standard_normal((rows, rank))) * (rng.random((rows, rank)) < 0.7)
    own = np.repeat(np.arange(rows), counts)
    vals = np.einsum('pr,pr->p', F_true[own], P[cols]) * (0.5 + rng.random(len(cols)))
    vals[::5] = 0.0
    F = np.maximum(np.abs(rng.standard_normal((rows, rank))) * 0.3, EPS)
    z = zero_row(counts)
    if z is not None:
        vals[ptr[z]:ptr[z + 1]] = 0.0
        F[z] *= ZERO_ROW_SCALE
    return F.astype(np.float32), P.astype(np.float32), ptr, cols.astype(np.int64), vals.astype(np.float32)


def zero_row(counts):
    """The all-zero row of ``sweep_case``: the first row with >= 2 entries, when another row has entries too."""
    counts = np.asarray(counts)
    big = np.nonzero(counts >= 2)[0]
    return int(big[0]) if len(big) and (counts > 0).sum() >= 2 else None


def fit_case(name):
    """The problems of the fit tests: (idx [2, nnz] sorted by (row, col), vals, shape, W0, H0), values exactly representable
    in fp32, about 20 % of the entries stored.  'small': 40 x 30 at rank 4; 'mid': 300 x 200 at rank 33 (column 5 and row 7
    store nothing)."""
    n, c, r, seed = {'small': (40, 30, 4, 11), 'mid': (300, 200, 33, 13)}[name]
    rng = np.random.default_rng(seed)
    Wt, Ht = np.abs(rng.standard_normal((c, r))), np.abs(rng.standard_normal((n, r)))
    mask = rng.random((n, c)) < 0.2
    if name == 'mid':
        mask[:, 5] = False
        mask[7, :] = False
    V = (Ht @ Wt.T) * (0.8 + 0.4 * rng.random((n, c)))
    idx = np.stack(np.nonzero(mask)).astype(np.int64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return idx, f32(V[mask]), (n, c), f32(np.abs(rng.standard_normal((c, r)))), f32(np.abs(rng.standard_normal((n, r))))


def full_case():
    """A fully stored target (every entry of a 60 x 45 matrix, rank 6) as (idx, vals, shape, V, W0, H0)."""
    rng = np.random.default_rng(5)
    n, c, r = 60, 45, 6
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    V = f32(rng.random((n, c)) + 0.05)
    idx = np.stack(np.nonzero(np.ones((n, c), dtype=bool))).astype(np.int64)
    return idx, V.reshape(-1), (n, c), V, f32(np.abs(rng.standard_normal((c, r)))), f32(np.abs(rng.standard_normal((n, r))))
