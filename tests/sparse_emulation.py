"""Float64 reference of the sparse-COO MU path (csrc/nmfmu_sparse.hip, torchnmf_amd/sparse_engine.py), test-only.

Written from the kernels and from oracle/mu_oracle.py (``sp_*``).  Nothing on the beta in {1, 2} path is rounded to 16 bits,
so there is no rounding to reproduce and no ambiguous element: what separates a kernel from this module is fp32 arithmetic
alone, and every element is held to the bound the standard model of floating-point arithmetic gives for the operations the
kernel performs on it (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3-4: a sum of n terms formed in ANY
order, every term passing through at most k roundings, is within k u sum |terms| of the exact one to first order;
u = 2^-24).  Such a bound cannot tell one summation order from another; fixed-order accumulation is the determinism tests'
claim, not this module's.

The bounds, derived from the kernel sources (``ops_*`` below):

* ``sp_partial_kernel<RL, KIND>``: s = <owner[row], panel[col]> -- every product a[q] b[q] is one multiply, joins its
  lane's partial through at most RL additions and the wave's through six butterfly additions: 1 + RL + 6 roundings, all
  terms non-negative, so s is relative (RL + 7) u.  ``+ eps``: one more (both addends >= 0).  beta == 1: an IEEE divide
  (one rounding; the library is built without fast-math).  beta == 2: g = v, exact.  Otherwise g = v exp2f(c log2f(se)),
  c = beta - 2: log2f and exp2f are 1 ulp = 2 u functions; a relative error e of se moves log2 by e / ln 2, the product
  c * L adds one rounding, and an absolute error d of the exponent moves exp2 by d ln 2 relative; the multiply by v adds
  one.  Then every term g b is one multiply and joins acc through at most ``count`` additions (storage order).
* ``gram_partial_kernel`` / ``gram_final_kernel``: one multiply, at most ceil(per / 4) + 1 additions into one of four
  accumulators (the remainder loop feeds s0), two to combine them, 64 chunk partials added in order.
* ``rowmat_kernel``: one multiply and at most ``rank`` additions on top of the Gram matrix it reads.
* ``sp_loss_kernel``: s as above (its dot product has the same RL + 7 roundings), logf / exp2f / log2f at 2 u, the
  multiply by v, for the generic branch the divide by (beta - 1); the sum itself runs in float64.
* the generic positive term of the loss (the fused kernel's loss mode without a target): S accumulated by MFMAs in fp32
  over the padded rank's operand products (3 planes' worth in split bf16), v_log / v_exp at 2 u amplified by
  beta |log2 S| ln 2, one multiply by S, the scaling, then fp32 sums of 128 x 64 x tiles elements per workgroup.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import mu_emulation as E

EPS = E.EPS
U = 2.0 ** -24          # unit roundoff of fp32
ULP_FN = 2.0            # roundings' worth of a 1-ulp library function (exp2f, log2f, logf; v_exp_f32, v_log_f32)
LN2 = math.log(2.0)
GRAM_CHUNKS = 64        # kGramChunks


def rank_slots(r_pad: int) -> int:
    """RL of sp_partial_kernel / sp_loss_kernel (nmfmu_sp_partial's dispatch)."""
    return 1 if r_pad <= 64 else (2 if r_pad == 128 else 4)


# ---- the host's CSR ---------------------------------------------------------------------------------------------------
def coalesce(idx, vals, shape):
    """torch's coalesce: duplicates summed, entries in (row, col) order, explicit zeros kept.  (The sum is formed in
    float64; the cases keep duplicate values on a 2^-10 grid, so that it is exact in fp32 in any order.)"""
    idx = np.asarray(idx, dtype=np.int64).reshape(2, -1)
    vals = np.asarray(vals, dtype=np.float64)
    key = idx[0] * shape[1] + idx[1]
    uniq, inv = np.unique(key, return_inverse=True)
    out = np.zeros(len(uniq), dtype=np.float64)
    np.add.at(out, inv, vals)
    return np.stack([uniq // shape[1], uniq % shape[1]]), out.astype(np.float32)


def csr(rows, cols, vals, n_rows: int):
    """(rowptr int32, colidx int32, vals fp32) sorted by (row, col): the mirror of either half of sparse_autograd.csr_csc."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float32)
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n_rows))
    return rowptr.astype(np.int32), cols[order].astype(np.int32), vals[order]


def row_of_entry(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr.astype(np.int64)))


# ---- numerator ----------------------------------------------------------------------------------------------------------
def ops_g(se, beta: float, RL: int):
    """Roundings behind g for entries with reconstruction se = s + eps (see the module docstring)."""
    se = np.asarray(se, dtype=np.float64)
    kind = E.beta_kind(beta)
    s_ops = RL + 7 + 1                           # the dot product, + eps
    if kind == 'euc':
        return np.zeros_like(se)
    if kind == 'kl':
        return np.full_like(se, s_ops + 1)       # the divide
    c = abs(float(np.float32(beta)) - 2.0)
    expo = c * np.abs(np.log2(se)) * (ULP_FN + 1) + c * s_ops / LN2      # absolute error of c * log2f(se), in u
    return expo * LN2 + ULP_FN + 1               # through exp2f, exp2f's own ulp, the multiply by v


def numerator(csr_, owner, panel, beta: float, rows=None, eps=EPS):
    """Per owner row, in storage order.  Returns a dict: num, abs_sum (sum |g panel[col, r]|), count (entries per row),
    g_ops (per row, the largest ``ops_g`` of its entries), s and g per entry -- all restricted to ``rows`` if given.
    ``eps``: the seeded-fault tests pass 0."""
    rowptr, colidx, vals = csr_
    owner = np.asarray(owner, dtype=np.float64)
    panel = np.asarray(panel, dtype=np.float64)
    R = panel.shape[1]
    sel = np.arange(len(rowptr) - 1) if rows is None else np.asarray(rows)
    p0, p1 = rowptr[sel].astype(np.int64), rowptr[sel + 1].astype(np.int64)
    count = p1 - p0
    ent = np.concatenate([np.arange(a, b) for a, b in zip(p0, p1)]) if len(sel) else np.zeros(0, np.int64)
    ent = ent.astype(np.int64)
    local = np.repeat(np.arange(len(sel)), count)
    col = colidx[ent].astype(np.int64)
    v = vals[ent].astype(np.float64)
    b = panel[col]
    kind = E.beta_kind(beta)
    s = np.einsum('pr,pr->p', owner[sel][local], b) if len(ent) else np.zeros(0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if kind == 'kl':
            g = v / (s + eps)
        elif kind == 'euc':
            g = v.copy()
        else:
            g = v * np.power(s + eps, float(np.float32(beta)) - 2.0)
        contrib = g[:, None] * b
    num = np.zeros((len(sel), R))
    abs_sum = np.zeros((len(sel), R))
    np.add.at(num, local, contrib)
    np.add.at(abs_sum, local, np.abs(contrib))
    g_ops = np.zeros(len(sel))
    if len(ent):
        np.maximum.at(g_ops, local, ops_g(s + EPS, beta, rank_slots(E.pad_rank(R))))
    return dict(num=num, abs_sum=abs_sum, count=count, g_ops=g_ops, s=s, g=g, local=local)


def numerator_bound(em):
    """|got - ref| <= k u abs_sum, k = (entries of the row: the additions into acc) + 1 (the multiply g b) + g_ops."""
    return ((em['count'] + 1 + em['g_ops']) * U)[:, None] * em['abs_sum']


def bound_err(got, ref, bound):
    """Per element |got - ref| / bound -- where the bound is 0 (an empty row: nothing is rounded) any difference is inf;
    inf where ``got`` is not finite."""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), e, np.inf)


# ---- denominators -------------------------------------------------------------------------------------------------------
def colsum(panel):
    return np.asarray(panel, dtype=np.float64).sum(0)


def gram(panel, drop_last_chunk=False):
    """(panel^T panel, its bound).  ``drop_last_chunk``: the seeded fault (h)."""
    f = np.asarray(panel, dtype=np.float64)
    rows = f.shape[0]
    per = -(-rows // GRAM_CHUNKS)
    if drop_last_chunk:
        last = (min(rows, GRAM_CHUNKS * per) - 1) // per          # the last chunk that holds a row
        f = f[:last * per]
    g = f.T @ f
    k = 1 + (-(-per // 4) + 1) + 2 + GRAM_CHUNKS
    return g, k * U * g                                             # (all terms >= 0: sum |terms| is the sum)


def gram_ops(rows: int) -> int:
    per = -(-rows // GRAM_CHUNKS)
    return 1 + (-(-per // 4) + 1) + 2 + GRAM_CHUNKS


def rowmat(owner, g, rows_panel: int):
    """(owner @ gram, its bound against the float64 Gram matrix: the Gram's own roundings + one multiply + rank adds)."""
    o = np.asarray(owner, dtype=np.float64)
    den = o @ g
    return den, (gram_ops(rows_panel) + 1 + g.shape[0]) * U * (np.abs(o) @ np.abs(g))


def generic_den(A_img, B_img, beta: float, precision: str, M: int, K: int):
    """What nmfmu_den_partial (kModeDen) leaves: den = Gp(S) @ panel from the image planes, no target.  Returns
    mu_emulation.half_step's dict ('den', 'den_amb')."""
    X = np.zeros((A_img[0].shape[0], B_img[0].shape[0]))
    return E.half_step(X, None, None, beta, precision, M=M, K=K, A_img=A_img, B_img=B_img)


def generic_den_exact(owner, panel, beta: float):
    """The same term with unrounded operands (oracle: (H W^T + eps)^(beta - 1) @ W)."""
    o, p = np.asarray(owner, np.float64), np.asarray(panel, np.float64)
    return np.power(o @ p.T + EPS, float(beta) - 1.0) @ p


apply = E.apply
apply_allowance = E.apply_allowance
APPLY_OPS = 8     # apply_kernel on top of its inputs: relu + eps twice, + l1, + l2 theta (2), divide, powf (2 u), multiply


def half_step(csr_, owner, panel, beta, gamma, l1=0.0, l2=0.0, rows=None, den=None, kl_den=None):
    """One unrounded half-step: (new owner rows, numerator dict, denominator)."""
    em = numerator(csr_, owner, panel, beta, rows)
    o = np.asarray(owner, np.float64)
    o = o if rows is None else o[rows]
    kind = E.beta_kind(beta)
    if kind == 'kl':
        kl_den = colsum(panel) if kl_den is None else kl_den
    elif den is None:
        den = rowmat(o, gram(panel)[0], len(panel))[0] if kind == 'euc' else generic_den_exact(o, panel, beta)
    return E.apply(o, em['num'], den, beta, gamma, l1, l2, kl_den=kl_den), em, den


# ---- loss ---------------------------------------------------------------------------------------------------------------
def v_norm(vals, beta: float) -> float:
    """nmf.py:172-181 over the stored values (a stored 0 at beta == 1 gives 0 log 0 = NaN, as in the reference)."""
    v = np.asarray(vals, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        if beta == 2:
            return float(v @ v * 0.5)
        if beta == 1:
            return float(np.sum(v * np.log(v)) - v.sum()) if len(v) else 0.0
        return float(np.power(v, beta).sum() / beta / (beta - 1))


def v_norm_bound(vals, beta: float) -> float:
    """A float64 sum of n terms in any order, each a 1-ulp log / pow and a multiply: (n + 4) 2^-53 sum |terms|."""
    v = np.asarray(vals, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        if beta == 2:
            a = float(v @ v * 0.5)
        elif beta == 1:
            a = float(np.nansum(np.abs(v * np.log(v))) + np.abs(v).sum())
        else:
            a = float(np.power(v, beta).sum() / beta / abs(beta - 1))
    return (len(v) + 4) * 2.0 ** -53 * a + 1e-300


def loss_neg(csr_h, H, W, beta: float):
    """(neg, bound): sum over the stored entries of v log(s + eps) | v s | v (s + eps)^(beta - 1) / (beta - 1)."""
    rowptr, colidx, vals = csr_h
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    RL = rank_slots(E.pad_rank(W.shape[1]))
    r = row_of_entry(rowptr)
    v = vals.astype(np.float64)
    s = np.einsum('pr,pr->p', H[r], W[colidx.astype(np.int64)]) if len(v) else np.zeros(0)
    se = s + EPS
    kind = E.beta_kind(beta)
    if kind == 'kl':
        t = v * np.log(se)
        b = np.abs(v) * (np.abs(np.log(se)) * (ULP_FN + 1) + (RL + 8))
    elif kind == 'euc':
        t = v * s
        b = np.abs(t) * (RL + 7 + 1)
    else:
        c = float(np.float32(beta)) - 1.0
        t = v * np.power(se, c) / c
        expo = abs(c) * np.abs(np.log2(se)) * (ULP_FN + 1) + abs(c) * (RL + 8) / LN2
        b = np.abs(t) * (expo * LN2 + ULP_FN + 2)
    return float(t.sum()), float(b.sum() * U)


def loss_pos(H, W, beta: float, A_img=None, B_img=None, r_pad=None, tiles=None):
    """(pos, bound).  beta == 1: colsum . colsum; beta == 2: 1/2 sum(H^T H * W^T W); otherwise sum (S + eps)^beta / beta
    over EVERY entry -- from the image planes the fused loss mode reads when they are given."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    kind = E.beta_kind(beta)
    if kind == 'kl':
        pos = float(W.sum(0) @ H.sum(0))
        return pos, 2e-6 * abs(pos) + 1e-300          # two column sums at the dense file's 1e-6 each
    if kind == 'euc':
        pos = 0.5 * float((H.T @ H).reshape(-1) @ (W.T @ W).reshape(-1))
        return pos, (gram_ops(len(H)) + gram_ops(len(W))) * U * abs(pos) + 1e-300
    if A_img is None:
        S = H @ W.T + EPS
        return float(np.power(S, beta).sum() / beta), 0.0
    planes = 3 if A_img[1] is not None else 1
    S = E._gemm([A_img[0]] if A_img[1] is None else list(A_img), B_img[0].T, None if B_img[1] is None else B_img[1].T) + EPS
    t = np.power(S, beta) / beta
    s_ops = planes * r_pad                                         # MFMA accumulation of S (every product exact in fp32)
    k = (s_ops * beta + beta * np.abs(np.log2(S)) * LN2 * (ULP_FN + 1) + ULP_FN + 3) + 32 * tiles + 16
    return float(t.sum()), float((k * t).sum() * U)


# ---- problems -------------------------------------------------------------------------------------------------------------
def parity_cases():
    """The case matrix of tests/test_gpu_sparse_emulated_parity.py."""
    cases = []

    def add(layout, beta, N, C, R, claims=(), regs=(0.0, 0.0), nsplit=None, axis=0, density=0.1, sample=None, dups=False,
            stored_zero=False, zero_owner=False, empty_col=False):
        r_pad = E.pad_rank(R)
        auto = [f'rl{rank_slots(r_pad)}', f'rpad{r_pad}']
        if E.beta_kind(beta) not in ('kl', 'euc'):
            auto.append('bf16x3' if r_pad <= 128 else 'bf16')
        for name, n in (('n', N), ('c', C)):
            if n % 4:
                auto.append(f'{name}_mod4_{n % 4}')
            if n < 4:
                auto.append(f'{name}_lt4')
            if n < GRAM_CHUNKS:
                auto.append(f'{name}_lt64')
        tag = f'{layout}{"T" if axis else ""}-b{beta:g}-{N}x{C}r{R}' + (f'-ns{nsplit}' if nsplit else '') + \
            ('-reg' if regs != (0.0, 0.0) else '') + ('-dup' if dups else '') + ('-z' if stored_zero else '') + \
            ('-zo' if zero_owner else '') + ('-ec' if empty_col else '')
        cases.append(dict(id=tag, layout=layout, beta=float(beta), N=N, C=C, R=R, regs=regs, nsplit=nsplit, axis=axis,
                          density=density, sample=sample, dups=dups, stored_zero=stored_zero, zero_owner=zero_owner,
                          empty_col=empty_col, claims=tuple(claims) + tuple(auto)))

    res = ('residues', 'empty_row', 'full_row')
    # every residue of the 4-entry unroll, an empty and a full row; owner-row counts off the 4-row workgroup and below the
    # 64 Gram chunks -- on the rows of V (H half-step) and on its columns (W half-step)
    add('res', 1, 61, 130, 5, res)
    add('res', 2, 61, 130, 33, res, regs=(0.1, 0.5))
    add('res', 1, 130, 62, 1, res, axis=1)
    add('res', 2, 131, 63, 64, res, axis=1)
    add('res', 1, 3, 50, 32, ('residues3',), regs=(0.1, 0.5))
    add('res', 2, 3, 50, 5, ('residues3',))
    add('res', 2, 50, 3, 65, ('residues3',), axis=1)
    add('res', 1, 50, 2, 100, ('residues2',), axis=1)
    add('res', 0.5, 61, 130, 5, res)
    add('res', 3, 131, 63, 200, res, axis=1)
    # both sides of every RL boundary and every pad_rank class
    for i, R in enumerate((32, 64, 65, 128, 129, 200, 256)):
        add('rand', 1, 70, 90, R, regs=(0.1, 0.5) if i % 2 else (0.0, 0.0))
    for i, R in enumerate((1, 100, 128, 129, 200, 256)):
        add('rand', 2, 90, 70, R, regs=(0.0, 0.0) if i % 2 else (0.1, 0.5))
    # generic beta: split-bf16 images up to padded rank 128, bf16 above; forced contraction splits
    add('rand', 0.5, 70, 90, 33)
    add('rand', 1.5, 90, 70, 128, regs=(0.1, 0.5))
    add('rand', 3, 70, 90, 64, regs=(0.1, 0.5))
    add('rand', 0.5, 70, 90, 129, regs=(0.1, 0.5))
    add('rand', 1.5, 90, 70, 200)
    add('rand', 3, 70, 90, 256)
    add('rand', 0.5, 300, 600, 33, ('split',), nsplit=2, density=0.03)
    add('rand', 1.5, 600, 300, 100, ('split',), nsplit=3, density=0.03, regs=(0.1, 0.5))
    add('rand', 3, 300, 600, 200, ('split',), nsplit=2, density=0.03)
    # duplicates in an uncoalesced target, a stored 0.0, an owner row of zeros, an empty column
    for beta, R in ((1, 5), (2, 65), (0.5, 100), (1, 200), (2, 129)):
        add('res', beta, 61, 130, R, ('residues', 'empty_row', 'empty_col', 'duplicates', 'stored_zero', 'zero_owner'),
            dups=True, stored_zero=True, zero_owner=True, empty_col=True)
    # no stored entry at all
    for beta in (1, 2, 0.5):
        add('empty', beta, 10, 9, 5, ('no_entries',))
    # a larger target: a few thousand rows, density below 1 %, skewed row lengths; a sample of the rows is checked
    add('skew', 1, 3001, 2502, 100, ('skewed', 'sparse1pct'), sample=64)
    add('skew', 2, 3001, 2502, 200, ('skewed', 'sparse1pct'), sample=64, regs=(0.1, 0.5))
    return cases


def _pattern(case, g):
    """Row lengths and columns of the entries on an (n, c) grid (n = the axis the layout is drawn on)."""
    n, c = (case['C'], case['N']) if case['axis'] else (case['N'], case['C'])
    allowed = np.arange(c)
    if case['empty_col'] and not case['axis']:
        allowed = np.delete(allowed, 1)
    layout = case['layout']
    if layout == 'res':
        cyc = [0, 1, 2, 3, 4, 5, len(allowed) if not case['empty_col'] else 6]
        counts = np.array([min(cyc[i % 7], len(allowed)) for i in range(n)])
    elif layout == 'rand':
        counts = g.binomial(len(allowed), case['density'], size=n)
    elif layout == 'skew':
        counts = np.minimum((g.pareto(1.2, size=n) * 4).astype(np.int64), len(allowed) // 4)
    else:
        counts = np.zeros(n, dtype=np.int64)
    rows = np.repeat(np.arange(n), counts)
    cols = np.concatenate([g.choice(allowed, size=k, replace=False) for k in counts]) if counts.sum() else np.zeros(0, np.int64)
    if case['empty_col'] and case['axis']:
        raise ValueError('empty_col is drawn on axis 0')
    return (cols, rows) if case['axis'] else (rows, cols)


def make_problem(case, seed=None):
    """(idx [2, nnz] int64 -- uncoalesced, with duplicates where the case asks --, vals fp32, (N, C), W0, H0) on the CPU."""
    N, C, R = case['N'], case['C'], case['R']
    g = np.random.default_rng(seed if seed is not None else (N * 7 + C * 3 + R * 11 + int(case['beta'] * 10)) % 100003)
    ii, jj = _pattern(case, g)
    vals = (np.floor(g.random(len(ii)) * 1024) + 1) / 1024            # on a 2^-10 grid in (0, 1]
    if case['stored_zero'] and len(vals):
        vals[g.choice(len(vals), size=min(3, len(vals)), replace=False)] = 0.0
    if case['dups'] and len(vals):
        pick = g.choice(len(vals), size=max(1, len(vals) // 5), replace=False)
        part = np.floor(vals[pick] * 512) / 1024                     # v = part + (v - part), both on the grid
        vals[pick] -= part
        ii, jj, vals = np.concatenate([ii, ii[pick]]), np.concatenate([jj, jj[pick]]), np.concatenate([vals, part])
        order = g.permutation(len(vals))
        ii, jj, vals = ii[order], jj[order], vals[order]
    tg = torch.Generator().manual_seed(int(g.integers(1 << 30)))
    W0 = torch.randn(C, R, generator=tg).abs() + 0.05
    H0 = torch.randn(N, R, generator=tg).abs() + 0.05
    if case['zero_owner']:       # an owner row of zeros in each half-step, on the row / column of V with the most entries
        H0[int(np.bincount(ii, minlength=N).argmax())] = 0.0
        W0[int(np.bincount(jj, minlength=C).argmax())] = 0.0
    idx = np.stack([ii, jj]).astype(np.int64).reshape(2, -1)
    return idx, vals.astype(np.float32), (N, C), W0, H0


def plan(case, ncu: int = 256):
    """Precision, padded rank and contraction splits the engine must choose."""
    r_pad = E.pad_rank(case['R'])
    generic = E.beta_kind(case['beta']) not in ('kl', 'euc')
    prec = 'bf16x3' if generic and r_pad <= 128 else 'bf16'
    ns = {'h': 1, 'w': 1}
    if generic:
        n_pad, c_pad = E.pad_rows(case['N']), E.pad_rows(case['C'])
        ns = {'h': E.choose_nsplit(n_pad, c_pad, r_pad, prec, case['beta'], 128, ncu, case['nsplit']),
              'w': E.choose_nsplit(c_pad, n_pad, r_pad, prec, case['beta'], 128, ncu, case['nsplit'])}
    return dict(precision=prec, r_pad=r_pad, nsplit=ns, generic=generic)


def claim_holds(claim: str, case, problem) -> bool:
    """Does the generated problem have the structure ``claim`` names?"""
    idx, vals, (N, C), W0, H0 = problem
    cidx, cvals = coalesce(idx, vals, (N, C))
    rc = np.bincount(cidx[0], minlength=N)
    cc = np.bincount(cidx[1], minlength=C)
    own, other = (cc, rc) if case['axis'] else (rc, cc)     # the axis the layout was drawn on
    width = N if case['axis'] else C
    pl = plan(case)
    if claim.startswith(('n_mod4_', 'c_mod4_')):
        return (N if claim[0] == 'n' else C) % 4 == int(claim[-1])
    if claim in ('n_lt4', 'c_lt4'):
        return (N if claim[0] == 'n' else C) < 4
    if claim in ('n_lt64', 'c_lt64'):
        return (N if claim[0] == 'n' else C) < GRAM_CHUNKS
    if claim.startswith('rl'):
        return rank_slots(pl['r_pad']) == int(claim[2:])
    if claim.startswith('rpad'):
        return pl['r_pad'] == int(claim[4:])
    return {
        'residues': lambda: set(range(6)) <= set(own.tolist()) and {0, 1, 2, 3} <= set((own % 4).tolist()),
        'residues3': lambda: {0, 1, 2} <= set(own.tolist()),
        'residues2': lambda: {0, 1} <= set(own.tolist()),
        'empty_row': lambda: (own == 0).any(),
        'full_row': lambda: own.max() == width,
        'empty_col': lambda: cc[1] == 0 and (rc == 0).any(),          # an empty owner row of BOTH half-steps
        'duplicates': lambda: len(cvals) < len(vals),
        'stored_zero': lambda: (cvals == 0).any(),
        'zero_owner': lambda: bool(((H0.abs().sum(1) == 0).numpy() & (rc > 0)).any()
                                   and ((W0.abs().sum(1) == 0).numpy() & (cc > 0)).any()),
        'no_entries': lambda: len(cvals) == 0,
        'split': lambda: max(pl['nsplit'].values()) > 1,
        'bf16x3': lambda: pl['generic'] and pl['precision'] == 'bf16x3',
        'bf16': lambda: pl['generic'] and pl['precision'] == 'bf16',
        'skewed': lambda: rc.max() >= 8 * max(np.median(rc), 1) and (rc == 0).any() and N >= 2000,
        'sparse1pct': lambda: len(cvals) <= 0.01 * N * C,
    }[claim]()
