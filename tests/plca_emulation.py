"""Float64 emulation of the PLCA / SIPLCA EM step from given numerators, with per-output error bounds (test-only).

An EM iteration (reference plca.py:248-290) is two contractions -- the unscaled numerators ``numW = G^T H`` and ``numH = G W``
with ``G = Vn / (H diag(Z) W^T + eps)``, emulated by ``mu_emulation.half_step`` (split panel: ``B2_img``) and by
tests/conv_emulation.py -- and an O((N + C) R) remainder that the small kernels of pytorch-nmf_amd/csrc/nmfmu_plca.hip
compute.  This module is that remainder, for 2-D factors (rows, R) and for [outer][R][inner...] factors alike: the rank axis
is axis 1 and "column sum" means the sum over every other axis (``get_norm`` of plca.py:27-35).

The update, exactly as plca.py:255-289 orders it (``em_step``):

    Zg[r]  = sum W_old * numW                                   (Z.grad, plca.py:250: always from the OLD W)
    if Z trains:  Z1 = Z_old * relu(Zg);  Z_prior = Z1          (BEFORE the Dirichlet prior of Z is added)
                  if Z_alpha != 1:  Z1 = max(Z1 + fp32(Z_alpha - 1), eps)
                  Z = Z1 / sum(Z1)
    if W trains:  W = W_old * relu(numW * Z_old);  if Z_prior is None: Z_prior = colsum(W)
                  W = W / Z_prior
                  if W_alpha != 1:  W = max(W + fp32(W_alpha - 1), eps);  W = W / colsum(W)      (only this branch renormalises)
    if H trains:  the same with numH, H_alpha; if neither Z nor W trained, Z_prior = colsum of the multiplied H

``fp32(alpha - 1)``: the reference subtracts two Python floats (double) and the in-place add on an fp32 tensor rounds the
result ONCE (``prior_shift``).  fp32(alpha) - 1.f -- what the kernels computed before -- is another number: 4.7e-5 relative
at alpha = 1.001 (seeded fault 'alpha_f32').  The clamp is ``x > eps ? x : eps`` (F.threshold).  All seven non-empty
combinations of trainable W / H / Z follow from the three ``if``s.

Error bounds
------------
Every fp32 operation of the kernels is correctly rounded (+, *, /; hipcc keeps fp32 division IEEE), so it returns its exact
result times (1 + d), |d| <= u = 2^-24, or is off by at most half the smallest subnormal (``TINY``) where it underflows.
The bounds below are these per-operation errors propagated to first order through the float64 formulas and multiplied by
``SECOND`` = 1 + 2^-10, which exceeds the neglected products of errors as long as every count k u stays below 2^-10 (k <
16384; the largest chain here is 407).  No number comes from a run.  A value is carried as ``Val(v, e)``: float64 value and
absolute bound; inputs read back from the device are exact (e = 0).

Elementwise chains (``stage_em``, ``stage_normalize``, ``stage_scale``, ``stage_z``):

* numerator n = sum of ``nslab`` slab planes, added in order onto 0.f (the first add is exact): nslab - 1 roundings,
  |dn| <= (nslab - 1) u sum_s |n_s|                                      (plca_kernel<0>, nmfmu_plca.hip:41)
* x = f * relu(n * z): two multiplies; relu is 1-Lipschitz:  e_x = |f z| dn + 2 u |x|                  (:43)
* Z.grad term p = f * n accumulated as ``zg += x * n`` (a product and an add, or ONE fma -- fewer roundings, same bound):
  e_p = |f| dn + u |p|, the add is counted in the sum's chain                                          (:42)
* q = x / d: one divide; with the divisor known to e_d:  e_q = e_x / d + |q| e_d / d + u |q|           (:45)
* y = q + shift: one add, e_y = e_q + u |y| -- ABSOLUTE, because q + (alpha - 1) cancels for alpha < 1; max(y, eps) is
  continuous and 1-Lipschitz, so the clamp adds nothing and needs no ambiguity allowance              (:46-49)
* o = y / c (plca_scale_kernel :67, plca3_kernel<2>):  e_o = e_y / c + |o| e_c / c + u |o|
* z1 = z * relu(zg): e = |z| e_zg + u |z1|; + shift, clamp as above; z = z1 / S: e_z = e_z1 / S + z e_S / S + u z  (:79-92)

Fixed-order sums: a sum of terms t_i, each known to e_i, added along chains of at most k fp32 additions, is within
sum e_i + k u sum (|t_i| + e_i) of the exact sum.  k is read off the kernels (``chain_rows``, ``chain_plca3``, ``CHAIN_Z``):

* plca_kernel (:34-62) + colsum_finalize_kernel (nmfmu_aux.hip:291-322): a thread adds its 32 / groups = r_pad / 8 rows onto
  0.f (r_pad / 8 - 1 roundings), thread group 0 adds the other ``groups`` - 1 partials in order, a finalize thread adds its
  ceil(nblk / 32) block partials onto 0.f (one less rounding; the unrolled loop of eight keeps the order of the plain one)
  and thread row 0 adds the 31 other rows in order:  k = (r_pad / 8 - 1) + (groups - 1) + (ceil(nblk / 32) - 1) + 31.
* plca3_kernel (:115-141) + plca3_final_kernel (:148-156): a thread adds ceil(per / 256) elements of its chunk (per =
  ceil(outer inner / 64)) onto 0.f, the LDS tree has 8 levels, the final thread adds the 64 chunk partials onto 0.f:
  k = (ceil(per / 256) - 1) + 8 + 63.
* plca_z_kernel (:88-91): an 8-level LDS tree over 256 slots: k = 8.  (SIPLCA updates Z with torch ops: the same
  roundings, the sum in an order torch does not promise: k = R - 1.)

Column sums that must be 1 (``unit_sum_bound``): after a renormalisation f = y / c with c the device's own fp32 sum of the
positive y: sum_i fl(y_i / c) = (1 + u') sum y_i / (sum y_i (1 + k u'')) -- within (k + 1) u of 1.  Without a prior and with
non-negative numerators, sum_i W_new = sum_i x_i / Z_prior with Z_prior = z relu(Zg): both are sums of the same products f n
z, x_i carrying (nslab - 1) + 2 roundings, Z_prior (nslab - 1) + 1 (product) + k (chain) + 1 (times z), the division one:
within (2 (nslab - 1) + 5 + k) u of 1; the larger of the two is used for both.

The loss (``kl_loss``): nmfmu_loss adds ``loss_elem`` (nmfmu_fused.h:333-341) = x (log2(x + eps) - log2 S) ln2 - x + (S - eps)
in fp32 per lane -- 32 elements per 64-column tile, then 6 shuffle levels and 2 adds -- and the block partials in double.  Per
element: S carries the r_pad fp32 accumulations of its MFMAs and eps (r_pad + 1 roundings: relative (r_pad + 1) u in S - eps,
absolute (r_pad + 1) u / ln2 in log2 S; three times the products in bf16x3), each v_log_f32 is good to one ulp (2 u of its result), ln2 as an fp32 constant, the
subtraction, two multiplies and two adds one rounding each.  Summed: ``elem_terms`` below; the chain adds k u sum |elem| with
k = 32 tiles + 8.

Host mirrors of the launch arithmetic (``pad_rank``, ``nblk``, ``groups``, ``finalize_plan``, ``part_bytes``,
``chunk_bounds``, ``part3_bytes``) let a case assert that it reaches the branch it is named for.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import mu_emulation as E

EPS = E.EPS
U = 2.0 ** -24
TINY = 2.0 ** -149
SECOND = 1.0 + 2.0 ** -10
PLCA_ROWS = 32          # kPlcaRows
PLCA3_CHUNKS = 64       # kPlca3Chunks
CHAIN_Z = 8             # plca_z_kernel's LDS tree
LN2 = float(np.float32(0.6931471805599453))

Val = namedtuple('Val', 'v e')


def exact(x) -> Val:
    x = np.asarray(x, dtype=np.float64)
    return Val(x, np.zeros_like(x))


# ---- host mirrors ----------------------------------------------------------------------------------------------------
pad_rank = E.pad_rank


def nblk(rows: int) -> int:
    return -(-rows // PLCA_ROWS)


def groups(r_pad: int) -> int:
    return 256 // r_pad


def part_bytes(rows: int, r_pad: int) -> int:
    """nmfmu_plca_part_bytes: two planes (column sums, Z.grad) of nblk x r_pad floats."""
    return 2 * nblk(rows) * r_pad * 4 if rows > 0 and r_pad > 0 else 0


def part3_bytes(rank: int) -> int:
    """nmfmu_plca3_part_bytes: (column sum, Z.grad) per rank and chunk."""
    return rank * PLCA3_CHUNKS * 2 * 4 if rank > 0 else 0


def finalize_plan(nb: int) -> dict:
    """colsum_finalize_kernel on ``nb`` partial blocks: thread row g (0..31) starts at b = g; the unrolled loop takes eight
    partials (stride 32) while b + 224 < nb, the plain loop the rest.  unrolled / tail: does any thread row run them."""
    unrolled = tail = 0
    terms = 0
    for g in range(32):
        b, n = g, 0
        while b + 7 * 32 < nb:
            b, n, unrolled = b + 8 * 32, n + 8, unrolled + 1
        while b < nb:
            b, n, tail = b + 32, n + 1, tail + 1
        terms = max(terms, n)
    return dict(unrolled=unrolled > 0, tail=tail > 0, tail_after_unrolled=unrolled > 0 and nb > 256, terms=terms)


def chain_rows(rows: int, r_pad: int) -> int:
    """Longest chain of fp32 additions behind one column sum of plca_kernel + colsum_finalize_kernel (module docstring)."""
    return (r_pad // 8 - 1) + (groups(r_pad) - 1) + (finalize_plan(nblk(rows))['terms'] - 1) + 31


def chunk_bounds(outer: int, inner: int):
    """[e0, e1) of each of the 64 chunks of plca3_kernel over the outer x inner index space (empty chunks: e0 >= e1)."""
    n = outer * inner
    per = -(-n // PLCA3_CHUNKS)
    return [(ch * per, min(n, ch * per + per)) for ch in range(PLCA3_CHUNKS)]


def chain_plca3(outer: int, inner: int) -> int:
    per = -(-(outer * inner) // PLCA3_CHUNKS)
    return max(-(-per // 256) - 1, 0) + 8 + (PLCA3_CHUNKS - 1)


def grid_scale(n: int):
    """(workgroups, elements per thread at most) of plca_scale_kernel: grid-stride above 4096 x 256 elements."""
    grid = min(-(-n // 256), 4096)
    return grid, -(-n // (grid * 256))


# ---- the constant of the Dirichlet prior -----------------------------------------------------------------------------
def prior_shift(alpha, rounding=True) -> float:
    """alpha - 1 as the reference adds it: the subtraction in double, rounded once to fp32 by the in-place add."""
    d = float(alpha) - 1.0
    return float(np.float32(d)) if rounding else d


def prior_shift_f32(alpha) -> float:
    """fp32(alpha) - 1.f: the seeded fault 'alpha_f32' (what the kernels computed from a float argument)."""
    return float(np.float32(np.float32(alpha) - np.float32(1.0)))


# ---- stages ----------------------------------------------------------------------------------------------------------
def _rv(v, like):
    """A rank vector broadcast along axis 1 of ``like``."""
    v = np.asarray(v, dtype=np.float64)
    return v.reshape((1, -1) + (1,) * (like.ndim - 2)) if like.ndim > 1 else v


def _axes(x):
    return tuple(i for i in range(x.ndim) if i != 1) if x.ndim > 1 else (0,)


def colsum(t: Val, k: int, u: float = U, drop=None) -> Val:
    """Fixed-order sum over everything but the rank axis.  ``drop``: index of axis 0 left out (seeded fault)."""
    v, e = t.v, t.e
    if drop is not None:
        keep = np.ones(v.shape[0], dtype=bool)
        keep[drop] = False
        v, e = v[keep], e[keep]
    ax = _axes(v)
    return Val(v.sum(ax), SECOND * (e.sum(ax) + k * u * (np.abs(v) + e).sum(ax)))


def stage_em(f, slabs, z_old, k: int, u: float = U, fault=None) -> dict:
    """plca_kernel<0> / plca3_kernel<0>: x = f * relu(n * z_old) with n = the sum of the slab planes ``slabs`` [nslab, *f.shape],
    cs = column sums of x, zg = sum f * n.  ``f`` may be a Val (composite steps)."""
    f = f if isinstance(f, Val) else exact(f)
    slabs = np.asarray(slabs, dtype=np.float64)
    if slabs.ndim == f.v.ndim:
        slabs = slabs[None]
    n = slabs.sum(0)
    dn = (slabs.shape[0] - 1) * u * np.abs(slabs).sum(0)
    z = _rv(z_old, f.v)
    t = n * z
    x = f.v * (t if fault == 'no_relu' else np.maximum(t, 0.0))
    ex = SECOND * (np.abs(f.v * z) * dn + 2 * u * np.abs(x) + f.e * np.abs(np.maximum(t, 0.0)) + TINY * (1 + np.abs(f.v)))
    p = f.v * n
    ep = SECOND * (np.abs(f.v) * dn + u * np.abs(p) + f.e * np.abs(n) + TINY)
    xv = Val(x, ex)
    return dict(x=xv, cs=colsum(xv, k, u, drop=(x.shape[0] - 1) if fault == 'ragged_row' else None),
                zg=colsum(Val(p, ep), k, u), n=n)


def _prior(q: Val, alpha, u, rounding, fault) -> Val:
    if alpha == 1:
        return q
    s = prior_shift_f32(alpha) if fault == 'alpha_f32' else prior_shift(alpha, rounding)
    y = q.v + s
    floor = 0.0 if fault == 'clamp0' else EPS
    return Val(np.where(y > floor, y, floor), SECOND * (q.e + u * np.abs(y)))


def stage_normalize(x, d, alpha, k: int, u: float = U, rounding=True, fault=None) -> dict:
    """plca_kernel<1> / plca3_kernel<1>: y = x / d[r]; with a prior y = max(y + shift, eps); cs = column sums of y."""
    x = x if isinstance(x, Val) else exact(x)
    d = d if isinstance(d, Val) else exact(d)
    dv, de = _rv(d.v, x.v), _rv(d.e, x.v)
    q = x.v / dv
    eq = SECOND * (x.e / np.abs(dv) + np.abs(q) * de / np.abs(dv) + u * np.abs(q) + TINY)
    y = _prior(Val(q, eq), alpha, u, rounding, fault)
    return dict(y=y, cs=colsum(y, k, u))


def stage_scale(y, c, u: float = U) -> Val:
    """plca_scale_kernel / plca3_kernel<2>: y / c[r]."""
    y = y if isinstance(y, Val) else exact(y)
    c = c if isinstance(c, Val) else exact(c)
    cv, ce = _rv(c.v, y.v), _rv(c.e, y.v)
    with np.errstate(divide='ignore', invalid='ignore'):        # (a zero column sum: only a seeded fault produces one)
        o = y.v / cv
        return Val(o, SECOND * (y.e / np.abs(cv) + np.abs(o) * ce / np.abs(cv) + u * np.abs(o) + TINY))


def stage_z(z, zg, alpha, k: int = CHAIN_Z, u: float = U, rounding=True, fault=None) -> dict:
    """plca_z_kernel (plca.py:253-260): prior = z * relu(zg); z = normalised (prior, with the Dirichlet prior added)."""
    z = np.asarray(z, dtype=np.float64)
    zg = zg if isinstance(zg, Val) else exact(zg)
    p = z * np.maximum(zg.v, 0.0)
    prior = Val(p, SECOND * (np.abs(z) * zg.e + u * np.abs(p) + TINY))
    z1 = _prior(prior, alpha, u, rounding, fault)
    S = z1.v.sum()
    eS = SECOND * (z1.e.sum() + k * u * (np.abs(z1.v) + z1.e).sum())
    zn = z1.v / S
    out = Val(zn, SECOND * (z1.e / S + np.abs(zn) * eS / S + u * np.abs(zn) + TINY))
    return dict(prior=z1 if fault == 'prior_after' else prior, z=out, zsum_bound=SECOND * (k + 1) * u)


def unit_sum_bound(k: int, nslab: int = 1, u: float = U) -> float:
    """|column sum - 1| of a factor after its update (module docstring): the larger of the two derivations."""
    return SECOND * max(k + 1, 2 * (nslab - 1) + 5 + k) * u


def em_step(W, H, Z, numW, numH, train=(True, True, True), alphas=(1.0, 1.0, 1.0), kW=None, kH=None, kZ=CHAIN_Z,
            u: float = U, rounding=True, fault=None) -> dict:
    """One EM step from the unscaled numerators (``numW`` / ``numH``: one plane, or the slab planes [nslab, ...] as the device
    holds them).  ``alphas`` = (W_alpha, H_alpha, Z_alpha), ``train`` = (W, H, Z).  kW / kH / kZ: chain lengths of the
    column sums (default: the number of terms -- any order -- as for float64 round-off with u = 2^-53).  rounding=False:
    the prior constant stays a double.  Returns Vals W, H, Z, z_prior (None when nothing defines it) and zg."""
    tW, tH, tZ = train
    aW, aH, aZ = alphas
    W, H, Z = (np.asarray(a, dtype=np.float64) for a in (W, H, Z))
    R = Z.shape[0]
    kW = W.size // R if kW is None else kW
    kH = H.size // R if kH is None else kH
    f = fault
    sub = lambda *names: f if f in names else None
    z_old = Z
    mw = stage_em(W, numW, z_old, kW, u, fault=sub('no_relu'))
    out = dict(W=exact(W), H=exact(H), Z=exact(Z), zg=mw['zg'], z_prior=None)
    z_prior = None
    if tZ:
        zs = stage_z(Z, mw['zg'], aZ, kZ, u, rounding, fault=sub('prior_after', 'alpha_f32', 'clamp0'))
        out['Z'], z_prior = zs['z'], zs['prior']
    z_mul = out['Z'].v if f == 'z_new_for_old' else z_old

    def factor(theta, num, k, alpha, z_prior, mul=None):
        m = mul or stage_em(theta, num, z_mul, k, u, fault=sub('no_relu'))
        if z_prior is None:
            z_prior = m['cs']
        nm = stage_normalize(m['x'], z_prior, alpha, k, u, rounding, fault=sub('alpha_f32', 'clamp0'))
        new = nm['y']
        if alpha != 1 and f != 'no_renorm':
            new = stage_scale(nm['y'], nm['cs'], u)
        return new, z_prior

    if tW:
        out['W'], z_prior = factor(W, numW, kW, aW, z_prior, mul=mw if f != 'z_new_for_old' else None)
    if tH:
        out['H'], z_prior = factor(H, numH, kH, aH, z_prior)
    out['z_prior'] = z_prior
    return out


def excess(got, ref: Val) -> float:
    """max over the elements of |got - ref.v| / ref.e (0 / 0 = 0, x / 0 = inf); inf where ``got`` is not finite.  The check
    is ``excess(...) <= 1``."""
    got = np.asarray(got, dtype=np.float64)
    diff = np.abs(got - ref.v)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(ref.e > 0, diff / ref.e, np.where(diff == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max()) if r.size else 0.0


# ---- the loss --------------------------------------------------------------------------------------------------------
def kl_loss(x, A_img, B_img, nprod: int, tiles: int):
    """(sum of loss_elem, bound) over x [M, K] (the stored target) with S = A B^T + eps from the image planes (hi, lo or
    None).  nprod: products accumulated into one S (r_pad, three times that in bf16x3); tiles: 64-column tiles a lane walks."""
    (Ah, Al), (Bh, Bl) = A_img, B_img
    S = E._gemm([Ah] if Al is None else [Ah, Al], Bh.T, None if Bl is None else Bl.T) + EPS
    x = np.asarray(x, dtype=np.float64)
    lx, ls = np.log2(x + EPS), np.log2(S)
    d = lx - ls
    L = d * LN2
    elem = x * L - x + (S - EPS)
    rs = nprod + 1
    # error of L: ln2 (2 |lx| + 2 |ls| + 3 |d|) u from the logarithms, the subtraction, the constant and its multiply, plus
    # (rs + 1) u from the roundings of S and of x + eps inside the logarithms; then x L, x L - x, S - eps and the last add
    elem_terms = (x * (LN2 * (2 * np.abs(lx) + 2 * np.abs(ls) + 3 * np.abs(d)) + rs + 1)
                  + np.abs(x * L) + np.abs(x * L - x) + (rs + 1) * S + np.abs(elem))
    k = 32 * tiles + 8
    return float(elem.sum()), float(SECOND * U * (elem_terms.sum() + k * np.abs(elem).sum()))


def read_slabs(flat, nslab: int, rows: int, rows_pad: int, r_pad: int, rank: int, fault=None):
    """The numerator planes [nslab, rows, rank] of a flat slab buffer as plca_kernel<0> addresses it: plane s at
    s * rows_pad * r_pad, row pitch r_pad.  fault 'stride': the plane stride taken as rows * r_pad."""
    flat = np.asarray(flat).reshape(-1)
    plane = (rows if fault == 'stride' else rows_pad) * r_pad
    idx = (np.arange(nslab)[:, None, None] * plane + np.arange(rows)[None, :, None] * r_pad + np.arange(rank)[None, None, :])
    return flat[idx]


# ---- problems and the case lists of tests/test_gpu_plca_emulated_parity.py ---------------------------------------------
def synthetic(shape, seed, nslab=1, plane_shape=None):
    """(f, slabs, z) for the ABI tests: operands of order 1; numerators with zeros and negative entries (relu); the slab
    planes are [nslab, *plane_shape] (plane_shape >= shape: padded rows / pitch), NaN outside the region a kernel may read."""
    g = np.random.default_rng(seed)
    f = g.random(shape).astype(np.float32) + np.float32(0.01)
    f[g.random(shape) < 0.05] = 0.0
    R = shape[1]
    z = (g.random(R).astype(np.float32) + np.float32(0.05))
    num = g.standard_normal((nslab,) + tuple(shape)).astype(np.float32) + np.float32(0.4)
    num[:, g.random(shape) < 0.1] = 0.0            # (in every slab: the summed numerator is an exact zero there)
    return f, num, z


def norm_problem(case, seed=0):
    """(f, divider) of a NORM case: f of order divider / rows (a probability table after the division), some exact zeros."""
    g = np.random.default_rng(case['rows'] * 5 + case['rank'] + seed)
    f = (g.random((case['rows'], case['rank'])) * 2.0 / case['rows']).astype(np.float32)
    f[g.random(f.shape) < 0.05] = 0.0
    return f, (g.random(case['rank']) + 0.5).astype(np.float32)


def z_problem(case):
    """(z, zgrad) of a Z case: z a distribution, Z.grad around 1 (what an EM step gives) with some non-positive entries."""
    g = np.random.default_rng(case['rank'] * 3 + int(case['alpha'] * 1000))
    z = g.random(case['rank']).astype(np.float32) + np.float32(0.1)
    zg = (g.random(case['rank']) + 0.5).astype(np.float32)
    zg[1::7] = -zg[1::7]
    if case['rank'] > 2:
        zg[2] = 0.0
    return (z / z.sum(dtype=np.float32)).astype(np.float32), zg


# nmfmu_plca_em: rows, rank, nslab, rows_pad, update, zgrad; what each is there for
EM_CASES = [
    dict(rows=1, rank=1, nslab=1, rows_pad=1, update=1, zgrad=1, what='one element'),
    dict(rows=31, rank=5, nslab=3, rows_pad=256, update=1, zgrad=1, what='short of one block; slabs; rows_pad > rows'),
    dict(rows=32, rank=33, nslab=1, rows_pad=32, update=1, zgrad=0, what='exactly one block; r_pad 64; null zgrad_out'),
    dict(rows=33, rank=5, nslab=1, rows_pad=33, update=1, zgrad=1, what='one ragged row in a second block'),
    dict(rows=33, rank=100, nslab=3, rows_pad=256, update=0, zgrad=1, what='update 0: f untouched; r_pad 128'),
    dict(rows=300, rank=200, nslab=1, rows_pad=300, update=1, zgrad=1, what='r_pad 256: groups == 1'),
    dict(rows=300, rank=256, nslab=3, rows_pad=512, update=1, zgrad=1, what='no rank padding; slabs'),
    dict(rows=300, rank=33, nslab=3, rows_pad=512, update=0, zgrad=0, what='update 0, null zgrad_out'),
    dict(rows=9590, rank=5, nslab=1, rows_pad=9590, update=1, zgrad=1, what='300 blocks: unrolled finalize loop and tail'),
]

ALPHAS = (1.0, 1.001, 1.02, 0.99)
# nmfmu_plca_normalize + nmfmu_plca_scale: rows, rank, alpha
NORM_CASES = [dict(rows=r, rank=k, alpha=a) for r, k, a in (
    (1, 1, 1.02), (31, 5, 1.001), (32, 33, 0.99), (33, 100, 1.0), (33, 5, 1.02), (300, 200, 1.001), (300, 256, 0.99),
    (300, 1, 1.0), (520, 5, 1.001), (520, 5, 1.02), (9590, 5, 0.99), (4100, 256, 1.001))]
Z_CASES = [dict(rank=k, alpha=a) for k in (1, 5, 200, 256) for a in ALPHAS]
# nmfmu_plca3: outer, R, inner, pitch (None: R * inner)
PLCA3_CASES = [
    dict(outer=3, rank=1, inner=5, pitch=None, what='15 elements: fewer than the 64 chunks'),
    dict(outer=7, rank=70, inner=1, pitch=None, what='inner == 1; R > 64: second block of plca3_final_kernel'),
    dict(outer=70, rank=5, inner=16, pitch=128, what='W of SIPLCA (C 70, R 5, T 16): pitch = rp_pad = 128'),
    dict(outer=5, rank=3, inner=7, pitch=40, what='num_pitch > R * inner'),
    dict(outer=9, rank=4, inner=33, pitch=None, what='297 elements: not a multiple of 64'),
    dict(outer=300, rank=2, inner=70, pitch=None, what='21000 elements: more than 256 per chunk (per-thread chain)'),
]

# one dense EM step on _PlcaEM: N, C, R, precision, forced split
DENSE_CASES = [
    dict(N=330, C=520, R=5, precision='bf16x3', nsplit=None),
    dict(N=300, C=200, R=100, precision='bf16x3', nsplit=None),
    dict(N=257, C=131, R=33, precision='bf16', nsplit=None),
    dict(N=200, C=330, R=200, precision=None, nsplit=None),
    dict(N=130, C=260, R=256, precision='bf16', nsplit=None),
    dict(N=330, C=520, R=33, precision='bf16x3', nsplit=2),
]
TRAINS = [(True, True, True), (True, True, False), (True, False, True), (False, True, True), (True, False, False),
          (False, True, False), (False, False, True)]          # (W, H, Z): the seven non-empty combinations
PRIORS = [(1.0, 1.0, 1.0), (1.02, 0.99, 1.01), (1.001, 1.001, 1.001)]     # (W_alpha, H_alpha, Z_alpha)


def dense_id(c):
    return f"{c['N']}x{c['C']}r{c['R']}-{c['precision']}-ns{c['nsplit']}"


def dense_steps(i: int):
    """The (train, alphas) settings case i runs: all seven combinations, the prior setting rotating with case and step so that
    over the six cases every combination meets every prior setting twice."""
    return [(t, PRIORS[(i + j) % 3]) for j, t in enumerate(TRAINS)]


def dense_problem(case, seed=None):
    """(Vn, W0, H0, Z0) fp32 numpy, normalised as the PLCA constructor and fit() normalise them."""
    N, C, R = case['N'], case['C'], case['R']
    g = np.random.default_rng(N * 7 + C * 3 + R if seed is None else seed)
    V = g.random((N, C)).astype(np.float32)
    V[g.random((N, C)) < 0.05] = 0.0
    W = g.random((C, R)).astype(np.float32) + np.float32(0.01)
    H = g.random((N, R)).astype(np.float32) + np.float32(0.01)
    Z = g.random(R).astype(np.float32) + np.float32(0.1)
    f32 = np.float32
    return ((V / V.sum(dtype=f32)).astype(f32), (W / W.sum(0, dtype=f32)).astype(f32), (H / H.sum(0, dtype=f32)).astype(f32),
            (Z / Z.sum(dtype=f32)).astype(f32))


def dense_numerators(Vn, W, H, Z):
    """(numW, numH) in float64 without rounding: G^T H and G W with G = Vn / (H diag(Z) W^T + eps)."""
    Vn, W, H, Z = (np.asarray(a, dtype=np.float64) for a in (Vn, W, H, Z))
    G = Vn / (H @ (W * Z).T + EPS)
    return G.T @ H, G @ W


def split_plane_sensitivity(Vn, W, H, Z, which: str, precision: str) -> float:
    """How far the AMBIGUITY band of ``mu_emulation`` can move an emulated numerator of the split-panel half-step, per element
    (relative, ``elem_err``'s measure): the half-step is emulated with every Gn moved to either end of the band.  Single-plane
    modes carry a term-by-term allowance for it; the hi + lo pair of bf16x3 carries none (``half_step``), because a flip of the
    lo word moves a term by 2^-17 of it at most and the terms of a numerator average that down -- unless a few terms dominate
    the sum.  After an EM step with alpha = 0.99 most of H sits at the clamp (1e-7 against 1 / N), a numerator of W is a
    handful of terms, and this figure reaches 8e-6, twice TOL['bf16x3'] (4e-6): the emulation cannot say which neighbour
    the kernel took (tests/conv_emulation.py meets the same on a batch's first frame and reads the device's ratio planes
    back; the dense kernel keeps Gn in registers).  The GPU test therefore starts every step from the dense case's own
    start state, where the figure is below half of TOL (tests/test_plca_emulation.py asserts it)."""
    f32 = np.float32
    W, H, Z = (np.asarray(a, dtype=f32) for a in (W, H, Z))
    owner, panel = (W, H) if which == 'w' else (H, W)
    X = np.asarray(Vn, dtype=f32).T if which == 'w' else np.asarray(Vn, dtype=f32)
    img = lambda a: tuple(None if p is None else p.reshape(a.shape) for p in E.factor_image(a, precision))
    A, Bz, B = img(owner), img((panel * Z[None, :]).astype(f32)), img(panel)
    num = []
    for f in (1.0, 1.0 + E.AMBIGUITY, 1.0 - E.AMBIGUITY):
        rr = (lambda G, split, f=f: E.rounded_terms(G * f, precision, split))
        num.append(E.half_step(X, None, None, 1.0, precision, A_img=A, B_img=Bz, B2_img=B, ratio_round=rr)['num'] / f)
    return float(max(E.elem_err(num[1], num[0]).max(), E.elem_err(num[2], num[0]).max()))


# one EM step on _ConvPlcaEM: class, (B, C, ls, R, ts); both TORCHNMF_AMD_NMFD_H_ROWS settings
CONV_SHAPES = [('SIPLCA2', (2, 6, (12, 24), 3, (3, 8))), ('SIPLCA3', (1, 70, (5, 6, 16), 2, (2, 2, 8))),
               ('SIPLCA2', (1, 5, (9, 11), 4, (2, 3))), ('SIPLCA', (2, 70, (304,), 5, (16,))),
               ('SIPLCA', (4, 6, (256,), 3, (8,)))]      # (the last: 16 k-tiles of B L -- the (G^T H) GEMM is contraction-split)
CONV_KSPLIT_SHAPE = CONV_SHAPES[-1][1]
CONV_CASES = [dict(cls=c, shape=s, h_rows=h) for c, s in CONV_SHAPES for h in ('1', '0')]


def conv_id(c):
    B, C, ls, R, ts = c['shape']
    return f"{c['cls']}-{B}x{C}x{'x'.join(map(str, ls))}r{R}t{'x'.join(map(str, ts))}-rows{c['h_rows']}"


def conv_steps(i: int):
    """Three (train, alphas) settings per case, rotating, so that the cases see every prior setting with W + H + Z, with
    Z frozen and with W frozen."""
    return [(TRAINS[0], PRIORS[(i + 1) % 3]), (TRAINS[1], PRIORS[(i + 2) % 3]), (TRAINS[3], PRIORS[i % 3])]


def conv_problem(case):
    """(Vn, W0, H0, Z0) fp32 numpy, normalised over everything but the rank axis; W holds scattered exact zeros."""
    B, C, ls, R, ts = case['shape']
    lhs = tuple(l - t + 1 for l, t in zip(ls, ts))
    g = np.random.default_rng(B * 7 + C * 3 + R * 11 + int(np.prod(ls)))
    f32 = np.float32
    V = g.random((B, C) + tuple(ls)).astype(f32)
    W = g.random((C, R) + tuple(ts)).astype(f32) + f32(0.01)
    W[g.random(W.shape) < 0.05] = 0.0
    H = g.random((B, R) + lhs).astype(f32) + f32(0.01)
    Z = g.random(R).astype(f32) + f32(0.1)
    nrm = lambda x: (x / x.sum(_axes(x), keepdims=True, dtype=f32)).astype(f32)
    return (V / V.sum(dtype=f32)).astype(f32), nrm(W), nrm(H), (Z / Z.sum(dtype=f32)).astype(f32)
