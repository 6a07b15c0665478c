"""Float64 emulation of one convolutive MU half-step (nmfd_engine.ConvMU) that rounds where the device rounds (test-only).

A convolutive half-step is a dense half-step on the unfolded matrices: with ``Wm = W.view(C, R T)``,
``Hu[(b,l)][(r,t)] = H[b][r][l-t]`` (zero outside) and ``X_w[c][(b,l)]``, the W half-step is the dense one on
(X_w, Wm, Hu) and the H half-step the dense one on (X_w^T, Hu, Wm) followed by the col2im sum
``neg[b][r][j] = sum_t Y[(b, j+t)][(r,t)]``.  Several shift axes are flattened row-major, as ConvMU flattens them.  The
arithmetic is tests/mu_emulation.py's (``round_op``, ``split_op``, ``factor_image``, ``mu_terms``, ``_gemm``, ``apply``,
``apply_allowance``, ``elem_err``, ``AMBIGUITY``); this module adds the unfold / fold, the places where the conv kernels
round differently from the dense ones, the checks of the GPU test and its case list.

Rounding points, as the sources have them (pytorch-nmf_amd/csrc):

* operand planes / window tables of W and H (conv_apply_pack_w_kernel, conv_pack_wk_kernel, conv_tables_kernel,
  conv_unfold_kernel, the table writer of conv_fold_parts_apply_h_kernel): ``pack_img`` -- bf16 RNE; fp16 RNE clamped at
  65504; bf16x3 hi = bf16(x), lo = bf16(x - hi).  Zero in all padding.  The MFMA loop of nt_gemm_kernel forms
  lo hi + hi lo + hi hi (nmfmu_gemm.h:505-512), the three products of ``mu_emulation._gemm``.
* the target stays fp32 in every precision (``x_w`` / ``x_h`` are fp32 planes written by pack2d_kernel).
* accumulators seeded with eps except at beta == 2 (nmfmu_gemm.h:433-441; the ragged block ``racc`` likewise).
* ratio planes: ``mu_elem`` then ``pack_op`` (nmfmu_gemm.h:660-675): bf16 RNE, hi + lo in bf16x3, fp16 saturating
  (MODE.FP16_OVFL, nmfmu_gemm.h:132).  'f16' exists at beta == 1 only, so no 2^ki scale on this side.  The GEMM
  dispatch knows four beta kinds (KL, Euclid, IS, generic): beta = 0.5 and 1.5 take the generic exp2 / log2 branch here,
  where the dense kernels have closed forms -- the same value within AMBIGUITY.  Unlike the dense 16-bit modes, beta == 2
  rounds the fp32 target to the ratio plane here (there the stored word is the operand).
* ragged channels by direct summation (conv_ragged_rows_kernel): in bf16x3 its ``rnd`` is the identity -- the unrounded
  fp32 W and H are multiplied, not hi hi + hi lo + lo hi; in bf16 / f16 it rounds like the planes.  It packs Gn with
  pack_img (fp16: fminf 65504 then RNE, the value the saturating conversion gives) and Gp with pack_bf16 whatever the mode
  -- no difference in value, because 'f16' has no Gp.  ``exact_channels`` is the per-channel switch.  The in-grid form (one
  16 x 16 MFMA block per workgroup) reads the rounded planes.
* numerator GEMMs contract the 16-bit ratio planes with the other operand's planes into fp32; split-K slabs, tail-round
  parts and tile diagonal sums only change the summation order.
* apply: ``mu_update`` (nmfmu_nmfd.hip) = ``mu_emulation.apply`` (relu + eps, penalties, powf).  beta == 1 denominators
  are the closed form from the fp32 masters (sum_{b,j} H, sum_{c,t} W) however they travel.
* loss (EPI_LOSS, ragged mode 2): ``loss_elem`` of the reconstruction from the same rounded operands against fp32 V.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

import mu_emulation as E

EPS = E.EPS


# ---- geometry ----------------------------------------------------------------------------------------------------
def geometry(W, H):
    """(B, C, R, ts, lhs, ls) of W (C, R, *ts) and H (B, R, *lhs)."""
    ts, lhs = tuple(W.shape[2:]), tuple(H.shape[2:])
    return H.shape[0], W.shape[0], W.shape[1], ts, lhs, tuple(lh + t - 1 for lh, t in zip(lhs, ts))


def unfold(H, ts):
    """Hu[(b, l)][(r, t)] = H[b][r][l - t], zero outside; l and t flattened row-major over the shift axes."""
    H = np.asarray(H, dtype=np.float64)
    B, R = H.shape[:2]
    lhs = H.shape[2:]
    nd = len(ts)
    ls = tuple(lh + t - 1 for lh, t in zip(lhs, ts))
    out = np.zeros((B,) + ls + (R,) + tuple(ts))
    src = np.moveaxis(H, 1, -1)                                   # (B, *lhs, R)
    for t in itertools.product(*[range(k) for k in ts]):
        win = tuple(slice(td, td + n) for td, n in zip(t, lhs))
        out[(slice(None),) + win + (slice(None),) + t] = src
    return out.reshape(B * int(np.prod(ls)), R * int(np.prod(ts))) if nd else out


def fold(Y, B, R, lhs, ts, taps=None):
    """The adjoint of ``unfold`` (col2im): neg[b][r][j] = sum_t Y[(b, j + t)][(r, t)].  ``taps(r)``: the tap tuples summed
    for rank r (seeded faults), default all."""
    ls = tuple(lh + t - 1 for lh, t in zip(lhs, ts))
    Y = np.asarray(Y, dtype=np.float64).reshape((B,) + ls + (R,) + tuple(ts))
    out = np.zeros((B,) + tuple(lhs) + (R,))
    for t in itertools.product(*[range(k) for k in ts]):
        win = tuple(slice(td, td + n) for td, n in zip(t, lhs))
        part = Y[(slice(None),) + win + (slice(None),) + t]
        if taps is not None:
            part = part * np.array([1.0 if t in taps(r) else 0.0 for r in range(R)])
        out += part
    return np.moveaxis(out, -1, 1)


def target_w(V):
    """X_w[c][(b, l)] of V (B, C, *ls)."""
    V = np.asarray(V, dtype=np.float64)
    return np.moveaxis(V, 1, 0).reshape(V.shape[1], -1)


def w_matrix(W):
    W = np.asarray(W, dtype=np.float64)
    return W.reshape(W.shape[0], -1)


# ---- one half-step, in stages (the seeded-fault tests replace one stage's output) ------------------------------------
def operands(W, H, precision, rounding=True):
    """The operand images the GEMMs read: Wm (hi, lo), Hu (hi, lo) -- the unfold of the rounded H is the rounding of the
    unfold -- and the unrounded fp32 matrices (ragged channels in bf16x3, closed-form denominators)."""
    ts = tuple(W.shape[2:])
    Wx, Hx = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    if rounding:
        wh, wl = E.factor_image(Wx.ravel(), precision)
        hh, hl = E.factor_image(Hx.ravel(), precision)
        wh, hh = wh.reshape(Wx.shape), hh.reshape(Hx.shape)
        wl = None if wl is None else wl.reshape(Wx.shape)
        hl = None if hl is None else hl.reshape(Hx.shape)
    else:
        wh, wl, hh, hl = Wx, None, Hx, None
    return dict(Wm=(w_matrix(wh), None if wl is None else w_matrix(wl)),
                Hu=(unfold(hh, ts), None if hl is None else unfold(hl, ts)),
                Wx=w_matrix(Wx), Hux=unfold(Hx, ts), W=Wx, H=Hx, ts=ts, lhs=tuple(H.shape[2:]))


def reconstruction(ops, beta, exact_channels=()):
    """S[c][(b, l)] as the accumulators hold it: the plane products on top of eps (none at beta == 2); ``exact_channels``
    from the unrounded fp32 masters (conv_ragged_rows_kernel in bf16x3)."""
    (wh, wl), (hh, hl) = ops['Wm'], ops['Hu']
    S = E._gemm([wh] if wl is None else [wh, wl], hh.T, None if hl is None else hl.T)
    ex = list(exact_channels)
    if ex:
        S[ex] = ops['Wx'][ex] @ ops['Hux'].T
    return S if E.beta_kind(beta) == 'euc' else S + EPS


def ratio(Xw, ops, beta, precision, exact_channels=(), rounding=True, ratio_round=None):
    """Ratio planes of either half-step in the W half-step's orientation [c][(b, l)] (the H half-step writes the
    transpose of the same values: its GEMM forms the same three products).  dict: S, gn, gp (before rounding; gp None at
    beta == 1), gn_ops / gp_ops = [hi] or [hi, lo] as the numerator GEMM reads them, gn_flip / gp_flip = per element the
    distance of the two 16-bit neighbours where the rounding is ambiguous (single-plane modes), else 0."""
    S = reconstruction(ops, beta, exact_channels if rounding else ())
    gn, gp = E.mu_terms(S, np.asarray(Xw, dtype=np.float64), beta)
    out = dict(S=S, gn=gn, gp=gp, gp_ops=None, gn_flip=None, gp_flip=None)
    if not rounding:
        out['gn_ops'], out['gp_ops'] = [gn], (None if gp is None else [gp])
        return out
    split = precision == 'bf16x3'
    rr = ratio_round or (lambda G, sp: E.rounded_terms(G, precision, sp))
    for key, G in (('gn', gn), ('gp', gp)):
        if G is None:
            continue
        out[key + '_ops'] = rr(G, split)
        if not split:       # (a hi + lo pair holds the term to 2^-16 whichever way hi went)
            out[key + '_flip'] = np.abs(E.round_op(G * (1 + E.AMBIGUITY), precision).reshape(G.shape)
                                        - E.round_op(G * (1 - E.AMBIGUITY), precision).reshape(G.shape))
    for key in ('gn_ops', 'gp_ops'):
        if out[key] is not None:
            out[key] = [p.reshape(S.shape) for p in out[key]]
    return out


def with_device_planes(rt, planes, precision, transpose=False):
    """``rt`` (see ``ratio``) with the words the device wrote -- planes = {'gn': (hi, lo), 'gp': (hi, lo)} int16
    [rows_pad][cols_pad] in the half-step's own orientation -- as the numerator GEMM's operands.  ``check_ratio`` holds
    those words to the emulated rounding one by one; contracting THEM, and not the emulation's own choice among ambiguous
    neighbours, leaves nothing ambiguous in the numerators: no allowance.  (It matters in split bf16: the lo word is the
    rounding of a small difference and flips under a 1e-7 change of the term by up to 2^-16 of it, which a numerator that
    one frame dominates -- a batch's first or last frame is reconstructed by a single tap, so S can be tiny there --
    shows undiluted: 4e-6 .. 1.25e-5 on the MI355X against the emulation's own planes, 2e-7 against the device's.)"""
    out = dict(rt, gn_flip=None, gp_flip=None)
    for key in ('gn', 'gp'):
        if rt[key] is None or key not in planes:
            continue
        r, c = (rt[key].T if transpose else rt[key]).shape
        ops = [decode(b, 'bf16' if i else precision)[:r, :c] for i, b in enumerate(planes[key]) if b is not None]
        out[key + '_ops'] = [o.T for o in ops] if transpose else ops
    return out


def _contract(planes, flip, rhs, transpose):
    """(G rhs, allowance) with G = the ratio planes (transposed for the H half-step) and rhs = (hi, lo) operand planes."""
    if planes is None:
        return None, 0.0
    lhs = [p.T for p in planes] if transpose else planes
    res = E._gemm(lhs, rhs[0], rhs[1])
    amb = 0.0
    if flip is not None and flip.any():
        amb = (flip.T if transpose else flip) @ np.abs(rhs[0])
    return res, amb


def numerators_w(rt, ops, Hu=None):
    """num / den [c][(r, t)] of the W half-step (``Hu``: the planes the numerator GEMM reads, seeded faults)."""
    Hu = Hu or ops['Hu']
    num, na = _contract(rt['gn_ops'], rt['gn_flip'], Hu, False)
    den, da = _contract(rt['gp_ops'], rt['gp_flip'], Hu, False)
    return dict(num=num, den=den, num_amb=na, den_amb=da)


def numerators_h(rt, ops, B, taps=None):
    """The H half-step: Y / Yd [(b, l)][(r, t)] before the col2im sum, and the folded num / den (B, R, *lhs)."""
    R = ops['H'].shape[1]
    f = lambda y: None if y is None else fold(y, B, R, ops['lhs'], ops['ts'], taps)
    fa = lambda a: fold(a, B, R, ops['lhs'], ops['ts']) if isinstance(a, np.ndarray) else 0.0
    y, ya = _contract(rt['gn_ops'], rt['gn_flip'], ops['Wm'], True)
    yd, yda = _contract(rt['gp_ops'], rt['gp_flip'], ops['Wm'], True)
    return dict(y=y, yd=yd, y_amb=ya, yd_amb=yda, num=f(y), den=f(yd), num_amb=fa(ya), den_amb=fa(yda))


def _rank_last(x):
    """(.., R, ..) factor -> [everything else, R] view for mu_emulation.apply, and the inverse."""
    x = np.asarray(x, dtype=np.float64)
    m = np.moveaxis(x, 1, -1)
    return m.reshape(-1, x.shape[1]), (lambda y: np.moveaxis(np.asarray(y).reshape(m.shape), -1, 1))


def update(theta, nm, other, beta, gamma, l1=0.0, l2=0.0, kl_den=None):
    """The MU apply on a factor (C, R, *ts) or (B, R, *lhs) from num / den of the same shape; the beta == 1 denominator is
    the sum of the OTHER fp32 master over everything but the rank axis (``kl_den`` overrides it: seeded faults).
    Returns (new, allowance)."""
    shape = np.asarray(theta).shape
    th, back = _rank_last(theta)
    rs = lambda a: _rank_last(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(
        shape if np.ndim(a) else (1,) * len(shape)), shape))[0]
    num = rs(np.asarray(nm['num']).reshape(shape))
    den = None if nm['den'] is None else rs(np.asarray(nm['den']).reshape(shape))
    if kl_den is None and E.beta_kind(beta) == 'kl':
        o = np.asarray(other, dtype=np.float64)
        kl_den = o.sum(axis=tuple(i for i in range(o.ndim) if i != 1))
    new = E.apply(th, num, den, beta, gamma, l1, l2, kl_den=kl_den)
    na = rs(np.asarray(nm['num_amb']).reshape(shape)) if np.ndim(nm['num_amb']) else nm['num_amb']
    da = rs(np.asarray(nm['den_amb']).reshape(shape)) if np.ndim(nm['den_amb']) else nm['den_amb']
    allow = E.apply_allowance(new, num, den, na, da, beta, gamma, l1=l1, l2=l2, theta=th)
    return back(new), back(np.broadcast_to(allow, th.shape))


def gamma_of(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else (1.0 / (beta - 1.0) if beta > 2 else 1.0)


def w_half_step(V, W, H, beta, precision, l1=0.0, l2=0.0, exact_channels=(), rounding=True, ratio_round=None,
                Hu_num=None, kl_den=None, planes=None):
    """One W half-step from fp32 masters (``planes``: the ratio words read back from the device, see
    ``with_device_planes``).  dict: ratio (see ``ratio``), num, den, num_amb, den_amb [C][R T], new
    (C, R, *ts), allow."""
    ops = operands(W, H, precision, rounding)
    rt = ratio(target_w(V), ops, beta, precision, exact_channels, rounding, ratio_round)
    nm = numerators_w(rt if planes is None else with_device_planes(rt, planes, precision), ops, Hu_num)
    new, allow = update(W, nm, H, beta, gamma_of(beta), l1, l2, kl_den)
    return dict(nm, ratio=rt, new=new, allow=allow, ops=ops)


def h_half_step(V, W, H, beta, precision, l1=0.0, l2=0.0, exact_channels=(), rounding=True, ratio_round=None, taps=None,
                kl_den=None, planes=None):
    """One H half-step from fp32 masters.  dict: ratio ([c][(b, l)] orientation), y / yd [(b, l)][(r, t)], num / den
    (B, R, *lhs), new, allow."""
    ops = operands(W, H, precision, rounding)
    rt = ratio(target_w(V), ops, beta, precision, exact_channels, rounding, ratio_round)
    nm = numerators_h(rt if planes is None else with_device_planes(rt, planes, precision, True), ops, H.shape[0], taps)
    new, allow = update(H, nm, W, beta, gamma_of(beta), l1, l2, kl_den)
    return dict(nm, ratio=rt, new=new, allow=allow, ops=ops)


def loss(V, W, H, beta, precision, exact_channels=(), rounding=True):
    """(beta_div, sum of the absolute addends) as ``loss_elem`` (nmfmu_fused.h) forms it per element from the rounded
    operands and the fp32 target; the second figure scales the fp32 rounding error of the device's sum."""
    ops = operands(W, H, precision, rounding)
    s = reconstruction(ops, beta, exact_channels if rounding else ())
    x = target_w(V)
    kind = E.beta_kind(beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == 'euc':
            terms = [0.5 * (s - x) ** 2]
        elif kind == 'kl':
            terms = [x * (np.log(x + EPS) - np.log(s)), -x, s - EPS]
        elif kind == 'is':
            xe = x + EPS
            terms = [xe / s, -(np.log(xe) - np.log(s)), -np.ones_like(s)]
        else:
            xb = x + EPS if beta < 0 else x
            t1 = np.where(xb > 0, np.power(np.where(xb > 0, xb, 1.0), beta), 0.0)
            sb1 = np.power(s, beta - 1.0)
            d = beta * (beta - 1.0)
            terms = [t1 / d, (beta - 1.0) * sb1 * s / d, -beta * xb * sb1 / d]
    return float(sum(t.sum() for t in terms)), float(sum(np.abs(t).sum() for t in terms))


# fp32 rounding of one loss_elem: a handful of operations and two hardware transcendentals on addends that cancel; sixteen
# half-ulps of the absolute addends bound it with room (the sum over elements itself runs in fp32 per tile, then float64)
LOSS_ULPS = 16 * 2.0 ** -24


# ---- per-element checks (shared by the seeded-fault tests and the GPU test) ------------------------------------------
AMB_SHARE_MAX = 0.02     # condition of the plane check: at most this share of a plane's valid elements may be ambiguous


def plane_dtype(precision):
    return torch.float16 if precision == 'f16' else torch.bfloat16


def decode(bits, precision):
    """int16 words of a plane -> float64."""
    t = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.int16))
    return t.view(plane_dtype(precision)).double().numpy()


def encode(vals, precision):
    """float64 values that are representable in the plane's type -> int16 words."""
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64)).to(plane_dtype(precision))
    return t.view(torch.int16).numpy()


def nan_word(precision):
    return 0x7e00 if precision == 'f16' else 0x7fc0


def check_plane(bits, G, precision, kl, gemm_rows=None, transpose=False, lo_of=None):
    """One 16-bit ratio plane [rows_pad][cols_pad] (int16 words) against the unrounded term G [rows][cols].

    Every valid element equals the emulated rounding, or its rounding is ambiguous (flips inside the AMBIGUITY band) and
    it equals the other neighbour.  ``lo_of`` = the decoded hi plane of the same buffer set: the plane is the lo plane of
    bf16x3, lo = bf16(G - hi) with the hi the device wrote; G - hi is a small difference of two near-equal numbers, so the
    band of G is many ulps of lo wide and the word has to lie between the roundings of the band's two ends.
    Padding: ``gemm_rows`` channels (rows, or columns with ``transpose``; None = all) are covered by the reconstruction
    GEMM, which writes their padding with what x = 0 gives: finite, and zero at beta == 1.  Beyond them (ragged channels,
    the 64-row channel tile) the engine zero-initialises the planes once and nothing may write there: all-zero words.
    Returns dict(bad, amb_share, pad_bad)."""
    rows, cols = G.shape
    got = decode(bits, precision)
    v = got[:rows, :cols]
    a = E.AMBIGUITY
    if lo_of is None:
        want = E.round_op(G, precision).reshape(G.shape)
        n0 = E.round_op(G * (1 - a), precision).reshape(G.shape)
        n1 = E.round_op(G * (1 + a), precision).reshape(G.shape)
        amb = n0 != n1
        ok = (v == want) | (amb & ((v == n0) | (v == n1)))
        share = float(amb.mean())
    else:
        hi = lo_of[:rows, :cols]
        n0 = E.round_bf16(G * (1 - a) - hi).reshape(G.shape)
        n1 = E.round_bf16(G * (1 + a) - hi).reshape(G.shape)
        ok = (v >= np.minimum(n0, n1)) & (v <= np.maximum(n0, n1))
        share = 0.0          # (judged on the hi plane)
    pad = np.ones(got.shape, dtype=bool)
    pad[:rows, :cols] = False
    untouched = np.zeros(got.shape, dtype=bool)
    if gemm_rows is not None:
        if transpose:
            untouched[:, gemm_rows:] = True
        else:
            untouched[gemm_rows:] = True
    written = got[pad & ~untouched]
    pad_bad = int((np.asarray(bits)[pad & untouched] != 0).sum())
    pad_bad += int((written != 0).sum()) if kl else int((~np.isfinite(written)).sum())
    return dict(bad=int((~ok).sum()), amb_share=share, pad_bad=pad_bad)


def planes_of(rt, key, precision, rows_pad, cols_pad, transpose=False):
    """The emulated ratio planes as the device stores them: int16 [rows_pad][cols_pad] (hi, lo or None), zero padding."""
    out = []
    for p in rt[key + '_ops']:
        p = p.T if transpose else p
        full = np.zeros((rows_pad, cols_pad), dtype=np.int16)
        full[:p.shape[0], :p.shape[1]] = encode(p, precision)
        out.append(full)
    return out[0], (out[1] if len(out) > 1 else None)


def check_ratio(planes, rt, precision, beta, gemm_rows=None, transpose=False):
    """All ratio planes of one half-step: planes = {'gn': (hi, lo), 'gp': (hi, lo)} int16 [rows_pad][cols_pad]."""
    kl = E.beta_kind(beta) == 'kl'
    res = {}
    for key in ('gn', 'gp'):
        if rt[key] is None or key not in planes:
            continue
        G = rt[key].T if transpose else rt[key]
        hi, lo = planes[key]
        res[key] = check_plane(hi, G, precision, kl, gemm_rows, transpose)
        if lo is not None:
            res[key + '_lo'] = check_plane(lo, G, 'bf16', kl, gemm_rows, transpose, lo_of=decode(hi, 'bf16'))
    return res


def ratio_ok(res):
    return all(r['bad'] == 0 and r['pad_bad'] == 0 and r['amb_share'] <= AMB_SHARE_MAX for r in res.values())


def _cols(x):
    """elem_err scales near-zero entries by their column's largest reference: factors go in rank-last."""
    x = np.asarray(x, dtype=np.float64)
    return _rank_last(x)[0] if x.ndim > 2 else x


def value_err(got, ref, allow=0.0):
    """(max per-element error after the ambiguity allowance, raw max)."""
    a = _cols(np.broadcast_to(allow, np.shape(ref))) if np.ndim(allow) else allow
    return float(E.elem_err(_cols(got), _cols(ref), a).max()), float(E.elem_err(_cols(got), _cols(ref)).max())


def check_half_step(got, em, precision, beta, which, gemm_rows=None, tol=None):
    """The per-element check of one half-step.  ``got``: what the device (or a faulty emulation) produced -- 'planes'
    (see check_ratio), optionally 'num' / 'den' (W: [C][R T]; H: the folded (B, R, *lhs)) and 'y' / 'yd', and 'new'.
    Returns (ok, figures)."""
    tol = E.TOL[precision] if tol is None else tol
    fig = {'ratio': check_ratio(got['planes'], em['ratio'], precision, beta, gemm_rows, transpose=(which == 'h'))}
    ok = ratio_ok(fig['ratio'])
    # a silent channel (W row all zero) has S = eps, ratios and numerators 1e7 times the others': judged on its own, or
    # elem_err's floor (1e-6 of the column's largest reference) would hide every other row of num_w / den_w
    silent = ~np.asarray(em['ops']['Wx']).any(axis=1) if which == 'w' else None
    for key, amb in (('num', 'num_amb'), ('den', 'den_amb'), ('y', 'y_amb'), ('yd', 'yd_amb')):
        if got.get(key) is not None and em.get(key) is not None:
            groups = [slice(None)]
            if silent is not None and key in ('num', 'den') and silent.any() and not silent.all():
                groups = [silent, ~silent]
            errs = [value_err(np.asarray(got[key])[g], np.asarray(em[key])[g],
                              em[amb][g] if np.ndim(em[amb]) else em[amb]) for g in groups]
            fig[key], fig[key + '_raw'] = max(e[0] for e in errs), max(e[1] for e in errs)
            ok = ok and fig[key] <= tol
    fig['master'], fig['master_raw'] = value_err(got['new'], em['new'], em['allow'])
    zero = np.asarray(em['new']) == 0
    fig['zeros_kept'] = bool((np.asarray(got['new'])[zero] == 0).all())
    return bool(ok and fig['master'] <= tol and fig['zeros_kept']), fig


def as_kernel_result(em, precision, which, rows_pad, cols_pad):
    """An emulated half-step in the form ``check_half_step`` takes from the device (the seeded-fault tests start here)."""
    tr = which == 'h'
    planes = {'gn': planes_of(em['ratio'], 'gn', precision, rows_pad, cols_pad, tr)}
    if em['ratio']['gp'] is not None:
        planes['gp'] = planes_of(em['ratio'], 'gp', precision, rows_pad, cols_pad, tr)
    return dict(planes=planes, num=em['num'], den=em['den'], y=em.get('y'), yd=em.get('yd'), new=em['new'])


# ---- reference-side error of the fp32 accumulation (the only ground for raising a case's tolerance) -----------------
def fp32_order_error(lhs_planes, rhs, ref):
    """Largest per-element difference to the float64 product ``ref`` of the same contraction accumulated in numpy
    float32, in k-chunks of 16, ascending and descending (what summation order alone can do; the MFMA's internal order
    is not reproduced)."""
    worst = 0.0
    K = rhs[0].shape[0]
    prods = [(lhs_planes[0], rhs[0])]
    if len(lhs_planes) == 2:
        prods += [(lhs_planes[1], rhs[0])] + ([(lhs_planes[0], rhs[1])] if rhs[1] is not None else [])
    for order in (1, -1):
        acc = np.zeros(ref.shape, dtype=np.float32)
        for k0 in list(range(0, K, 16))[::order]:
            for a, b in prods:
                acc = acc + (a[:, k0:k0 + 16].astype(np.float32) @ b[k0:k0 + 16].astype(np.float32))
        worst = max(worst, float(E.elem_err(acc.astype(np.float64), ref).max()))
    return worst


# ---- ConvMU's path selection for a case -------------------------------------------------------------------------------
def plan(case, ncu):
    """The control flow ConvMU takes for a case on ``ncu`` CUs: nmfd_engine.plan_conv, the function the engine itself
    plans with, on the case's sizes and switches alone (the library's static predicates run on the host), as a dict of the
    plan's fields plus ``h_tail`` = (rows, split).  The GPU test asserts that the engine built for the case carries it."""
    import dataclasses
    from torchnmf_amd import _capi, nmfd_engine as N
    p = dataclasses.asdict(N.plan_conv(_capi.load(), case['B'], case['C'], case['ls'], case['R'], case['ts'], case['beta'],
                                       ncu=ncu, env=case['env']))
    return dict(p, h_tail=(p['h_tail_rows'], p['h_tail_split']))


def signature(p):
    """What a plan (a ConvPlan as a dict) decides, without sizes, contraction splits and beta: (shift axes, implicit, H path,
    ragged channels, c_rows, fused_sums, fused_tables, rows_fused, wk_fold).  test_conv_emulation.py holds the plans of a
    default-switch grid against the case list by it."""
    h_path = 'fold_parts' if p['fold_parts'] else 'h_rows' if p['h_rows'] else 'store_y'
    rag = 'in_grid' if p['ragged_in_grid'] else 'ragged' if p['ragged'] else None
    return (p['nd'], bool(p['implicit']), h_path, rag, p['c_rows'], bool(p['fused_sums']), bool(p['fused_tables']),
            bool(p['rows_fused']), p['wk_fold'])


def claim_holds(claim, p, case):
    """Does the plan reach the control flow ``claim`` names?  A claim is 'flag' (truthy), '!flag' (falsy) or 'flag=value'."""
    if '=' in claim:
        k, v = claim.split('=')
        return str(p[k]) == v
    if claim.startswith('!'):
        return not p[claim[1:]]
    if claim == 'tail_split':
        return p['h_tail'][0] > 0 and p['h_tail'][1] > 1
    if claim == 'h_ksplit>1':
        return p['h_ksplit'] is not None and p['h_ksplit'] > 1
    if claim == 'rank_in_ktile':         # a rank boundary inside a 64-wide k-tile: T / 8 odd
        return p['T'] % 8 == 0 and (p['T'] // 8) % 2 == 1
    if claim == 'batch_in_tile':         # a batch boundary inside a 128-row tile
        return case['B'] > 1 and p['L'] % 128 != 0
    return bool(p[claim])


# Claims only a launch can answer (asserted on the GPU): staged[...].
def conv_cases():
    """The case list of tests/test_gpu_conv_emulated_parity.py.  Each case: shapes, precision, beta, environment switches,
    regularisation, the control-flow claims it is there for (checked against ``plan`` on the CPU and against the engine on
    the GPU), the launches that must (1) or must not (0) stage their implicit operand as a window, whether the case runs
    through WideRankMU, and ``tol_x`` -- the factor on mu_emulation.TOL, 1 unless a reference-side figure is written
    beside the case."""
    cases = []

    def add(tag, B, C, ls, R, ts, prec, beta, claims, env=None, regs=(0.0, 0.0), staged=None, wide=False, zeros=True):
        env = {('TORCHNMF_AMD_NMFD_' + k): v for k, v in (env or {}).items()}
        ls, ts = (ls,) if isinstance(ls, int) else tuple(ls), (ts,) if isinstance(ts, int) else tuple(ts)
        # (beta = -1 with a silent channel: S = eps there and the generic branch's exp2(-2 log2 eps) carries 1 ulp of a
        # logarithm of magnitude 23 -- 2e-6 relative, the whole AMBIGUITY band; the zeros are checked at the other betas)
        zeros = zeros and beta != -1
        cid = f'{tag}-{prec}-b{beta:g}' + ('-reg' if regs != (0.0, 0.0) else '')
        cases.append(dict(id=cid, B=B, C=C, ls=ls, R=R, ts=ts, precision=prec, beta=float(beta), claims=tuple(claims),
                          env=env, regs=regs, staged=staged or {}, wide=wide, zeros=zeros, tol_x=1.0))

    ALL = [('bf16x3', 1), ('bf16x3', 2), ('bf16x3', 0.5), ('bf16x3', 0), ('bf16', 1.5), ('bf16', -1), ('bf16', 1)]
    REG = (0.05, 0.05)
    # explicit planes: T or L not a multiple of 8; store-then-fold where the window-operand path is switched off
    for i, (prec, beta) in enumerate(ALL):
        add('explicit-T5', 2, 70, 61, 6, 5, prec, beta, ('!implicit', 'h_rows', '!fold_parts', 'batch_in_tile'),
            regs=REG if i % 2 else (0.0, 0.0))
    add('explicit-L-odd', 1, 130, 203, 3, 16, 'bf16x3', 1, ('!implicit', 'ragged', '!ragged_in_grid', 'h_rows'))
    add('explicit-fold', 2, 40, 50, 5, 6, 'bf16x3', 0.5, ('!implicit', '!h_rows', '!fold_parts'), env={'H_ROWS': '0'})
    add('explicit-fold', 2, 40, 50, 5, 6, 'bf16', 1, ('!implicit', '!h_rows', '!fold_parts'), env={'H_ROWS': '0'}, regs=REG)
    add('explicit-fold2d', 1, 20, (14, 19), 3, (3, 4), 'bf16x3', 1, ('!implicit', '!h_rows'), env={'H_ROWS': '0'})
    add('explicit-fold2d', 1, 20, (14, 19), 3, (3, 4), 'bf16', 2, ('!implicit', '!h_rows'), env={'H_ROWS': '0'})
    # T = 1 through WideRankMU (rank above 256): V (N, C) becomes (1, C, N), W (C, R, 1)
    add('wide-r300', 1, 90, 150, 300, 1, 'bf16x3', 1, ('!implicit', '!h_rows', '!fold_parts'), wide=True)
    add('wide-r300', 1, 90, 150, 300, 1, 'bf16', 2, ('!implicit', '!h_rows', '!fold_parts'), wide=True, regs=REG)
    add('wide-r300', 1, 90, 150, 300, 1, 'bf16x3', 0.5, ('!implicit', '!h_rows', '!fold_parts'), wide=True)
    # implicit tables: chunk-major and window-staged; T / 8 odd puts rank boundaries inside k-tiles, B > 1 with L % 128
    # != 0 puts batch boundaries inside tiles
    for prec, beta in (('bf16x3', 1), ('bf16', 2), ('bf16x3', 0), ('f16', 1)):
        add('implicit-T24', 2, 70, 200, 5, 24, prec, beta, ('implicit', 'h_rows', 'rank_in_ktile', 'batch_in_tile', '!rows_fused'),
            staged=dict(recon_w=0, recon_h=0))
    for prec, beta in (('bf16x3', 1), ('bf16', 1), ('f16', 1), ('bf16x3', 1.5)):
        add('staged-T72', 1, 140, 256, 8, 72, prec, beta, ('implicit', 'h_rows', 'rank_in_ktile') + (('rows_fused',) if beta == 1 else ()),
            staged=dict(recon_w=1, recon_h=1))
        add('chunk-T72', 1, 140, 256, 8, 72, prec, beta, ('implicit', 'h_rows', 'rank_in_ktile'), env={'WINSTAGE': '0'},
            staged=dict(recon_w=0, recon_h=0))
    # fold-parts (T >= 128): fused sums + fused tables, and each switched off; B > 1; forced tail-round split; T = 136 has
    # rank boundaries inside k-tiles; every beta of the unfused fold-parts kernel
    for prec in ('bf16x3', 'bf16', 'f16'):
        add('fold-T128', 2, 70, 256, 2, 128, prec, 1, ('fold_parts', 'fused_sums', 'fused_tables', 'w_ksplit=1'),
            regs=REG if prec == 'bf16' else (0.0, 0.0))
        add('fold-T136-tail', 1, 129, 264, 3, 136, prec, 1, ('fold_parts', 'fused_tables', 'tail_split', 'ragged', 'rank_in_ktile'),
            env={'TAIL_SPLIT': '2,2'})
        add('fold-T128-notables', 2, 70, 256, 2, 128, prec, 1, ('fold_parts', 'fused_sums', '!fused_tables'), env={'FUSED_TABLES': '0'})
    add('fold-T128-nosums', 2, 70, 256, 2, 128, 'bf16x3', 1, ('fold_parts', '!fused_sums', '!fused_tables'), env={'FUSED_SUMS': '0'})
    add('fold-T128-nosums', 2, 70, 256, 2, 128, 'bf16', 1, ('fold_parts', '!fused_sums'), env={'FUSED_SUMS': '0'}, regs=REG)
    for prec, beta in (('bf16x3', 2), ('bf16x3', 0.5), ('bf16', 0), ('bf16', 1.5), ('bf16x3', -1)):
        add('fold-T128', 2, 70, 256, 2, 128, prec, beta, ('fold_parts', '!fused_sums'))
    add('fold-T400', 1, 40, 640, 2, 400, 'bf16x3', 1, ('fold_parts', 'fused_tables'))
    add('fold-T400', 1, 40, 640, 2, 400, 'f16', 1, ('fold_parts', 'fused_tables'))
    for prec in ('bf16x3', 'f16'):
        add('fold-ksplit2', 2, 70, 1024, 2, 128, prec, 1, ('fold_parts', 'fused_sums', 'w_ksplit=2'),
            staged=dict(recon_w=1, recon_h=1))
    # window-operand H numerator: tap folds 1 / 2 / 4, split contraction, rows_fused on and off, R not a power of two,
    # two and three shift axes, the 64-row channel tile
    add('rows-fold4', 1, 200, 128, 6, 16, 'bf16x3', 1, ('h_rows', 'wk_fold=4', 'h_ksplit>1', '!rows_fused'))
    add('rows-fold4', 1, 200, 128, 6, 16, 'bf16', 0.5, ('h_rows', 'wk_fold=4', 'h_ksplit>1'))
    add('rows-fold2', 1, 100, 128, 11, 64, 'bf16x3', 1, ('h_rows', 'wk_fold=2', 'rows_fused'))
    add('rows-fold2', 1, 100, 128, 11, 64, 'f16', 1, ('h_rows', 'wk_fold=2', 'rows_fused'), regs=REG)
    add('rows-fold2-unfused', 1, 100, 128, 11, 64, 'bf16x3', 1, ('h_rows', 'wk_fold=2', '!rows_fused'), env={'ROWS_FUSED': '0'})
    add('rows-fold1', 2, 70, 96, 40, 8, 'bf16x3', 1, ('h_rows', 'wk_fold=1', '!rows_fused', 'batch_in_tile'))
    add('rows-fold1', 2, 70, 96, 40, 8, 'bf16', 2, ('h_rows', 'wk_fold=1'))
    add('rows-fold1', 2, 70, 96, 40, 8, 'bf16', 0, ('h_rows', 'wk_fold=1'), regs=REG)
    for prec, beta in (('bf16x3', 1), ('f16', 1), ('bf16', 1.5), ('bf16x3', -1)):
        add('rows-2d-narrow', 2, 20, (30, 40), 3, (8, 8), prec, beta,
            ('implicit', 'h_rows', 'c_rows', 'wk_fold=4') + (('rows_fused',) if beta == 1 else ()))
    add('rows-2d', 1, 70, (18, 24), 5, (3, 8), 'bf16x3', 1, ('implicit', 'h_rows', '!c_rows', 'wk_fold=4', '!rows_fused'))
    add('rows-2d', 1, 70, (18, 24), 5, (3, 8), 'bf16', 2, ('implicit', 'h_rows', '!c_rows'), regs=REG)
    add('rows-3d', 1, 20, (6, 9, 16), 3, (2, 3, 8), 'bf16x3', 1, ('implicit', 'h_rows', 'c_rows', '!rows_fused'))
    add('rows-3d', 1, 20, (6, 9, 16), 3, (2, 3, 8), 'f16', 1, ('implicit', 'h_rows', 'c_rows'))
    add('rows-3d', 1, 20, (6, 9, 16), 3, (2, 3, 8), 'bf16', 0.5, ('implicit', 'h_rows', 'c_rows'))
    # ragged channels (C = 128 k + 1, 2, 8) through the separate kernel: both half-steps and the loss, every beta branch
    for extra, (prec, beta) in zip((1, 2, 8, 1, 2, 8, 1), ALL):
        add(f'ragged{extra}', 1, 128 + extra, 136, 3, 16, prec, beta, ('ragged', '!ragged_in_grid', 'implicit', 'h_rows'))
    add('ragged2', 1, 130, 136, 3, 16, 'f16', 1, ('ragged', '!ragged_in_grid', 'implicit'))
    # ... and in-grid (one extra 16 x 16 MFMA block per workgroup of the staged reconstruction GEMMs)
    for prec, beta in (('bf16x3', 1), ('f16', 1), ('bf16', 2), ('bf16x3', 0.5)):
        add('ragged-in-grid', 1, 1025, 1024, 2, 128, prec, beta, ('ragged', 'ragged_in_grid', 'fold_parts'),
            staged=dict(recon_w=1, recon_h=1, num_w=1))
    # ---- the plans the default switches reach on small shapes and the cases above do not: one case or more per signature
    # (``signature``; test_conv_emulation.py holds the list against a grid of default plans).  Per (shift axes, operand
    # form, H path): beta 1, 2 and a third, split and single bf16, 'f16' where the plan admits it; rows_fused is beta == 1.
    EXP, ROWS = ('!implicit', 'h_rows'), ('implicit', 'h_rows')
    fold = lambda f: ('wk_fold=%d' % f,)
    # one shift axis.  Explicit planes with the window-operand numerator: tap folds 2 / 4, ragged channels at folds 1 / 2
    add('explicit-fold2', 2, 20, 50, 2, 6, 'bf16x3', 1, EXP + fold(2) + ('!ragged', 'batch_in_tile'))
    add('explicit-fold4', 1, 20, 203, 2, 16, 'bf16', 2, EXP + fold(4) + ('!ragged',))
    add('explicit-ragged-fold1', 1, 129, 61, 2, 5, 'bf16x3', 0.5, EXP + fold(1) + ('ragged', '!ragged_in_grid'))
    add('explicit-ragged-fold2', 1, 129, 50, 2, 6, 'bf16', 1, EXP + fold(2) + ('ragged', '!ragged_in_grid'))
    add('explicit-ragged-fold2', 1, 129, 50, 2, 6, 'bf16x3', 2, EXP + fold(2) + ('ragged', '!ragged_in_grid'), regs=REG)
    # the unfused fold-parts kernel beside a ragged channel (beta == 1: with the fused sums switched off)
    FRAG = ('implicit', 'fold_parts', '!fused_sums', '!fused_tables', 'ragged', '!ragged_in_grid')
    add('fold-ragged-unfused', 1, 129, 256, 2, 128, 'bf16x3', 2, FRAG)
    add('fold-ragged-unfused', 1, 129, 256, 2, 128, 'bf16', 1.5, FRAG)
    add('fold-ragged-unfused', 1, 129, 256, 2, 128, 'bf16x3', 1, FRAG, env={'FUSED_SUMS': '0'}, regs=REG)
    # window tables with the window-operand numerator: rows_fused at fold 1; ragged channels at folds 1 / 2 (8 taps) and,
    # with rows_fused, at folds 1 / 2 / 4 (64 taps)
    add('rows-fused-fold1', 1, 20, 128, 40, 64, 'bf16x3', 1, ROWS + fold(1) + ('rows_fused', '!ragged'))
    add('rows-ragged-fold1', 1, 129, 96, 40, 8, 'bf16x3', 2, ROWS + fold(1) + ('ragged', '!rows_fused'))
    add('rows-ragged-fold1', 1, 129, 96, 40, 8, 'bf16', 1, ROWS + fold(1) + ('ragged', '!rows_fused'), regs=REG)
    add('rows-ragged-fold2', 1, 129, 96, 11, 8, 'bf16', 1.5, ROWS + fold(2) + ('ragged', '!rows_fused'))
    add('rows-ragged-fold2', 1, 129, 96, 11, 8, 'f16', 1, ROWS + fold(2) + ('ragged', '!rows_fused'))
    add('rows-ragged-fused-fold1', 1, 129, 128, 40, 64, 'bf16x3', 1, ROWS + fold(1) + ('ragged', 'rows_fused'), regs=REG)
    add('rows-ragged-fused-fold2', 1, 129, 128, 11, 64, 'bf16', 1, ROWS + fold(2) + ('ragged', 'rows_fused'))
    add('rows-ragged-fused-fold4', 1, 129, 128, 2, 64, 'f16', 1, ROWS + fold(4) + ('ragged', 'rows_fused'))
    # two shift axes.  Explicit planes (last axis no multiple of 8) with the window-operand numerator: folds 1 / 2 / 4
    add('explicit-2d-fold1', 2, 20, (12, 31), 2, (2, 5), 'bf16x3', 1, EXP + fold(1) + ('!c_rows', 'batch_in_tile'))
    add('explicit-2d-fold1', 2, 20, (12, 31), 2, (2, 5), 'bf16', 0.5, EXP + fold(1) + ('!c_rows', 'batch_in_tile'), regs=REG)
    add('explicit-2d-fold2', 1, 20, (14, 19), 11, (3, 4), 'bf16', 2, EXP + fold(2) + ('!c_rows',))
    add('explicit-2d-fold4', 1, 20, (14, 19), 2, (3, 4), 'bf16x3', 2, EXP + fold(4) + ('!c_rows',), regs=REG)
    # window tables: the 128-row and the 64-row channel tile at folds 1 / 2 (24 taps) and with rows_fused (64 taps)
    add('rows-2d-fold1', 1, 70, (18, 24), 40, (3, 8), 'bf16x3', 2, ROWS + fold(1) + ('!c_rows', '!rows_fused'))
    add('rows-2d-fold1', 1, 70, (18, 24), 40, (3, 8), 'f16', 1, ROWS + fold(1) + ('!c_rows', '!rows_fused'))
    add('rows-2d-fold2', 1, 70, (18, 24), 11, (3, 8), 'bf16', 0.5, ROWS + fold(2) + ('!c_rows', '!rows_fused'), regs=REG)
    add('rows-2d-fused-fold1', 1, 70, (30, 40), 40, (8, 8), 'bf16', 1, ROWS + fold(1) + ('!c_rows', 'rows_fused'))
    add('rows-2d-fused-fold2', 1, 70, (30, 40), 11, (8, 8), 'bf16x3', 1, ROWS + fold(2) + ('!c_rows', 'rows_fused'))
    add('rows-2d-fused-fold4', 1, 70, (30, 40), 2, (8, 8), 'f16', 1, ROWS + fold(4) + ('!c_rows', 'rows_fused'), regs=REG)
    add('rows-2d-narrow-fold1', 1, 20, (18, 24), 40, (3, 8), 'bf16', 1, ROWS + fold(1) + ('c_rows', '!rows_fused'))
    add('rows-2d-narrow-fold2', 1, 20, (18, 24), 11, (3, 8), 'bf16x3', 1.5, ROWS + fold(2) + ('c_rows', '!rows_fused'))
    add('rows-2d-narrow-fused-fold1', 1, 20, (30, 40), 40, (8, 8), 'bf16x3', 1, ROWS + fold(1) + ('c_rows', 'rows_fused'), regs=REG)
    add('rows-2d-narrow-fused-fold2', 1, 20, (30, 40), 11, (8, 8), 'bf16', 1, ROWS + fold(2) + ('c_rows', 'rows_fused'))
    # three shift axes.  Explicit planes: folds 1 / 2, and fold 4 with a middle tap axis of extent 1
    add('explicit-3d-fold1', 1, 20, (5, 7, 9), 40, (2, 3, 2), 'bf16', 2, EXP + fold(1) + ('!c_rows',))
    add('explicit-3d-fold2', 2, 20, (5, 7, 9), 2, (2, 3, 2), 'bf16x3', 1, EXP + fold(2) + ('!c_rows', 'batch_in_tile'), regs=REG)
    add('explicit-3d-fold2', 2, 20, (5, 7, 9), 2, (2, 3, 2), 'bf16', 1.5, EXP + fold(2) + ('!c_rows', 'batch_in_tile'))
    add('explicit-3d-fold4', 1, 20, (4, 5, 11), 2, (2, 1, 4), 'bf16x3', 2, EXP + fold(4) + ('!c_rows',), regs=REG)
    # window tables: both channel tiles at folds 1 / 2 / 4 (48 taps) and with rows_fused (64 taps)
    add('rows-3d-wide-fold1', 1, 70, (6, 9, 16), 40, (2, 3, 8), 'bf16x3', 1, ROWS + fold(1) + ('!c_rows', '!rows_fused'))
    add('rows-3d-wide-fold2', 1, 70, (6, 9, 16), 11, (2, 3, 8), 'bf16', 2, ROWS + fold(2) + ('!c_rows', '!rows_fused'))
    add('rows-3d-wide-fold4', 1, 70, (6, 9, 16), 2, (2, 3, 8), 'f16', 1, ROWS + fold(4) + ('!c_rows', '!rows_fused'), regs=REG)
    add('rows-3d-wide-fused-fold1', 1, 70, (5, 6, 32), 40, (2, 2, 16), 'bf16', 1, ROWS + fold(1) + ('!c_rows', 'rows_fused'))
    add('rows-3d-wide-fused-fold2', 1, 70, (5, 6, 32), 11, (2, 2, 16), 'f16', 1, ROWS + fold(2) + ('!c_rows', 'rows_fused'))
    add('rows-3d-wide-fused-fold4', 1, 70, (5, 6, 32), 2, (2, 2, 16), 'bf16x3', 1, ROWS + fold(4) + ('!c_rows', 'rows_fused'), regs=REG)
    # (the third beta of this rank-40 case in split bf16 is 1.5, not 0: the lo-word check holds a term to AMBIGUITY = 2e-6,
    # and S summed in fp32 over its 3 x 1920 products differs from the float64 sum by 1.2e-6 on the reference side alone
    # (numpy float32, k-chunks of 16, either order), which Gn = x S^(beta - 2) doubles at beta == 0: 2.3e-6 before the
    # device's reciprocal, 2.3 .. 2.6e-6 in 10 of 17 280 words on the MI355X, one each in ten channels.  At beta == 1.5 the
    # exponent is -0.5 and no word leaves the band.)
    add('rows-3d-fold1', 1, 20, (6, 9, 16), 40, (2, 3, 8), 'bf16x3', 1.5, ROWS + fold(1) + ('c_rows', '!rows_fused'))
    add('rows-3d-fold2', 1, 20, (6, 9, 16), 11, (2, 3, 8), 'bf16', 1, ROWS + fold(2) + ('c_rows', '!rows_fused'))
    add('rows-3d-fused-fold1', 1, 20, (5, 6, 32), 40, (2, 2, 16), 'bf16x3', 1, ROWS + fold(1) + ('c_rows', 'rows_fused'), regs=REG)
    add('rows-3d-fused-fold2', 1, 20, (5, 6, 32), 11, (2, 2, 16), 'bf16', 1, ROWS + fold(2) + ('c_rows', 'rows_fused'))
    add('rows-3d-fused-fold4', 1, 20, (5, 6, 32), 2, (2, 2, 16), 'f16', 1, ROWS + fold(4) + ('c_rows', 'rows_fused'))
    return cases


def make_problem(case):
    """(V, W0, H0) fp32 on the CPU: rand + 1e-3 targets and |randn| factors as the NMFD tests use; one silent channel and
    one silent rank segment of H where the case asks for zeros."""
    B, C, R, ts, ls = case['B'], case['C'], case['R'], case['ts'], case['ls']
    lhs = tuple(l - t + 1 for l, t in zip(ls, ts))
    g = torch.Generator().manual_seed((B * 7 + C * 3 + R * 11 + int(np.prod(ls))) % 100003)
    V = torch.rand(B, C, *ls, generator=g) + 1e-3
    W0 = torch.randn(C, R, *ts, generator=g).abs()
    H0 = torch.randn(B, R, *lhs, generator=g).abs()
    if case['zeros']:
        W0[3] = 0.0
        H0[0, R - 1].reshape(-1)[: max(1, H0[0, R - 1].numel() // 3)] = 0.0
    return V, W0, H0
