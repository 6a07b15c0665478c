"""Float64 reference of ``separation.separate`` (csrc/nmfmu_separate.hip), test-only, plain numpy on the CPU.

The host tables are restated in plain Python (``normalise``, ``tables``, ``slots``); ``Y_g``, ``D``, the masks and the outputs are
formed in float64 from the ORIGINAL factors, unpermuted, so the permutation and padding of the fused route are checked and not
assumed.  ``D`` is the float64 sum of the ``Y_g^p`` for every power: at ``p == 1`` the kernels use the one reconstruction over all
components instead, which is the same number, and the bound below carries that reconstruction's own error.

What separates a kernel from this module is fp32 arithmetic alone, and every element is held to the first-order bound the
standard model gives for the operations the kernel performs on it (Higham, Accuracy and Stability of Numerical Algorithms,
ch. 3: every operation one relative rounding u = 2^-24).  No bound is taken from a run.  From the kernel source:

* ``y_g``: an fp32 dot product of the group's ``R_g`` components (the zero column that pads a group adds exactly nothing):
  ``(R_g + 2) u |H_g| |W_g|^T``, as tests/forward_reference.py, whatever the order.  A convolutive plane comes from
  ``nmfd_engine.reconstruct``: forward_reference's tier-2 bound ``(3 * 2^-16 + (3 K_g + 2) u) bound64``, ``K_g = R_g prod(T)``.
  A plane that is GIVEN (the planes kernel on its own) has no error.
* ``y^p``: ``p == 1`` nothing; ``p == 2`` one multiplication (in a sum it enters by one fused multiply-add: no more than that); otherwise ``exp2f(p * log2f(y))``, counted as
  tests/weighted_emulation.py counts it with its ``ULP_FN``: the relative error e of y moves the result by p e; log2f adds
  ``ULP_FN u |L|`` and the product p L one rounding, an absolute error d of the exponent moves exp2 by ``d ln 2`` relative, and
  exp2f adds ``ULP_FN u``.
* ``D``: ``p != 1``: the errors of its terms and ``G - 1`` additions, each at most ``u D`` (all partial sums are below ``D``:
  the terms are non-negative); ``p == 1``: the error of the full reconstruction, ``(R + 2) u |H| |W|^T`` (tier 2 with
  ``K = R prod(T)`` for a convolutive model).
* ``+ eps``: one rounding.
* the division: fp32 ``/`` compiles to the correctly rounded division sequence (v_div_scale / v_div_fmas / v_div_fixup): one
  rounding.
* the multiplication by ``v``: one rounding per part.

``SECOND_ORDER`` covers the products of these terms the first-order count drops: the largest first-order relative term here
is below 2e-4 (rank 256, p = 2), so they are below 1e-3 of the bound.  Results below the normal range round to a multiple of
2^-149 instead of relatively; ``TINY`` per element covers a few hundred such roundings and is far below every value these
tests produce.  The factors are taken to be non-negative (negative ``y`` under a fractional power is NaN in the kernel and is
not modelled).
"""
from __future__ import annotations

import numpy as np

import forward_reference as FR
import weighted_emulation as WE

U = FR.U
ULP_FN = WE.ULP_FN
LN2 = WE.LN2
EPS = 2.0 ** -23                 # constants.eps
SECOND_ORDER = 1.001
TINY = 2.0 ** -140


# ---- the host tables, as plain Python ------------------------------------------------------------------------------------------
def normalise(groups, R):
    return list(range(R)) if groups is None else [int(g) for g in groups]


def tables(labels):
    """(G, members, cols, gstart): see ``separation.group_tables``."""
    G = max(labels) + 1
    members = [[r for r, lab in enumerate(labels) if lab == g] for g in range(G)]
    cols, gstart = [], [0]
    for m in members:
        cols += m + ([-1] if len(m) % 2 else [])
        gstart.append(len(cols))
    return G, members, cols, gstart


def slots(G, select):
    """(slot [G], S, copies): see ``separation.slot_table``."""
    if select is None:
        return list(range(G)), G, []
    slot, copies = [-1] * G, []
    for s, g in enumerate(select):
        if slot[g] < 0:
            slot[g] = s
        else:
            copies.append((s, slot[g]))
    return slot, len(select), copies


def permuted(F, cols):
    """The factor with its rank axis (axis 1) permuted and padded as the fused route does, by plain indexing."""
    F = np.asarray(F)
    out = np.zeros((F.shape[0], len(cols)) + F.shape[2:], dtype=F.dtype)
    for k, c in enumerate(cols):
        if c >= 0:
            out[:, k] = F[:, c]
    return out


# ---- reconstructions -------------------------------------------------------------------------------------------------------------
def _recon64(H, W):
    """(float64 reconstruction, the same contraction of |H| and |W|, terms per element K, whether convolutive)."""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    if W.ndim == 2:
        return H @ W.T, np.abs(H) @ np.abs(W).T, W.shape[1], False
    return FR._conv64(H, W), FR._conv64(np.abs(H), np.abs(W)), FR.conv_k(W), True


def plane_error(bound64, K, conv):
    """The bound of |fp32 plane - float64 plane|."""
    return ((FR.U_BF16X3 + (3 * K + 2) * U) if conv else (K + 2) * U) * bound64


def group_planes(H, W, labels):
    """(Y [G, ...] float64, EY [G, ...] its fp32 error bound, full reconstruction, its error bound)."""
    H, W = np.asarray(H), np.asarray(W)
    G, members, _, _ = tables(labels)
    full, fb, K, conv = _recon64(H, W)
    Y, EY = np.zeros((G,) + full.shape), np.zeros((G,) + full.shape)
    for g, idx in enumerate(members):
        if idx:
            y, b, Kg, _ = _recon64(H[:, idx], W[:, idx])
            Y[g], EY[g] = y, plane_error(b, Kg, conv)
    return Y, EY, full, plane_error(fb, K, conv)


# ---- masks -----------------------------------------------------------------------------------------------------------------------
def power_of(Y, EY, p):
    """(Y^p, its error bound) for the fp32 power ``p``."""
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(Y > 0, EY / np.where(Y > 0, Y, 1.0), 0.0)
        if p == 1.0:
            return Y, EY
        if p == 2.0:
            P = Y * Y
            return P, P * (2 * rel + U)
        P = np.where(Y > 0, np.power(np.where(Y > 0, Y, 1.0), p), 0.0)
        L = np.abs(np.log2(np.where(Y > 0, Y, 1.0)))
        return P, P * (p * rel + (p * L * (ULP_FN + 1) * LN2 + ULP_FN) * U)


def masks_of(Y, EY, p, D1=None, ED1=None):
    """(masks [G, ...], bound) from planes with error bounds; ``D1`` / ``ED1``: the denominator the kernel is given at
    ``p == 1`` (the reference value stays the float64 sum) and its error against that sum."""
    p = float(np.float32(p))
    G = Y.shape[0]
    P, EP = power_of(Y, EY, p)
    D = P.sum(0)
    ED = ED1 if D1 is not None else EP.sum(0) + (G - 1) * U * D
    den = D + EPS
    Eden = ED + U * den
    M = P / den
    return M, EP / den + P * Eden / den ** 2 + U * M


def emulate(H, W, V=None, groups=None, power=1.0, select=None):
    """(out [S, ...] float64 or complex128, bound [S, ...] float64 -- for a complex output it holds for either part)."""
    labels = normalise(groups, np.shape(W)[1])
    Y, EY, full, Efull = group_planes(H, W, labels)
    p = float(np.float32(power))
    if p == 1.0:
        # the kernels' denominator is the full reconstruction; against the float64 sum of the planes it is off by its own
        # fp32 error (the two float64 numbers agree to 2^-53 relative, which the bound of any fp32 result swallows)
        M, EM = masks_of(Y, EY, p, full, Efull)
    else:
        M, EM = masks_of(Y, EY, p)
    sel = list(range(Y.shape[0])) if select is None else [int(s) for s in select]
    return apply_mixture(M[sel], EM[sel], V)


def apply_mixture(M, EM, V):
    if V is None:
        return M, finish(EM)
    V = np.asarray(V)
    if np.iscomplexobj(V):
        V = V.astype(np.complex128)
        big = np.maximum(np.abs(V.real), np.abs(V.imag))[None]
        return V[None] * M, finish(big * EM + U * big * M)
    V = V.astype(np.float64)
    return V[None] * M, finish(np.abs(V)[None] * EM + U * np.abs(V[None] * M))


def finish(bound):
    bound = np.where(np.isnan(bound), 0.0, bound)
    return np.where(bound > 0, bound * SECOND_ORDER + TINY, 0.0)


def from_planes(Y, V=None, power=1.0, select=None, D=None):
    """The planes kernel on its own: ``Y`` [G, n] are GIVEN fp32 planes (no error of their own), ``D`` a given denominator."""
    Y = np.asarray(Y, np.float64)
    M, EM = masks_of(Y, np.zeros_like(Y), power)
    if D is not None:
        # a given denominator is used as it is: the reference is formed with it
        p = float(np.float32(power))
        P, EP = power_of(Y, np.zeros_like(Y), p)
        den = np.asarray(D, np.float64) + EPS
        M = P / den
        EM = EP / den + P * (U * den) / den ** 2 + U * M
    sel = list(range(Y.shape[0])) if select is None else [int(s) for s in select]
    return apply_mixture(M[sel], EM[sel], V)


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def check(got, ref, bound, what):
    """Every element: a NaN of ``ref`` must be a NaN of ``got``; elsewhere ``|got - ref| <= bound`` (for a complex output in
    either part; bound == 0 means exactly ``ref``).  Returns the worst error / bound."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f'{what}: shape {got.shape} != {ref.shape}'
    if np.iscomplexobj(ref):
        parts = [(got.real, ref.real), (got.imag, ref.imag)]
    else:
        parts = [(got, ref)]
    worst = 0.0
    for gp, rp in parts:
        gp, rp = np.asarray(gp, np.float64), np.asarray(rp, np.float64)
        nan = np.isnan(rp)
        assert np.array_equal(np.isnan(gp), nan), f'{what}: NaN pattern differs ({int(np.isnan(gp).sum())} vs {int(nan.sum())})'
        err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, gp) - np.where(nan, 0.0, rp)))
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = np.where(nan, 0.0, ratio)
        w = float(ratio.max()) if ratio.size else 0.0
        assert w <= 1.0, f'{what}: {int((ratio > 1.0).sum())} of {ratio.size} elements off, worst error / bound = {w:.4g}'
        worst = max(worst, w)
    return worst

