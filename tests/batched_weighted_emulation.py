"""Float64 reference of weighted batched NMF (the nmfmu_bwmu entries of csrc/nmfmu_bmu.hip, ``BatchedNMF.fit(V, weights=M)``,
``model_selection.cross_validate``), test-only.

The weighted batched kernel is the weighted kernel of csrc/nmfmu_wmu.hip with the problem index as a grid coordinate: the same
stage (V and M travel together), the same seeds (``m * g`` with the weightless entries selected away), the same summation
order, the same split rule in which neither the batch nor the weights appear, the same apply -- with the problem's own
``(l1, l2)`` when a ``reg`` vector is given.  So the per-element model IS tests/weighted_emulation.py driven per problem with
the problem's own ``M`` and ``(l1, l2)``, and the bounds counted there (Higham's k u sum |terms| with k counted from the kernel
source; none taken from a run) hold unchanged: this kernel does perform the ``m * g`` multiply that is counted.

The loss: weighted_emulation.loss per problem (the partials are reduced per problem as in batched_emulation).  The terms of v
alone (``nmfmu_bwmu_v_term``): every term, its product with m and the sum in double on the device.

The fit loop and the judge are batched_emulation's, restated here with per-problem weights and regularisers because
``batched_emulation.fit`` steps every problem unweighted with one (l1, l2); ``cross_validate`` is restated from given starts
and masks on top of it.
"""
from __future__ import annotations

import numpy as np

import batched_emulation as BE
import weighted_emulation as WE

EPS, U = WE.EPS, WE.U
kind_of, gamma_of, bound_err = WE.kind_of, WE.gamma_of, WE.bound_err
split, loss_parts = WE.split, WE.loss_parts
workspace_floats = BE.workspace_floats          # the slab is the unweighted batch's: the weights do not enter
judge, sqrt2 = BE.judge, BE.sqrt2


def _slice(A, b, index=None):
    """Problem b's target or weights: A [N, C] shared, A [B, N, C], or A [G, N, C] read through ``index``."""
    A = np.asarray(A)
    if A.ndim == 2:
        return A
    return A[b if index is None else int(index[b])]


def _reg(reg, b):
    """Problem b's (l1, l2): ``reg`` is one pair or [B, 2]."""
    reg = np.asarray(reg, dtype=np.float64)
    return (float(reg[0]), float(reg[1])) if reg.ndim == 1 else (float(reg[b, 0]), float(reg[b, 1]))


def l1_l2(alpha, l1_ratio):
    """nmf.py:348-349 in double: [..., 2] pairs (l1, l2) (the library rounds them to fp32 once, as it does the scalars)."""
    a, r = np.asarray(alpha, np.float64), np.asarray(l1_ratio, np.float64)
    return np.stack(np.broadcast_arrays(a * r, a * (1 - r)), -1)


def terms(V, M, H, W, beta, side, nsplit=0, index=None):
    """Per problem: a list of WE.terms dicts."""
    return [WE.terms(_slice(V, b), _slice(M, b, index), H[b], W[b], beta, side, nsplit) for b in range(len(H))]


def step(V, M, H, W, beta, side, reg=(0.0, 0.0), nsplit=0, index=None):
    """Per problem: a list of (new owner, bound, terms)."""
    return [WE.step(_slice(V, b), _slice(M, b, index), H[b], W[b], beta, side, *_reg(reg, b), nsplit) for b in range(len(H))]


def loss(V, M, H, W, beta, index=None):
    """Per problem: a list of (weighted loss, bound)."""
    return [WE.loss(_slice(V, b), _slice(M, b, index), H[b], W[b], beta) for b in range(len(H))]


def v_term(V, M, beta, B, index=None):
    """([B] the terms of v alone: WE.v_term per problem, [B] sum |m * term|: the magnitude the device's double sum is judged
    against)."""
    out, mag = np.zeros(B), np.zeros(B)
    for b in range(B):
        Vb, Mb, sel = WE.clean(_slice(V, b), _slice(M, b, index))
        v, m = Vb[sel], Mb[sel]
        kind = kind_of(beta)
        if kind == 'euc':
            continue
        if kind == 'kl':
            a = np.abs(v * np.log(v + EPS)) + v
        elif kind == 'is':
            a = np.abs(np.log(v + EPS)) + 1.0
        else:
            a = np.power(v + EPS if beta < 0 else v, beta)
        out[b], mag[b] = WE.v_term(_slice(V, b), _slice(M, b, index), beta), float(m @ a)
    return out, mag


def fit(V, M, W0, H0, beta, tol, max_iter, reg=(0.0, 0.0), index=None, update_W=True, update_H=True):
    """``BatchedNMF.fit(V, weights=M, weight_index=index)`` in float64 -- batched_emulation.fit's loop and judge with every
    problem stepped under its own weights and (l1, l2) and judged on its weighted loss: (W, H, n_iter, checkpoint losses)."""
    W, H = np.asarray(W0, np.float64).copy(), np.asarray(H0, np.float64).copy()
    B = H.shape[0]

    def divs(only=None):
        out = np.zeros(B)
        for b in range(B):
            if only is None or only[b]:
                out[b] = WE.loss(_slice(V, b), _slice(M, b, index), H[b], W[b], beta)[0]
        return out
    loss_init = np.array([sqrt2(d) for d in divs()])
    previous = loss_init.copy()
    active = np.ones(B, dtype=np.int32)
    n_iter = np.full(B, max_iter, dtype=np.int64)
    trace = [[float(x)] for x in loss_init]
    for it in range(max_iter):
        for b in range(B):
            if not active[b]:
                continue
            Vb, Mb, (l1, l2) = _slice(V, b), _slice(M, b, index), _reg(reg, b)
            if update_W:
                W[b] = WE.step(Vb, Mb, H[b], W[b], beta, 'w', l1, l2)[0]
            if update_H:
                H[b] = WE.step(Vb, Mb, H[b], W[b], beta, 'h', l1, l2)[0]
        if it % 10 == 9:
            was = active.copy()
            with np.errstate(invalid='ignore', divide='ignore'):
                d = divs(active)
                for b in range(B):
                    if was[b]:
                        trace[b].append(sqrt2(float(d[b])))
                alive = judge(d, loss_init, previous, tol, it, active, n_iter)
            if alive == 0:
                break
    return W, H, n_iter, trace


def judged_margins(trace, tol):
    """|(previous - loss) / loss_init - tol| of every judged checkpoint of ``fit``'s traces, flattened: how far the float64
    model's decisions lie from the threshold."""
    out = []
    for tr in trace:
        for prev, cur in zip(tr[:-1], tr[1:]):
            out.append(abs((prev - cur) / tr[0] - tol))
    return np.asarray(out)


def problem_layout(n_alpha, folds, n_init):
    """model_selection.problem_layout: the batch is [alpha][fold][start] flattened."""
    idx = np.arange(n_alpha * folds * n_init)
    return idx // (folds * n_init), (idx // n_init) % folds, idx % n_init


def cross_validate(V, train, test, starts, ranks, alphas, beta, l1_ratio, max_iter, tol=-1e9):
    """``model_selection.cross_validate`` in float64 from given masks (``train`` / ``test`` [K, N, C]) and starts
    (``starts[i] = (W0 [B, C, R_i], H0 [B, N, R_i])``): dict(W, H, n_iter, train_loss, test_loss, n_test, mean_test, best)."""
    folds = len(train)
    n_init = starts[0][0].shape[0] // (len(alphas) * folds)
    a_of, k_of, _ = problem_layout(len(alphas), folds, n_init)
    reg = l1_l2(np.asarray(alphas, np.float64)[a_of], l1_ratio)
    shape = (len(ranks), len(alphas), folds, n_init)
    out = dict(W=[], H=[], n_iter=np.zeros(shape, np.int64), train_loss=np.zeros(shape), test_loss=np.zeros(shape))
    for i in range(len(ranks)):
        W, H, n, _ = fit(V, train, starts[i][0], starts[i][1], beta, tol, max_iter, reg, k_of)
        out['W'].append(W)
        out['H'].append(H)
        out['n_iter'][i] = n.reshape(shape[1:])
        out['train_loss'][i] = np.array([x[0] for x in loss(V, train, H, W, beta, k_of)]).reshape(shape[1:])
        out['test_loss'][i] = np.array([x[0] for x in loss(V, test, H, W, beta, k_of)]).reshape(shape[1:])
    out['n_test'] = np.asarray(test, np.float64).sum(axis=(1, 2))
    out['mean_test'], out['best'] = summarise(out['test_loss'], out['n_test'], ranks, alphas)
    return out


def summarise(test_loss, n_test, ranks, alphas):
    mean_test = (test_loss / n_test.reshape(1, 1, -1, 1)).mean(axis=(2, 3))
    flat = np.where(np.isnan(mean_test), np.inf, mean_test).reshape(-1)
    at = int(flat.argmin())
    return mean_test, (ranks[at // len(alphas)], alphas[at % len(alphas)])


def make_problems(B, N, C, R, seed=0):
    """B distinct problems of weighted_emulation.make_problem: (V [B, N, C], M [B, N, C], W0 [B, C, R], H0 [B, N, R])."""
    ps = [WE.make_problem(N, C, R, seed=seed + 17 * b) for b in range(B)]
    return tuple(np.stack([p[k] for p in ps]) for k in range(4))


def make_stop_problems(B, N, C, R, seed=0):
    """make_problems with a planted target of rank 2 or 3 (noisy, as ``planted``) wherever the weight is positive: fits that
    reach the stop rule's threshold within a hundred iterations, at different counts."""
    V, M, W0, H0 = make_problems(B, N, C, R, seed)
    P = np.stack([planted(N, C, 2 + b % 2, seed=40 + b + 100 * seed) for b in range(B)])
    return np.where(M > 0, P, V).astype(np.float32), M, W0, H0


def planted(N=131, C=70, R=4, seed=0):
    """The planted target of the cross-validation test: |H W^T (1 + 0.1 randn)| + 1e-3 at true rank R, fp32."""
    g = np.random.default_rng(seed)
    H, W = g.random((N, R)), g.random((C, R))
    return (np.abs((H @ W.T) * (1 + 0.1 * g.standard_normal((N, C)))) + 1e-3).astype(np.float32)
