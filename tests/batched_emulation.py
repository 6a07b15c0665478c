"""Float64 reference of batched NMF (csrc/nmfmu_bmu.hip, batched.BatchedNMF), test-only: terms, step and loss of every
problem, the stop rule of the device (``judge``) and the whole ``fit`` loop with problems that stop on their own.

The batched kernel is the weighted kernel of csrc/nmfmu_wmu.hip with the problem index as a grid coordinate and no weights: the
same tile, the same stages, the same summation order (y: one MFMA accumulator over the full padded rank; a term rides the fmaf
chain of its part; the parts are added in part order), the same split rule -- a function of (rows, contraction, r_pad) in which
the batch does not appear.  So the per-element model IS tests/weighted_emulation.py driven with weights == 1, per problem, and
the counted bounds derived there (Higham's k u sum |terms| with k counted from the kernel source; none taken from a run) hold
here.  One count is loose by one: weighted_emulation counts a rounding for ``m * g``, which this kernel does not perform (it
stores g itself) -- the bound stays a bound.  An entry outside the matrix or the part is selected away by the kernel as a
weightless one is there, so nothing else differs.

The loss: per entry one fp32 expression of y widened to double, summed in double per lane, wave, workgroup, then per problem over
its workgroups' partials (strided lanes, tree): n 2^-53 sum |terms| as in weighted_emulation.loss; the terms of v alone are
float64 on the host.

The judge (bmu_judge_kernel) and the loop (BatchedNMF.fit) are restated in float64 as they are written: nmf.py:355-407 per
problem, a stopped problem frozen.
"""
from __future__ import annotations

import numpy as np

import weighted_emulation as WE

EPS, U = WE.EPS, WE.U
BK, TILE_ROWS = WE.BK, WE.TILE_ROWS
kind_of, gamma_of, bound_err = WE.kind_of, WE.gamma_of, WE.bound_err
split, part_len, stages, parts_for = WE.split, WE.part_len, WE.stages, WE.parts_for
loss_parts = WE.loss_parts          # per problem; the batch holds batch * loss_parts(n, c) partials


def workspace_floats(batch: int, rows: int, contraction: int, r_pad: int, nsplit: int = 0) -> int:
    """include/nmfmu.h, nmfmu_bmu_ws: the slab [problem][part][num | den][rows][r_pad]; the split ignores the batch."""
    return batch * split(rows, contraction, r_pad, nsplit) * 2 * rows * r_pad


def _ones(V):
    return np.ones(np.shape(V), dtype=np.float64)


def _target(V, b):
    """Problem b's target: V [B, N, C], or [N, C] shared by every problem."""
    V = np.asarray(V)
    return V if V.ndim == 2 else V[b]


def terms(V, H, W, beta: float, side: str, nsplit: int = 0):
    """One problem: dict(num, den, num_bound, den_bound, parts), [owner rows, R]."""
    return WE.terms(V, _ones(V), H, W, beta, side, nsplit)


def step(V, H, W, beta: float, side: str, l1=0.0, l2=0.0, nsplit: int = 0):
    """One problem: (new owner, bound, terms) of one half-step."""
    return WE.step(V, _ones(V), H, W, beta, side, l1, l2, nsplit)


def loss(V, H, W, beta: float):
    """One problem: (beta_div(H W^T, V, beta), its bound)."""
    return WE.loss(V, _ones(V), H, W, beta)


def dense_loss(V, H, W, beta: float) -> float:
    return WE.dense_loss(V, _ones(V), H, W, beta)


def v_term(V, beta: float) -> float:
    return WE.v_term(V, _ones(V), beta)


def sqrt2(div: float) -> float:
    d = 2.0 * div
    return float(np.sqrt(d)) if d >= 0 else float('nan')


def judge(div, loss_init, previous, tol: float, iteration: int, active, n_iter) -> int:
    """bmu_judge_kernel on numpy arrays, in place: for every active problem loss = sqrt(2 div) (NaN when div < 0); it stops
    (n_iter = iteration + 1, active = 0) when (previous - loss) / loss_init < tol, else previous = loss.  Returns the number
    of problems still active."""
    alive = 0
    for b in range(len(div)):
        if not active[b]:
            continue
        ls = sqrt2(float(div[b]))
        if (previous[b] - ls) / loss_init[b] < tol:          # (a NaN on either side: False)
            n_iter[b] = iteration + 1
            active[b] = 0
        else:
            previous[b] = ls
            alive += 1
    return alive


def fit(V, W0, H0, beta: float, tol: float, max_iter: int, l1=0.0, l2=0.0, update_W=True, update_H=True, loss_fn=None):
    """BatchedNMF.fit in float64: (W [B, C, R], H [B, N, R], n_iter [B] int64, checkpoint losses per problem).  ``loss_fn(b, H,
    W)`` replaces the divergence of problem b (the tests feed a negative one)."""
    W, H = np.asarray(W0, np.float64).copy(), np.asarray(H0, np.float64).copy()
    B = H.shape[0]

    def divs(only=None):
        out = np.zeros(B)
        for b in range(B):
            if only is None or only[b]:
                out[b] = loss(_target(V, b), H[b], W[b], beta)[0] if loss_fn is None else loss_fn(b, H[b], W[b])
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
            Vb = _target(V, b)
            if update_W:
                W[b] = step(Vb, H[b], W[b], beta, 'w', l1, l2)[0]
            if update_H:
                H[b] = step(Vb, H[b], W[b], beta, 'h', l1, l2)[0]
        if it % 10 == 9:
            was = active.copy()
            d = divs(active)
            for b in range(B):
                if was[b]:
                    trace[b].append(sqrt2(float(d[b])))
            if judge(d, loss_init, previous, tol, it, active, n_iter) == 0:
                break
    return W, H, n_iter, trace


def make_problems(B: int, N: int, C: int, R: int, seed: int = 0):
    """(V [B, N, C], W0 [B, C, R], H0 [B, N, R]) fp32: distinct problems, targets uniform in [0.1, 2), factors in [0.1, 1)."""
    g = np.random.default_rng(5000 * seed + 11 * N + 5 * C + R + 977 * B)
    V = (g.random((B, N, C)) * 1.9 + 0.1).astype(np.float32)
    W0 = (g.random((B, C, R)) * 0.9 + 0.1).astype(np.float32)
    H0 = (g.random((B, N, R)) * 0.9 + 0.1).astype(np.float32)
    return V, W0, H0
