#!/usr/bin/env python3
"""Generate tests/golden/g24_batched_fit.npz by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden_weighted.py:
the reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs, and only inputs and
outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_batched.py

Six problems 37 x 29, rank 5, fitted ONE AT A TIME by the reference's own ``NMF.fit`` (tol = 1e-3, max_iter = 80): what
``BatchedNMF.fit`` must give for each of them when it fits all six together.  Problems 0, 1: near-low-rank targets
(``rand(N, 5) @ rand(5, C) + 0.05``); 2, 3: uniform in [0.1, 2); 4, 5: heavy-tailed (``rand^4 * 3 + 0.01``).  ``W0``, ``H0``
uniform in [0.1, 1).  Sets: beta in {0.5, 1, 2}, one regularised (beta = 1, alpha = 0.07, l1_ratio = 0.3) and one with W
frozen (beta = 2).  Stored per set: the iteration counts, the factors and the final divergences of the float64 runs.

Conditions on the fixture, enforced here (none of them is a tolerance of a test):
  * the reference's float64 and fp32 runs return the same count for every problem and factors (W and H) within 1e-5
    relative Frobenius;
  * per beta (the three plain sets) at least one problem stops before max_iter and at least one reaches it;
  * at every checkpoint of the float64 run |(previous - loss) / loss_init - tol| >= 0.05 tol, so that fp32 rounding cannot
    flip a decision.  The checkpoint losses are the reference's: ``fit(max_iter=k, tol=-inf)`` for k = 10, 20, ... from the
    same start, then ``beta_div(m(), V, beta).mul(2).sqrt()``.
The last problem is the one that must stop early for every beta.  A problem that misses one of the per-problem conditions in
any set moves on to its next seed (100 + b, then + 6, + 12, ...); the seeds that were taken are stored.
"""
import os
import sys

import numpy as np
import torch

if os.environ.get('NMF_REFERENCE'):
    sys.path.insert(0, os.environ['NMF_REFERENCE'])
import torchnmf  # noqa: E402
from torchnmf.metrics import beta_div as ref_beta_div  # noqa: E402
from torchnmf.nmf import NMF as RefNMF  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
B, N, C, R = 6, 37, 29, 5
TOL, MAX_ITER = 1e-3, 80
ALPHA, L1_RATIO = 0.07, 0.3
SCREEN, MARGIN = 1e-5, 0.05
EARLY = (5,)             # problems that must stop before max_iter for every beta (problems 0 and 1 reach it)
# name -> (beta, alpha, l1_ratio, update_W)
SETS = {'b0.5': (0.5, 0.0, 0.0, True), 'b1': (1.0, 0.0, 0.0, True), 'b2': (2.0, 0.0, 0.0, True),
        'b1_reg': (1.0, ALPHA, L1_RATIO, True), 'b2_frozenW': (2.0, 0.0, 0.0, False)}


def problem(b, seed):
    g = torch.Generator().manual_seed(seed)
    if b < 2:
        V = torch.rand(N, 5, generator=g) @ torch.rand(5, C, generator=g) + 0.05
    elif b < 4:
        V = torch.rand(N, C, generator=g) * 1.9 + 0.1
    else:
        V = torch.rand(N, C, generator=g) ** 4 * 3 + 0.01
    W0 = torch.rand(C, R, generator=g) * 0.9 + 0.1
    H0 = torch.rand(N, R, generator=g) * 0.9 + 0.1
    return V, W0, H0


def fit(V, W0, H0, par, dtype, max_iter=MAX_ITER, tol=TOL):
    beta, alpha, l1_ratio, update_W = par
    m = RefNMF(W=W0, H=H0, trainable_W=update_W).to(dtype)
    m.W.data.copy_(W0.to(dtype))
    m.H.data.copy_(H0.to(dtype))
    n = 0          # (the reference's fit cannot run zero iterations: its return value is the loop variable)
    if max_iter > 0:
        n = m.fit(V.to(dtype), beta=beta, tol=tol, max_iter=max_iter, alpha=alpha, l1_ratio=l1_ratio)
    with torch.no_grad():
        div = float(ref_beta_div(m(), V.to(dtype), beta))
    return n, m.W.detach().clone(), m.H.detach().clone(), div


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def margins(V, W0, H0, par):
    """min over the checkpoints the float64 run judges of |(previous - loss) / loss_init - tol| / tol"""
    def loss_after(k):
        return (2 * fit(V, W0, H0, par, torch.float64, k, -float('inf'))[3]) ** 0.5
    loss_init = previous = loss_after(0)
    worst = float('inf')
    for k in range(10, MAX_ITER + 1, 10):
        loss = loss_after(k)
        q = (previous - loss) / loss_init
        worst = min(worst, abs(q - TOL) / TOL)
        if q < TOL:
            break
        previous = loss
    return worst


def screen(b, seed):
    """None when the problem fails a per-problem condition in any set, else {set: (count, W, H, div)}"""
    V, W0, H0 = problem(b, seed)
    out = {}
    for name, par in SETS.items():
        n64, W64, H64, d64 = fit(V, W0, H0, par, torch.float64)
        n32, W32, H32, _ = fit(V, W0, H0, par, torch.float32)
        ew, eh, mg = rel(W32, W64), rel(H32, H64), margins(V, W0, H0, par)
        ok = n64 == n32 and max(ew, eh) <= SCREEN and mg >= MARGIN and np.isfinite(d64)
        if b in EARLY and par[1] == 0 and par[3]:       # the problem that must stop early in every plain set
            ok = ok and n64 < MAX_ITER
        print(f'g24 problem {b} seed {seed} {name}: count {n64} (fp32 {n32}), fp32-fp64 W {ew:.1e} H {eh:.1e}, '
              f'margin {mg:.3f} tol{"" if ok else "  -> refused"}')
        if not ok:
            return None
        out[name] = (n64, W64, H64, d64)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    seeds, results = [], []
    for b in range(B):
        for seed in range(100 + b, 100 + b + 6 * 40, 6):
            res = screen(b, seed)
            if res is not None:
                break
        else:
            raise SystemExit(f'g24: no seed of problem {b} meets the conditions')
        seeds.append(seed)
        results.append(res)
    probs = [problem(b, s) for b, s in enumerate(seeds)]
    data = dict(V=np.stack([p[0].numpy() for p in probs]), W0=np.stack([p[1].numpy() for p in probs]),
                H0=np.stack([p[2].numpy() for p in probs]), seeds=np.asarray(seeds, dtype=np.int64),
                tol=np.asarray(TOL), max_iter=np.asarray(MAX_ITER, dtype=np.int64), cases=np.asarray(list(SETS)))
    for name, par in SETS.items():
        counts = np.asarray([r[name][0] for r in results], dtype=np.int64)
        if par[1] == 0 and par[3] and not (counts.min() < MAX_ITER and counts.max() == MAX_ITER):
            raise SystemExit(f'g24 {name}: counts {counts.tolist()} -- one problem must stop early and one reach max_iter')
        data[f'{name}_par'] = np.asarray([par[0], par[1], par[2], float(par[3])])
        data[f'{name}_n_iter'] = counts
        data[f'{name}_W'] = np.stack([r[name][1].numpy() for r in results])
        data[f'{name}_H'] = np.stack([r[name][2].numpy() for r in results])
        data[f'{name}_div'] = np.asarray([r[name][3] for r in results], dtype=np.float64)
        print(f'g24 {name}: counts {counts.tolist()}')
    path = os.path.join(OUT, 'g24_batched_fit.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_batched.txt'), 'w') as f:
        f.write(f'g24_batched_fit: generated by `python tools/make_golden_batched.py{"".join(" " + a for a in sys.argv[1:])}` '
                f'from torchnmf {torchnmf.__version__} (the reference, imported), torch {torch.__version__}, CPU, 1 thread, '
                f'seeds {seeds}.  The reference\'s own NMF.fit once per problem (tol {TOL:g}, max_iter {MAX_ITER}), float64 on '
                f'fp32-rounded inputs.  Every problem screened in every set: same count in the reference\'s fp32 run, W and H '
                f'within {SCREEN:g}, every judged checkpoint at least {MARGIN:g} tol away from the threshold.\n')
