#!/usr/bin/env python3
"""Generate tests/golden/g22_fold_in.npz by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden_masked.py: the
reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs, and only inputs and
outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_fold_in.py

Fold-in: H for new rows with W FROZEN, 20 iterations of the H half-step.  The problem is g20's (tools/make_golden_masked.py:
37 x 29, rank 5, about 30 % stored, row 11 and column 7 without entries, seed 20), read as 37 new rows against a fitted W0.

* ``zero_*``: the reference's own ``NMF(W=W0, H=H0, trainable_W=False).fit(V_sparse, beta, tol=-inf, max_iter=20)`` (the stop
  rule ``(previous - loss) / loss_init < tol`` cannot fire; the call is asserted to return 20), beta in {1, 2}.
* ``missing_*``: the reference has no such mode; its ``_double_backward_update`` is driven on the GATHERED graph
  ``(H @ W.T)[rows, cols]`` against the stored values, exactly as tools/make_golden_masked.py does, with W frozen,
  beta in {-1, 0, 0.5, 1, 1.5, 2, 3}.

Each x (no regulariser | alpha = 0.07, l1_ratio = 0.3).  Everything runs in float64 on the fp32-rounded inputs; each case is
SCREENED against the reference's own fp32 run (refused above 1e-5 relative Frobenius on H, or if W moved -- a condition on the
fixture, not a tolerance of any test).
"""
import os
import sys

import numpy as np
import torch

if os.environ.get('NMF_REFERENCE'):
    sys.path.insert(0, os.environ['NMF_REFERENCE'])
import torchnmf  # noqa: E402
from torchnmf import nmf as ref_nmf  # noqa: E402
from torchnmf.constants import eps as REF_EPS  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
SEED = 20
N, C, R, K = 37, 29, 5, 20
ZERO_BETAS = (1.0, 2.0)
MISSING_BETAS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
ALPHA, L1_RATIO = 0.07, 0.3
SCREEN = 1e-5


def problem():       # tools/make_golden_masked.py: problem(), draw for draw
    g = torch.Generator().manual_seed(SEED)
    keep = torch.rand(N, C, generator=g) < 0.3
    keep[11] = False
    keep[:, 7] = False
    V = torch.rand(N, C, generator=g) * 1.9 + 0.1
    idx = keep.nonzero().T.contiguous()
    vals = V[keep]
    W0 = torch.rand(C, R, generator=g) * 0.9 + 0.1
    H0 = torch.rand(N, R, generator=g) * 0.9 + 0.1
    return idx, vals, W0, H0


def gamma_of(beta):      # nmf.py:341-346
    return 1 / (2 - beta) if beta < 1 else (1 / (beta - 1) if beta > 2 else 1)


def run_zero(idx, vals, W0, H0, beta, alpha, l1_ratio, dtype):
    m = ref_nmf.NMF(W=W0, H=H0, trainable_W=False).to(dtype)
    with torch.no_grad():
        m.W.copy_(W0.to(dtype))
        m.H.copy_(H0.to(dtype))
    V = torch.sparse_coo_tensor(idx, vals.to(dtype), (N, C))
    n = m.fit(V, beta=beta, tol=-float('inf'), max_iter=K, alpha=alpha, l1_ratio=l1_ratio)
    assert n == K, f'the reference ran {n} iterations, not {K}'
    return m.W.detach().clone(), m.H.detach().clone()


def run_missing(idx, vals, W0, H0, beta, alpha, l1_ratio, dtype):
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    W = torch.nn.Parameter(W0.to(dtype).clone(), requires_grad=False)
    H = torch.nn.Parameter(H0.to(dtype).clone())
    v = vals.to(dtype)
    for _ in range(K):
        WH = (H @ W.T)[idx[0], idx[1]]
        pos = None
        if beta == 1:
            (g,) = torch.autograd.grad(WH.sum(), H, retain_graph=True)
            pos = g.relu_().add_(REF_EPS)
        ref_nmf._double_backward_update(v, WH, H, beta, gamma_of(beta), l1, l2, pos)
    return W.detach(), H.detach()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    idx, vals, W0, H0 = problem()
    data = dict(shape=np.asarray([N, C], dtype=np.int64), indices=idx.numpy(), values=vals.numpy(), W0=W0.numpy(),
                H0=H0.numpy(), iterations=np.asarray(K, dtype=np.int64))
    cases = [('zero', b, reg) for b in ZERO_BETAS for reg in (False, True)]
    cases += [('missing', b, reg) for b in MISSING_BETAS for reg in (False, True)]
    names = []
    for mode, beta, reg in cases:
        alpha, l1_ratio = (ALPHA, L1_RATIO) if reg else (0.0, 0.0)
        run = run_zero if mode == 'zero' else run_missing
        W64, H64 = run(idx, vals, W0, H0, beta, alpha, l1_ratio, torch.float64)
        W32, H32 = run(idx, vals, W0, H0, beta, alpha, l1_ratio, torch.float32)
        err = rel(H32, H64)
        worst = float((H32.double() - H64).abs().max())
        name = f'{mode}_b{beta:g}' + ('_reg' if reg else '')
        if not (torch.equal(W64, W0.double()) and torch.equal(W32, W0)):
            raise SystemExit(f'g22 {name}: W moved')
        if err > SCREEN or not bool(torch.isfinite(H64).all()):
            raise SystemExit(f'g22 {name}: refused by the screen (fp32-fp64 H {err:.2e})')
        print(f'g22 {name}: fp32-fp64 H {err:.1e}, worst element {worst:.1e}')
        names.append(name)
        data[f'{name}_par'] = np.asarray([beta, alpha, l1_ratio, float(mode == 'missing')])
        data[f'{name}_H'] = H64.numpy()
    data['cases'] = np.asarray(names)
    path = os.path.join(OUT, 'g22_fold_in.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_fold_in.txt'), 'w') as f:
        f.write(f'g22_fold_in: generated by `python tools/make_golden_fold_in.py{"".join(" " + a for a in sys.argv[1:])}` '
                f'from torchnmf {torchnmf.__version__} (the reference, imported), torch {torch.__version__}, CPU, 1 thread, '
                f'seed {SEED} (the problem of g20).  W frozen, {K} iterations of the H half-step, float64 on fp32-rounded '
                f'inputs.  zero_*: the reference\'s NMF(W=W0, H=H0, trainable_W=False).fit(V_sparse, beta, tol=-inf, '
                f'max_iter={K}), asserted to run {K} iterations.  missing_*: the reference\'s _double_backward_update driven '
                f'on the gathered graph (H @ W.T)[rows, cols] against the stored values.  Every case screened against the '
                f'reference\'s own fp32 run (H within {SCREEN:g}, W bitwise unchanged).\n')
