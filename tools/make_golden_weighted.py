#!/usr/bin/env python3
"""Generate tests/golden/g23_weighted_fit.npz by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden_masked.py: the
reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs, and only inputs and
outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_weighted.py

Weighted NMF: ``sum_ij m_ij d_beta(v_ij | y_ij)`` on a dense target.  The reference has no weights, but for INTEGER weights
the weighted update is its own update rule (nmf.py: _double_backward_update) driven on the gathered graph
``(H @ W.T)[rows, cols]`` in which every pair (i, j) appears ``m_ij`` times: both backward passes then reach the factors
through every entry as often as its weight says, and a weightless entry not at all.  beta == 1: the function takes its
positive term ready-made; it is handed what it forms itself from a ones seed, the gradient of ``WH[idx].sum()``, relu, plus
eps.  W half-step, then H half-step with the new W, ``K`` iterations (nmf.py:365-398); then
``metrics.beta_div(WH[idx], values, beta)`` on the repeated pairs -- the weighted loss.

Target 37 x 29, rank 5, weights in {0, 1, 2, 3} (each with probability 1/4), row 11 and column 7 weightless, values uniform
in [0.1, 2); factors uniform in [0.1, 1).  Cases: beta in {-1, 0, 0.5, 1, 1.5, 2, 3} x (no regulariser | alpha = 0.07,
l1_ratio = 0.3), and one with W frozen (beta = 1.5).  Everything runs in float64 on the fp32-rounded inputs; each case is
SCREENED against the reference's own fp32 run (refused above 1e-5 relative Frobenius on either factor -- a condition on the
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
from torchnmf.metrics import beta_div as ref_beta_div  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
SEED = 23
N, C, R, K = 37, 29, 5, 20
BETAS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
ALPHA, L1_RATIO = 0.07, 0.3
SCREEN = 1e-5


def problem():
    g = torch.Generator().manual_seed(SEED)
    M = torch.randint(0, 4, (N, C), generator=g)
    M[11] = 0
    M[:, 7] = 0
    V = torch.rand(N, C, generator=g) * 1.9 + 0.1
    pairs = M.nonzero()
    idx = pairs.repeat_interleave(M[pairs[:, 0], pairs[:, 1]], dim=0).T.contiguous()     # every pair m_ij times
    vals = V[idx[0], idx[1]]
    W0 = torch.rand(C, R, generator=g) * 0.9 + 0.1
    H0 = torch.rand(N, R, generator=g) * 0.9 + 0.1
    return V, M, idx, vals, W0, H0


def gamma_of(beta):      # nmf.py:341-346
    return 1 / (2 - beta) if beta < 1 else (1 / (beta - 1) if beta > 2 else 1)


def half_step(param, H, W, idx, vals, beta, l1, l2):
    WH = (H @ W.T)[idx[0], idx[1]]
    pos = None
    if beta == 1:
        (g,) = torch.autograd.grad(WH.sum(), param, retain_graph=True)
        pos = g.relu_().add_(REF_EPS)
    ref_nmf._double_backward_update(vals, WH, param, beta, gamma_of(beta), l1, l2, pos)


def run(idx, vals, W0, H0, beta, l1, l2, dtype, update_W=True):
    W = torch.nn.Parameter(W0.to(dtype).clone(), requires_grad=update_W)
    H = torch.nn.Parameter(H0.to(dtype).clone())
    v = vals.to(dtype)
    for _ in range(K):
        if update_W:
            half_step(W, H, W, idx, v, beta, l1, l2)
        half_step(H, H, W, idx, v, beta, l1, l2)
    with torch.no_grad():
        loss = ref_beta_div((H @ W.T)[idx[0], idx[1]], v, beta)
    return W.detach(), H.detach(), float(loss)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    V, M, idx, vals, W0, H0 = problem()
    data = dict(V=V.numpy(), M=M.numpy().astype(np.int32), W0=W0.numpy(), H0=H0.numpy(),
                iterations=np.asarray(K, dtype=np.int64))
    cases = [(beta, reg, True) for beta in BETAS for reg in (False, True)] + [(1.5, False, False)]
    names = []
    for beta, reg, update_W in cases:
        l1, l2 = (ALPHA * L1_RATIO, ALPHA * (1 - L1_RATIO)) if reg else (0.0, 0.0)
        W64, H64, loss64 = run(idx, vals, W0, H0, beta, l1, l2, torch.float64, update_W)
        W32, H32, loss32 = run(idx, vals, W0, H0, beta, l1, l2, torch.float32, update_W)
        errs = (rel(W32, W64), rel(H32, H64))
        name = f'b{beta:g}' + ('_reg' if reg else '') + ('' if update_W else '_frozenW')
        if max(errs) > SCREEN or not np.isfinite(loss64):
            raise SystemExit(f'g23 {name}: refused by the screen (fp32-fp64 W {errs[0]:.2e} H {errs[1]:.2e}, loss {loss64})')
        print(f'g23 {name}: loss {loss64:.12g} (fp32 run {loss32:.9g}), fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e}')
        names.append(name)
        data[f'{name}_par'] = np.asarray([beta, ALPHA if reg else 0.0, L1_RATIO if reg else 0.0, float(update_W)])
        data[f'{name}_W'], data[f'{name}_H'] = W64.numpy(), H64.numpy()
        data[f'{name}_loss'] = np.asarray(loss64, dtype=np.float64)
    data['cases'] = np.asarray(names)
    path = os.path.join(OUT, 'g23_weighted_fit.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_weighted.txt'), 'w') as f:
        f.write(f'g23_weighted_fit: generated by `python tools/make_golden_weighted.py{"".join(" " + a for a in sys.argv[1:])}` '
                f'from torchnmf {torchnmf.__version__} (the reference, imported), torch {torch.__version__}, CPU, 1 thread, '
                f'seed {SEED}.  The reference\'s _double_backward_update driven on the gathered graph (H @ W.T)[rows, cols] '
                f'with every pair repeated as often as its integer weight says, W then H half-step, {K} iterations, float64 on fp32-rounded inputs; '
                f'metrics.beta_div on the gathered reconstruction afterwards.  Every case screened against the reference\'s '
                f'own fp32 run (both factors within {SCREEN:g}).\n')
