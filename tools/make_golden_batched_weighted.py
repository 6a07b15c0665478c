#!/usr/bin/env python3
"""Generate tests/golden/g25_batched_weighted.npz by RUNNING the reference (torchnmf 0.3.5), like
tools/make_golden_weighted.py: the reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded
inputs, and only inputs and outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_batched_weighted.py

Weighted batched NMF: four problems of ONE shared target, each under its own integer weights and its own regulariser.  The
recipe per problem is g23's: for integer weights the weighted update is the reference's own rule (nmf.py:
_double_backward_update) driven on the gathered graph ``(H @ W.T)[rows, cols]`` in which every pair (i, j) appears ``m_ij``
times; W half-step, then H half-step with the new W, ``K`` iterations; then ``metrics.beta_div`` on the gathered reconstruction
-- the weighted loss.

Target 37 x 29, rank 5; two weight matrices in {0, 1, 2, 3} stored as (2, N, C), row 11 and column 7 weightless in both;
``weight_index`` [0, 1, 0, 1]; problems 0, 1 under (alpha, l1_ratio) = (0, 0) and problems 2, 3 under (0.07, 0.3); four distinct
starts; beta in {0, 0.5, 1, 2}.  Everything runs in float64 on the fp32-rounded inputs; each problem of each case is SCREENED
against the reference's own fp32 run (refused above 1e-5 relative Frobenius on either factor -- a condition on the fixture,
not a tolerance of any test).
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
SEED = 25
N, C, R, K, B, G = 37, 29, 5, 20, 4, 2
BETAS = (0.0, 0.5, 1.0, 2.0)
INDEX = (0, 1, 0, 1)
ALPHA = (0.0, 0.0, 0.07, 0.07)
L1_RATIO = (0.0, 0.0, 0.3, 0.3)
SCREEN = 1e-5


def problem():
    g = torch.Generator().manual_seed(SEED)
    M = torch.randint(0, 4, (G, N, C), generator=g)
    M[:, 11] = 0
    M[:, :, 7] = 0
    V = torch.rand(N, C, generator=g) * 1.9 + 0.1
    W0 = torch.rand(B, C, R, generator=g) * 0.9 + 0.1
    H0 = torch.rand(B, N, R, generator=g) * 0.9 + 0.1
    return V, M, W0, H0


def gathered(V, M):
    pairs = M.nonzero()
    idx = pairs.repeat_interleave(M[pairs[:, 0], pairs[:, 1]], dim=0).T.contiguous()     # every pair m_ij times
    return idx, V[idx[0], idx[1]]


def gamma_of(beta):      # nmf.py:341-346
    return 1 / (2 - beta) if beta < 1 else (1 / (beta - 1) if beta > 2 else 1)


def half_step(param, H, W, idx, vals, beta, l1, l2):
    WH = (H @ W.T)[idx[0], idx[1]]
    pos = None
    if beta == 1:
        (g,) = torch.autograd.grad(WH.sum(), param, retain_graph=True)
        pos = g.relu_().add_(REF_EPS)
    ref_nmf._double_backward_update(vals, WH, param, beta, gamma_of(beta), l1, l2, pos)


def run(idx, vals, W0, H0, beta, l1, l2, dtype):
    W = torch.nn.Parameter(W0.to(dtype).clone())
    H = torch.nn.Parameter(H0.to(dtype).clone())
    v = vals.to(dtype)
    for _ in range(K):
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
    V, M, W0, H0 = problem()
    data = dict(V=V.numpy(), M=M.numpy().astype(np.int32), W0=W0.numpy(), H0=H0.numpy(),
                weight_index=np.asarray(INDEX, dtype=np.int64), alpha=np.asarray(ALPHA), l1_ratio=np.asarray(L1_RATIO),
                iterations=np.asarray(K, dtype=np.int64))
    names = []
    for beta in BETAS:
        name = f'b{beta:g}'
        Ws, Hs, losses = [], [], []
        for b in range(B):
            idx, vals = gathered(V, M[INDEX[b]])
            l1, l2 = ALPHA[b] * L1_RATIO[b], ALPHA[b] * (1 - L1_RATIO[b])
            W64, H64, loss64 = run(idx, vals, W0[b], H0[b], beta, l1, l2, torch.float64)
            W32, H32, loss32 = run(idx, vals, W0[b], H0[b], beta, l1, l2, torch.float32)
            errs = (rel(W32, W64), rel(H32, H64))
            if max(errs) > SCREEN or not np.isfinite(loss64):
                raise SystemExit(f'g25 {name} problem {b}: refused by the screen (fp32-fp64 W {errs[0]:.2e} H {errs[1]:.2e}, '
                                 f'loss {loss64})')
            print(f'g25 {name} problem {b}: loss {loss64:.12g} (fp32 run {loss32:.9g}), fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e}')
            Ws.append(W64.numpy()), Hs.append(H64.numpy()), losses.append(loss64)
        names.append(name)
        data[f'{name}_beta'] = np.asarray(beta)
        data[f'{name}_W'], data[f'{name}_H'] = np.stack(Ws), np.stack(Hs)
        data[f'{name}_loss'] = np.asarray(losses, dtype=np.float64)
    data['cases'] = np.asarray(names)
    path = os.path.join(OUT, 'g25_batched_weighted.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_batched_weighted.txt'), 'w') as f:
        f.write(f'g25_batched_weighted: generated by `python tools/make_golden_batched_weighted.py'
                f'{"".join(" " + a for a in sys.argv[1:])}` from torchnmf {torchnmf.__version__} (the reference, imported), torch '
                f'{torch.__version__}, CPU, 1 thread, seed {SEED}.  Four problems of one shared {N} x {C} target at rank {R}: two '
                f'integer weight matrices in {{0, 1, 2, 3}} read through weight_index {list(INDEX)}, (alpha, l1_ratio) '
                f'{list(zip(ALPHA, L1_RATIO))}.  Per problem the reference\'s _double_backward_update driven on the gathered '
                f'graph (H @ W.T)[rows, cols] with every pair repeated as often as its integer weight says, W then H half-step, '
                f'{K} iterations, float64 on fp32-rounded inputs; metrics.beta_div on the gathered reconstruction afterwards.  '
                f'Every problem of every case screened against the reference\'s own fp32 run (both factors within {SCREEN:g}).\n')
