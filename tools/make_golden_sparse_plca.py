#!/usr/bin/env python3
"""Generate tests/golden/g21_sparse_plca.npz by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden_masked.py: the
reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs, and only inputs and
outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_sparse_plca.py

PLCA on a sparse count matrix.  The reference has no sparse path; it is run on the DENSIFIED target (zeros where nothing is
stored), which is the problem ``PLCA.fit`` solves on a sparse-COO target: G = Vn / (H diag(Z) W^T + eps) is zero wherever the
target is.  Target 37 x 29, about 30 % stored integer counts 1..9, row 11 and column 7 without entries, rank 5; factors uniform
in [0.1, 1).  Cases: plain (30 iterations, no stop), prior (W_alpha 1.02, H_alpha 0.99, Z_alpha 1.01), frozenZ, frozenW, and
stop (tol 1e-3, max_iter 200).

Everything runs in float64 on the fp32-rounded inputs.  Each case is SCREENED -- conditions on the fixture, not tolerances of
any test: the float64 run is within 1e-5 (relative Frobenius, W, H and Z) of the reference's own fp32 run and both stop at the
same iteration; for ``stop``, at every checkpoint up to the stop the tracked quantity (previous - loss) / loss_init keeps at
least 10 % of tol away from tol, so that no fp32 implementation of the same iterations stops elsewhere.
"""
import os
import sys

import numpy as np
import torch

if os.environ.get('NMF_REFERENCE'):
    sys.path.insert(0, os.environ['NMF_REFERENCE'])
import torchnmf  # noqa: E402
from torchnmf import plca as ref_plca  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
SEED = 21
N, C, R = 37, 29, 5
NO_STOP = -1e9
SCREEN = 1e-5
MARGIN = 0.1
CASES = {'plain': {}, 'prior': dict(W_alpha=1.02, H_alpha=0.99, Z_alpha=1.01), 'frozenZ': dict(trainable_Z=False),
         'frozenW': dict(trainable_W=False), 'stop': dict(tol=1e-3, max_iter=200)}


def problem():
    g = torch.Generator().manual_seed(SEED)
    keep = torch.rand(N, C, generator=g) < 0.3
    keep[11] = False
    keep[:, 7] = False
    counts = torch.floor(torch.rand(N, C, generator=g) * 9) + 1
    idx = keep.nonzero().T.contiguous()
    vals = counts[keep]
    W0 = torch.rand(C, R, generator=g) * 0.9 + 0.1
    H0 = torch.rand(N, R, generator=g) * 0.9 + 0.1
    Z0 = torch.rand(R, generator=g) * 0.9 + 0.1
    return idx, vals, W0, H0, Z0


def run(V, W0, H0, Z0, dtype, kw):
    """(n, norm, W, H, Z, tracked losses) of the reference's fit in ``dtype``."""
    kw = dict(kw)
    ctor = {k: kw.pop(k) for k in ('trainable_W', 'trainable_Z') if k in kw}
    kw.setdefault('tol', NO_STOP)
    kw.setdefault('max_iter', 30)
    m = ref_plca.PLCA(W=W0, H=H0, Z=Z0, **ctor).to(dtype)
    losses = []
    kl = ref_plca.kl_div

    def tap(*a, **k):
        out = kl(*a, **k)
        losses.append(float(out.mul(2).sqrt()))
        return out
    ref_plca.kl_div = tap
    try:
        n, norm = m.fit(V.to(dtype), **kw)
    finally:
        ref_plca.kl_div = kl
    return n, float(norm), m.W.detach(), m.H.detach(), m.Z.detach(), losses, kw['tol']


def initial(W0, H0, Z0):
    """The factors as the constructor normalises them (fp32): where every run starts."""
    m = ref_plca.PLCA(W=W0, H=H0, Z=Z0)
    return m.W.detach().numpy().copy(), m.H.detach().numpy().copy(), m.Z.detach().numpy().copy()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    idx, vals, W0, H0, Z0 = problem()
    V = torch.zeros(N, C)
    V[idx[0], idx[1]] = vals
    assert float(V[11].sum()) == 0 and float(V[:, 7].sum()) == 0
    data = dict(shape=np.asarray([N, C], dtype=np.int64), indices=idx.numpy(), values=vals.numpy(), W0=W0.numpy(),
                H0=H0.numpy(), Z0=Z0.numpy(), cases=np.asarray(list(CASES)))
    data['W_init'], data['H_init'], data['Z_init'] = initial(W0, H0, Z0)
    for name, kw in CASES.items():
        n64, norm64, W64, H64, Z64, losses, tol = run(V, W0, H0, Z0, torch.float64, kw)
        n32, norm32, W32, H32, Z32, _, _ = run(V, W0, H0, Z0, torch.float32, kw)
        errs = (rel(W32, W64), rel(H32, H64), rel(Z32, Z64))
        if n32 != n64 or max(errs) > SCREEN:
            raise SystemExit(f'g21 {name}: refused by the screen (n {n32} / {n64}, fp32-fp64 W {errs[0]:.2e} H {errs[1]:.2e} '
                             f'Z {errs[2]:.2e})')
        steps = [(a - b) / losses[0] for a, b in zip(losses, losses[1:])]
        if tol > 0:
            gap = min(abs(s - tol) for s in steps)
            if gap < MARGIN * tol:
                raise SystemExit(f'g21 {name}: a checkpoint is {gap:.2e} from tol {tol:g}: too close')
            print(f'g21 {name}: stop at n = {n64}; last steps {steps[-2]:.3e}, {steps[-1]:.3e} against tol {tol:g}')
        print(f'g21 {name}: n {n64}, norm {norm64:g}, fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e} Z {errs[2]:.1e}')
        data[f'{name}_n'] = np.asarray(n64, dtype=np.int64)
        data[f'{name}_norm'] = np.asarray(norm64, dtype=np.float64)
        data[f'{name}_W'], data[f'{name}_H'], data[f'{name}_Z'] = W64.numpy(), H64.numpy(), Z64.numpy()
        data[f'{name}_losses'] = np.asarray(losses, dtype=np.float64)
    path = os.path.join(OUT, 'g21_sparse_plca.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_sparse_plca.txt'), 'w') as f:
        f.write(f'g21_sparse_plca: generated by `python tools/make_golden_sparse_plca.py{"".join(" " + a for a in sys.argv[1:])}` '
                f'from torchnmf {torchnmf.__version__} (the reference, imported), torch {torch.__version__}, CPU, 1 thread, '
                f'seed {SEED}.  The reference\'s PLCA.fit on the densified {N} x {C} count target (rank {R}), float64 on '
                f'fp32-rounded inputs; cases {", ".join(CASES)}.  Every case screened against the reference\'s own fp32 run '
                f'(W, H, Z within {SCREEN:g}, same last iteration); the stop case keeps every checkpoint at least '
                f'{MARGIN:g} tol away from tol.\n')
