#!/usr/bin/env python3
"""Generate tests/golden/g19_sparse_autograd.npz by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden_hoyer.py:
the reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs, and only inputs
and outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_sparse_autograd.py

  (a) the reference's sparse loss V_norm + pos - neg (nmf.py: _get_V_norm, _nmf_sp_recon_beta_pos_neg) in float64 with autograd,
      on fp32-rounded inputs: target 64 x 96 with the entries of rand > 0.9 stored, rank 8, beta in {1, 2}: indices, values,
      H, W, and per beta the loss, grad_H, grad_W
  (b) the reference's trainer.SparsityProj (sparsity 0.3, beta = 2) on W and on H of an NMF on the same target, closure
      beta_div(m(), V.to_dense(), 2): 10 steps, the factors after steps 1 and 10, lr after every step

(b) is SCREENED and refused when it fails -- a condition on the fixture, not a tolerance of any test:
  * the fp32 and the fp64 run of the reference make the same number of loss evaluations, leave the same lr sequence and end
    within 1e-5 (relative Frobenius) on both factors;
  * every line-search comparison ``loss <= init_loss`` of the fp64 run is decided by a margin of at least 1e-4 of the
    positive term 1/2 sum(H^T H * W^T W) of the two evaluations compared (the larger one): three orders above the fp32
    rounding of that term, so that no evaluation order of the loss can flip a decision.
"""
import os
import sys

import numpy as np
import torch

if os.environ.get('NMF_REFERENCE'):
    sys.path.insert(0, os.environ['NMF_REFERENCE'])
import torchnmf  # noqa: E402
from torchnmf import nmf as ref_nmf  # noqa: E402
from torchnmf import trainer as ref_trainer  # noqa: E402
from torchnmf.constants import eps as REF_EPS  # noqa: E402
from torchnmf.metrics import beta_div as ref_beta_div  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
SCREEN = 1e-5
MARGIN = 1e-4
SEED = 0


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def problem():
    torch.manual_seed(SEED)
    V = torch.rand(64, 96)
    W0, H0 = torch.randn(96, 8).abs(), torch.randn(64, 8).abs()
    Vs = torch.where(V > 0.9, V, torch.zeros(())).to_sparse().coalesce()
    return Vs, W0, H0


def part_a(Vs, W0, H0):
    out = {}
    V64 = Vs.double().coalesce()
    for beta in (1, 2):
        H = H0.double().requires_grad_()
        W = W0.double().requires_grad_()
        pos, neg = ref_nmf._nmf_sp_recon_beta_pos_neg(V64, H, W, float(beta), float(REF_EPS))
        loss = ref_nmf._get_V_norm(V64, beta) + pos - neg
        loss.backward()
        out[f'a_loss_b{beta}'] = np.asarray(loss.item(), dtype=np.float64)
        out[f'a_gH_b{beta}'] = H.grad.numpy().copy()
        out[f'a_gW_b{beta}'] = W.grad.numpy().copy()
        print(f'g19 (a) beta {beta}: loss {loss.item():.12g}')
    return out


def part_b(Vs, W0, H0):
    out = {}
    Vd32 = Vs.to_dense()
    for attr in ('W', 'H'):
        runs = []
        for dt in (torch.float32, torch.float64):
            m = ref_nmf.NMF(W=W0, H=H0).to(dt)
            Vd = Vd32.to(dt)
            tr = ref_trainer.SparsityProj([getattr(m, attr)], 0.3)
            evals = []          # (loss, positive term) of every evaluation

            def closure():
                tr.zero_grad()
                loss = ref_beta_div(m(), Vd, 2)
                with torch.no_grad():
                    Hd, Wd = m.H.double(), m.W.double()
                    pos = 0.5 * float(((Hd.T @ Hd) * (Wd.T @ Wd)).sum())
                evals.append((float(loss), pos))
                return loss
            lrs, snaps, margins = [], {}, []
            for step in range(1, 11):
                first = len(evals)
                tr.step(closure)
                lrs.append(float(tr.param_groups[0]['lr']))
                init_loss, init_pos = evals[first]
                for loss, pos in evals[first + 1:]:
                    margins.append(abs(loss - init_loss) / max(pos, init_pos))
                if step in (1, 10):
                    snaps[step] = (m.W.detach().clone(), m.H.detach().clone())
            runs.append((lrs, len(evals), snaps, min(margins)))
        (lr32, ev32, s32, _), (lr64, ev64, s64, margin) = runs
        errs = [rel(s32[10][k], s64[10][k]) for k in (0, 1)]
        if lr32 != lr64 or ev32 != ev64 or max(errs) > SCREEN or margin < MARGIN:
            raise SystemExit(f'g19 (b) {attr}: refused by the screen (lr {lr32} vs {lr64}, evaluations {ev32} vs {ev64}, '
                             f'fp32-fp64 {errs}, smallest margin {margin:.2e})')
        print(f'g19 (b) {attr}: {ev32} evaluations, lr[-1] {lr32[-1]:.6g}, fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e}, '
              f'smallest line-search margin {margin:.2e} of the positive term')
        out[f'b_{attr}_lr'] = np.asarray(lr32, dtype=np.float64)
        for step in (1, 10):
            out[f'b_{attr}_W{step}'] = s32[step][0].numpy()
            out[f'b_{attr}_H{step}'] = s32[step][1].numpy()
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    Vs, W0, H0 = problem()
    data = dict(shape=np.asarray(Vs.shape, dtype=np.int64), indices=Vs.indices().numpy(), values=Vs.values().numpy(),
                W0=W0.numpy(), H0=H0.numpy())
    data.update(part_a(Vs, W0, H0))
    data.update(part_b(Vs, W0, H0))
    path = os.path.join(OUT, 'g19_sparse_autograd.npz')
    np.savez_compressed(path, **data)
    print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_sparse_autograd.txt'), 'w') as f:
        f.write(f'g19_sparse_autograd: generated by `python tools/make_golden_sparse_autograd.py'
                f'{"".join(" " + a for a in sys.argv[1:])}` from torchnmf {torchnmf.__version__} (the reference, imported), '
                f'torch {torch.__version__}, CPU, 1 thread, seed {SEED}.  (a) float64 loss and gradients of the reference\'s sparse '
                f'loss on fp32-rounded inputs; (b) fp32 SparsityProj runs of the reference, screened against an fp64 run from the '
                f'same initial factors (same number of loss evaluations, same lr sequence, final factors within {SCREEN:g}, '
                f'every line-search comparison decided by at least {MARGIN:g} of the positive term)\n')
