#!/usr/bin/env python3
"""Time one iteration (W half-step + H half-step) of missing-data NMF, ``fit(..., unstored='missing')``'s engine, beside the
two things a user could do without it, in the same run on the same target:

    python tools/bench_masked.py [--out profiles/masked_fit.json]

  masked   sparse_engine.MaskedMU: two nmfmu_sp_masked_step launches (plus the finishing kernel of the split rows)
  zero     (a) sparse_engine.SparseMU on the same target -- ``unstored='zero'``, ANOTHER problem (every unstored entry is an
           observed zero): closed-form / Gram denominators at beta 1 / 2, a dense N x C pass at beta 0.5
  torch    (b) the masked update from torch ops on the device: gather both factors' rows per stored entry, elementwise g,
           two ``index_add_`` per side, elementwise apply

Fixed inputs: 65 536 x 16 384, 10 M stored entries whose row and column degrees follow a power law (probability ~ k^-1/2 over
a random order), rank 64, beta in {1, 2, 0.5}; values uniform in [0.1, 1.1), factors uniform in [0.05, 1.05).  Device events,
2 warm-up iterations, then the median of 10 with min - max; the three paths alternate.

``gather_bytes`` per iteration: each half-step reads index + value (8 B) and ONE panel row (4 R B) per stored entry -- the row
feeds the dot product and both accumulators from registers -- and reads and writes its owner (8 R B per owner row).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.constants import eps as EPS  # noqa: E402
from torchnmf_amd.engine import mu_gamma  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from torchnmf_amd.sparse_engine import MaskedMU, SparseMU  # noqa: E402

N, C, NNZ, R = 65536, 16384, 10_000_000, 64
BETAS = (1.0, 2.0, 0.5)
WARMUP, REPEATS = 2, 10


def make_target(dev, seed=2):
    g = torch.Generator(device=dev).manual_seed(seed)
    draw = int(NNZ * 1.5)

    def axis(n):
        w = torch.arange(1, n + 1, device=dev, dtype=torch.float32).pow(-0.5)
        return torch.randperm(n, generator=g, device=dev)[torch.multinomial(w, draw, replacement=True, generator=g)]
    lin = torch.unique(axis(N) * C + axis(C))
    assert lin.numel() >= NNZ, lin.numel()
    lin = lin[torch.randperm(lin.numel(), generator=g, device=dev)[:NNZ]]
    vals = torch.rand(NNZ, generator=g, device=dev) + 0.1
    return torch.sparse_coo_tensor(torch.stack([lin // C, lin % C]), vals, (N, C)).coalesce()


def degree_stats(T):
    out = {}
    for name, ptr in (('row', T.csr[0]), ('col', T.csc[0])):
        d = torch.diff(ptr.long()).float()
        out[name] = dict(max=int(d.max()), median=float(d.median()), mean=float(d.mean()), empty=int((d == 0).sum()))
    return out


def torch_masked_iteration(rows, cols, vals, H, W, beta):
    """The same update from torch ops (no regulariser)."""
    gamma = mu_gamma(beta)
    for owner, panel, oi, pi in ((W, H, cols, rows), (H, W, rows, cols)):
        b = panel[pi]
        s = (owner[oi] * b).sum(1)
        if beta == 2.0:
            gn, gp = vals, s
        elif beta == 1.0:
            gn, gp = vals / (s + EPS), None
        else:
            se = s + EPS
            gn, gp = vals * se.pow(beta - 2), se.pow(beta - 1)
        num = torch.zeros_like(owner).index_add_(0, oi, gn[:, None] * b)
        den = torch.zeros_like(owner).index_add_(0, oi, b if gp is None else gp[:, None] * b)
        mult = (num.relu_() + EPS) / (den.relu_() + EPS)
        owner.mul_(mult if gamma == 1 else mult.pow_(gamma))


def timed(fns):
    for _ in range(WARMUP):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(REPEATS):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return times


def summary(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'masked_fit.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    V = make_target(dev)
    T = SparseTarget(V)
    rows, cols = V.indices()[0].contiguous(), V.indices()[1].contiguous()
    vals = V.values().float().contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    H0 = torch.rand(N, R, generator=g, device=dev) + 0.05
    W0 = torch.rand(C, R, generator=g, device=dev) + 0.05
    gather_bytes = 2 * NNZ * (8 + 4 * R) + (N + C) * R * 8
    res = dict(tool='tools/bench_masked.py', device=torch.cuda.get_device_name(0), shape=[N, C], nnz=NNZ, rank=R,
               warmup=WARMUP, repeats=REPEATS, chunk=T.chunk, degrees=degree_stats(T),
               segments=dict(h=T.seg_h.shape[0], w=T.seg_w.shape[0]), split_rows=dict(h=T.multi_h.shape[0], w=T.multi_w.shape[0]),
               gather_bytes_per_iteration=gather_bytes, betas={})
    for beta in BETAS:
        # one iteration from the same factors: the kernel and the torch ops compute the same update
        Hm, Wm, Ht, Wt = H0.clone(), W0.clone(), H0.clone(), W0.clone()
        em = MaskedMU(T, Wm, Hm, beta)
        em.w_step()
        em.h_step()
        torch_masked_iteration(rows, cols, vals, Ht, Wt, beta)
        agree = dict(H=float((Hm - Ht).norm() / Ht.norm()), W=float((Wm - Wt).norm() / Wt.norm()))
        # timing: every path keeps iterating on its own factors (a few iterations from the start; the work per iteration
        # does not depend on the values)
        Hz, Wz = H0.clone(), W0.clone()
        ez = SparseMU(V, Wz, Hz, beta)

        def masked():
            em.w_step()
            em.h_step()

        def zero():
            ez.w_step()
            ez.h_step()

        def torch_ops():
            torch_masked_iteration(rows, cols, vals, Ht, Wt, beta)
        tm, tz, tt = timed([masked, zero, torch_ops])
        med = statistics.median(tm)
        entry = dict(masked=summary(tm), zero=summary(tz), torch=summary(tt), masked_tb_per_s=gather_bytes / med / 1e9,
                     zero_over_masked=statistics.median(tz) / med, torch_over_masked=statistics.median(tt) / med,
                     one_iteration_rel_diff_vs_torch=agree, masked_loss=em.divergence())
        res['betas'][f'{beta:g}'] = entry
        print(f'beta {beta:g}', json.dumps(entry), flush=True)
        del ez
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
