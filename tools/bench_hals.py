#!/usr/bin/env python3
"""Time ``solver='hals'`` beside the multiplicative update (beta = 2) in the same run on the same targets:

    python tools/bench_hals.py [--out profiles/hals.json]

  sparse   65 536 x 16 384, 10 M stored entries, rank 64 (the target of tools/bench_masked.py / profiles/sparse_plca.json):
           hals.HalsEngine against sparse_engine.SparseMU -- ms per iteration, the sweep kernel's own time on both sides
  dense    4096 x 65 536, rank 128: hals.HalsEngine (exact-fp32 MFMA numerators) against the engine of ``fit(beta=2)`` in
           'auto' and in 'bf16x3'

and, on both, what the feature stands on: iterations and milliseconds each solver needs to reach the loss MU has after 200
iterations, from the same |randn| factors (HALS scales them first; that step is timed with its first iteration).

Device events; per-iteration times: 2 warm-up iterations, then the median of 10 with min - max, the solvers alternating.
The time-to-loss runs time every iteration on its own (the loss evaluations between HALS iterations are not counted).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_masked import C, N, NNZ, R, make_target, summary, timed  # noqa: E402
from torchnmf_amd import _capi, hals  # noqa: E402
from torchnmf_amd.nmf import NMF  # noqa: E402
from torchnmf_amd.sparse_engine import SparseMU  # noqa: E402

DN, DC, DR = 4096, 65536, 128
MU_ITERS = 200


def one(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def iteration(eng):
    def f():
        eng.w_step()
        eng.h_step()
    return f


def race(mu, hl):
    """MU for MU_ITERS iterations, then HALS until its loss is at or below MU's."""
    t_mu = sum(one(iteration(mu)) for _ in range(MU_ITERS))
    target = mu.divergence()
    t_h, n_h, loss = one(hl.divergence), 0, float('inf')           # the initial scale
    start = hl.divergence()
    while n_h < MU_ITERS and loss > target:
        t_h += one(iteration(hl))
        n_h += 1
        loss = hl.divergence()
    return dict(mu=dict(iterations=MU_ITERS, ms=t_mu, loss=target),
                hals=dict(iterations=n_h, ms=t_h, loss=loss, loss_after_initial_scale=start, reached=loss <= target),
                mu_ms_over_hals_ms=t_mu / t_h)


def sweep_times(eng):
    """The sweep kernel alone on both sides, on copies of the factors, with the numerator and Gram matrix of the moment."""
    out = {}
    for which, own, pan in (('h', eng.H, eng.W), ('w', eng.W, eng.H)):
        A, lda = eng._numerator(which)
        eng._gram(pan, eng.gram)
        F = own.clone()
        ts, = timed([lambda: hals._sweep(F, A, lda, eng.gram, 0.0, 0.0)])
        out[which] = dict(rows=own.shape[0], **summary(ts))
    return out


def factors(n, c, r, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(c, r, generator=g, device=dev).abs(), torch.randn(n, r, generator=g, device=dev).abs())


def sparse_part(dev):
    V = make_target(dev)
    W0, H0 = factors(N, C, R, dev)
    Wh, Hh, Wm, Hm = W0.clone(), H0.clone(), W0.clone(), H0.clone()
    hl, mu = hals.HalsEngine(V, Wh, Hh), SparseMU(V, Wm, Hm, 2.0)
    hl.divergence()
    th, tm = timed([iteration(hl), iteration(mu)])
    sw = sweep_times(hl)
    res = dict(shape=[N, C], nnz=NNZ, rank=R, hals=summary(th), mu=summary(tm),
               hals_over_mu=statistics.median(th) / statistics.median(tm), sweep=sw,
               sweep_share_of_hals_iteration=(sw['h']['median_ms'] + sw['w']['median_ms']) / statistics.median(th))
    for a, b in ((Wh, W0), (Hh, H0), (Wm, W0), (Hm, H0)):
        a.copy_(b)
    res['to_mu_200_loss'] = race(mu, hals.HalsEngine(V, Wh, Hh))
    return res


def dense_part(dev):
    g = torch.Generator(device=dev).manual_seed(3)
    V = torch.rand(DN, DC, generator=g, device=dev)
    W0, H0 = factors(DN, DC, DR, dev)
    res = dict(shape=[DN, DC], rank=DR)
    Wh, Hh = W0.clone(), H0.clone()
    hl = hals.HalsEngine(V, Wh, Hh)
    hl.divergence()
    engines = {}
    for mode in ('auto', 'bf16x3'):
        m = NMF(W=W0.cpu(), H=H0.cpu()).to(dev)
        engines[mode] = (m, m._make_engine(V, 2.0, 0.0, 0.0, mode, None))
    th, ta, tb = timed([iteration(hl), iteration(engines['auto'][1]), iteration(engines['bf16x3'][1])])
    res.update(hals=summary(th), mu_auto=dict(precision=engines['auto'][1].precision_name, **summary(ta)),
               mu_bf16x3=summary(tb), hals_over_mu_auto=statistics.median(th) / statistics.median(ta),
               hals_over_mu_bf16x3=statistics.median(th) / statistics.median(tb), sweep=sweep_times(hl))
    del engines
    for mode in ('auto', 'bf16x3'):
        m = NMF(W=W0.cpu(), H=H0.cpu()).to(dev)
        Wh.copy_(W0)
        Hh.copy_(H0)
        res[f'to_mu_{mode}_200_loss'] = race(m._make_engine(V, 2.0, 0.0, 0.0, mode, None), hals.HalsEngine(V, Wh, Hh))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hals.json'))
    ap.add_argument('--only', choices=['sparse', 'dense'])
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    res = dict(tool='tools/bench_hals.py', device=torch.cuda.get_device_name(0), beta=2, mu_iterations=MU_ITERS)
    for name, part in (('sparse', sparse_part), ('dense', dense_part)):
        if a.only in (None, name):
            res[name] = part(dev)
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
