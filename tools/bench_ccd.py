#!/usr/bin/env python3
"""Time ``solver='ccd'`` beside the masked multiplicative update (beta = 2, unstored='missing') in the same run on the same
target:

    python tools/bench_ccd.py [--out profiles/ccd.json]

  65 536 x 16 384, 10 M stored entries, rank 64 (the target of tools/bench_masked.py): ccd.CcdEngine against
  sparse_engine.MaskedMU -- ms per iteration; each side's sweep on its own, once per panel layout ('lds': rows that fit stage
  their panel rows in LDS, the rest gather from the transposed copy; 'transposed': every row gathers from the transposed
  copy; 'direct': every row gathers from the row-major panel) -- the A/B behind ``ccd._Side``'s default -- and once per
  workgroup threshold; and the race:
  iterations and milliseconds CCD needs to reach the loss MU has after 200 iterations, from the same |randn| factors (CCD
  scales them first; that step is timed with its first iteration).

Device events; per-iteration and per-sweep times: 2 warm-up calls, then the median of 10 with min - max, the arms
alternating.  The race times every iteration on its own (the loss evaluations between CCD iterations are not counted).
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
from bench_hals import factors, iteration, one  # noqa: E402
from bench_masked import C, N, NNZ, R, degree_stats, make_target, summary, timed  # noqa: E402
from torchnmf_amd import _capi, ccd  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from torchnmf_amd.sparse_engine import MaskedMU  # noqa: E402

MU_ITERS = 200


def race(mu, cd):
    """MU for MU_ITERS iterations, then CCD until its loss is at or below MU's."""
    t_mu = sum(one(iteration(mu)) for _ in range(MU_ITERS))
    target = mu.divergence()
    t_c, n_c, loss = one(cd.divergence), 0, float('inf')           # the initial scale
    start = cd.divergence()
    trace = []
    while n_c < MU_ITERS and loss > target:
        t_c += one(iteration(cd))
        n_c += 1
        loss = cd.divergence()
        trace.append(loss)
    return dict(mu=dict(iterations=MU_ITERS, ms=t_mu, loss=target),
                ccd=dict(iterations=n_c, ms=t_c, loss=loss, loss_after_initial_scale=start, reached=loss <= target,
                         loss_per_iteration=trace[:20]),
                mu_ms_over_ccd_ms=t_mu / t_c)


def layout_ab(T, W, H):
    """Each side's sweep alone on a copy of its factor, once per layout, the layouts alternating."""
    out = {}
    for side, own, pan in (('h', H, W), ('w', W, H)):
        sides = {name: ccd._Side(T, side, R, name) for name in ('lds', 'transposed', 'direct')}
        F = own.clone()
        ts = timed([(lambda s=s: s.sweep(F, pan, 0.0, 0.0)) for s in sides.values()])
        out[side] = dict(rows=own.shape[0], lds_rows=ccd.lds_rows(R), **{name: summary(t) for name, t in zip(sides, ts)})
        # the count above which a row takes a workgroup (the default is the first): it moves rows between two summation orders
        wgs = (128, 256, ccd.RESIDENT_LIMIT, 1024, 2048, 1 << 30)
        tw = timed([(lambda w=w: sides['direct'].sweep(F, pan, 0.0, 0.0, wg_rows=w)) for w in wgs])
        out[side]['direct_by_wg_rows'] = {str(w): summary(t) for w, t in zip(wgs, tw)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ccd.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    V = make_target(dev)
    T = SparseTarget(V)
    W0, H0 = factors(N, C, R, dev)
    Wc, Hc, Wm, Hm = W0.clone(), H0.clone(), W0.clone(), H0.clone()
    cd, mu = ccd.CcdEngine(T, Wc, Hc), MaskedMU(T, Wm, Hm, 2.0)
    cd.divergence()
    tc, tm = timed([iteration(cd), iteration(mu)])
    res = dict(tool='tools/bench_ccd.py', device=torch.cuda.get_device_name(0), beta=2, unstored='missing', shape=[N, C],
               nnz=NNZ, rank=R, degrees=degree_stats(T), resident_limit=ccd.RESIDENT_LIMIT, wg_waves=ccd.WG_WAVES,
               ccd=summary(tc), mu=summary(tm), ccd_over_mu=statistics.median(tc) / statistics.median(tm),
               layouts=dict(h=cd.side_h.layout, w=cd.side_w.layout))
    print(json.dumps(res), flush=True)
    res['sweep'] = layout_ab(T, Wc, Hc)
    print(json.dumps(res['sweep']), flush=True)
    for x, y in ((Wc, W0), (Hc, H0), (Wm, W0), (Hm, H0)):
        x.copy_(y)
    res['to_mu_200_loss'] = race(mu, ccd.CcdEngine(T, Wc, Hc))
    print(json.dumps(res['to_mu_200_loss']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
