#!/usr/bin/env python3
"""Time ``fit(solver='ccd', unstored=omega)`` beside its two end points in the same run on the same target:

    python tools/bench_wccd.py [--out profiles/wccd.json] [--omega 0.05]

  65 536 x 16 384, 10 M stored entries, rank 64 (the target of tools/bench_ccd.py): wccd.WeightedCcdEngine against
  ccd.CcdEngine (omega = 0: the unstored entries are missing) and hals.HalsEngine (omega = 1: they are observed zeros) -- ms
  per iteration, the three alternating; then each side's sweep on its own -- the weighted sweep with its Gram matrix ready,
  ``nmfmu_gram`` on that side's panel, and the unweighted sweep of ``ccd._Side`` -- alternating as well.

Device events; 2 warm-up calls, then the median of 10 with min - max.
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
from bench_hals import factors, iteration  # noqa: E402
from bench_masked import C, N, NNZ, R, degree_stats, make_target, summary, timed  # noqa: E402
from torchnmf_amd import _capi, ccd, hals, wccd  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402


def sweeps(T, W, H, omega):
    """Each side's sweep alone on a copy of its factor: weighted (Gram matrix ready), the Gram matrix, unweighted."""
    out = {}
    for side, own, pan in (('h', H, W), ('w', W, H)):
        ws, cs = wccd._WSide(T, side, R), ccd._Side(T, side, R)
        F = own.clone()
        G = ws.make_gram(pan)
        tw, tg, tc = timed([lambda: ws.wsweep(F, pan, G, omega, 0.0, 0.0), lambda: ws.make_gram(pan),
                            lambda: cs.sweep(F, pan, 0.0, 0.0)])
        out[side] = dict(rows=own.shape[0], wccd_sweep=summary(tw), gram=summary(tg), ccd_sweep=summary(tc),
                         wccd_sweep_over_ccd_sweep=statistics.median(tw) / statistics.median(tc))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wccd.json'))
    ap.add_argument('--omega', type=float, default=0.05)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    V = make_target(dev)
    T = SparseTarget(V)
    W0, H0 = factors(N, C, R, dev)
    Ww, Hw, Wc, Hc, Wh, Hh = (x.clone() for x in (W0, H0, W0, H0, W0, H0))
    wc, cd, hl = wccd.WeightedCcdEngine(T, Ww, Hw, a.omega), ccd.CcdEngine(T, Wc, Hc), hals.HalsEngine(V, Wh, Hh)
    for e in (wc, cd, hl):
        e.divergence()                      # the initial scale
    tw, tc, th = timed([iteration(wc), iteration(cd), iteration(hl)])
    res = dict(tool='tools/bench_wccd.py', device=torch.cuda.get_device_name(0), beta=2, omega=a.omega, shape=[N, C], nnz=NNZ,
               rank=R, degrees=degree_stats(T), wccd=summary(tw), ccd=summary(tc), hals=summary(th),
               wccd_over_ccd=statistics.median(tw) / statistics.median(tc),
               wccd_over_ccd_range=[min(tw) / max(tc), max(tw) / min(tc)],
               wccd_over_hals=statistics.median(tw) / statistics.median(th))
    print(json.dumps(res), flush=True)
    res['sweep'] = sweeps(T, Ww, Hw, a.omega)
    print(json.dumps(res['sweep']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
