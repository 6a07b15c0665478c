#!/usr/bin/env python3
"""Time one iteration (W half-step + H half-step) of weighted NMF, ``fit(V, weights=M)``'s engine, beside the two routes a user
has without it, on the same 4096 x 65536 target:

    python tools/bench_weighted.py [--out profiles/weighted_fit.json]

  weighted   wmu.WeightedMU: two nmfmu_wmu_step calls (the fused exact-fp32 MFMA kernel + the finishing kernel), once with a
             0 / 1 mask that keeps half of V and once with real weights in [0.25, 4) -- the work does not depend on the weights
  masked     sparse_engine.MaskedMU on ``V.sparse_mask(mask)`` (``unstored='missing'``) for masks that keep 0.5, 0.1 and 0.02
             of V: one gathered panel row per stored entry, O(nnz R)
  dense      the UNWEIGHTED fit's engine in 'bf16x3' (engine.DenseMU): another problem, shown for the cost of the weights

Ranks 64 and 128, beta in {1, 2, 0.5}; values uniform in [0.1, 1.1), factors uniform in [0.05, 1.05).  Device events, 2 warm-up
iterations, then the median of 10 with min - max.  ``fraction_of_fp32_mfma_peak`` counts 12 N C R flop per iteration (y, num
and den, both sides) against 157.3 TFLOP/s; ``peak_allocated_bytes`` is torch's high-water mark of the work item.

Every work item runs in a child process of its own under its own time limit; the items run one after the other, the first
that fails ends the run (no retries), and what finished is still written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))

N, C = 4096, 65536
RANKS = (64, 128)
BETAS = (1.0, 2.0, 0.5)
DENSITIES = (0.5, 0.1, 0.02)
WARMUP, REPEATS = 2, 10
FP32_MFMA_PEAK = 157.3e12
ITEMS = ['weighted', 'dense'] + [f'masked_{d:g}' for d in DENSITIES]
ITEM_LIMIT_S = 300


def timed(step):
    import torch
    for _ in range(WARMUP):
        step()
    ts = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def run_item(item):
    import torch
    from torchnmf_amd import _capi
    dev = torch.device('cuda:0')
    _capi.load()
    g = torch.Generator(device=dev).manual_seed(3)
    V = torch.rand(N, C, generator=g, device=dev) + 0.1
    keep = torch.rand(N, C, generator=g, device=dev)              # mask of density d: keep < d (nested masks)
    out = dict(item=item, rows=[])

    def factors(R):
        gf = torch.Generator(device=dev).manual_seed(1)
        return torch.rand(C, R, generator=gf, device=dev) + 0.05, torch.rand(N, R, generator=gf, device=dev) + 0.05

    def both(eng):
        def step():
            eng.w_step()
            eng.h_step()
        return step

    if item == 'weighted':
        from torchnmf_amd.wmu import WeightedMU, WeightedTarget
        gw = torch.Generator(device=dev).manual_seed(5)
        real = (torch.rand(N, C, generator=gw, device=dev) * 3.75 + 0.25) * (keep < 0.7)
        for kind, Mw in (('mask_0.5', (keep < 0.5).float()), ('real', real)):
            T = WeightedTarget(V, Mw)
            for R in RANKS:
                for beta in BETAS:
                    W, H = factors(R)
                    torch.cuda.reset_peak_memory_stats()
                    eng = WeightedMU(T, None, W, H, beta)
                    t = timed(both(eng))
                    t.update(path='weighted', weights=kind, rank=R, beta=beta, loss=eng.divergence(),
                             fraction_of_fp32_mfma_peak=12.0 * N * C * R / (t['median_ms'] * 1e-3) / FP32_MFMA_PEAK,
                             peak_allocated_bytes=torch.cuda.max_memory_allocated())
                    out['rows'].append(t)
                    print(json.dumps(t), flush=True)
            del T
    elif item == 'dense':
        from torchnmf_amd.engine import DenseMU
        for R in RANKS:
            for beta in BETAS:
                W, H = factors(R)
                torch.cuda.reset_peak_memory_stats()
                eng = DenseMU(V, W, H, beta, precision='bf16x3')
                t = timed(both(eng))
                t.update(path='dense_bf16x3', rank=R, beta=beta, peak_allocated_bytes=torch.cuda.max_memory_allocated())
                out['rows'].append(t)
                print(json.dumps(t), flush=True)
                del eng
    else:
        from torchnmf_amd.metrics import SparseTarget
        from torchnmf_amd.sparse_engine import MaskedMU
        density = float(item.split('_')[1])
        torch.cuda.reset_peak_memory_stats()
        Vs = V.sparse_mask((keep < density).float().to_sparse().coalesce())
        del keep
        T = SparseTarget(Vs)
        for R in RANKS:
            for beta in BETAS:
                W, H = factors(R)
                eng = MaskedMU(T, W, H, beta)
                t = timed(both(eng))
                t.update(path='masked', density=density, nnz=T.nnz, rank=R, beta=beta, loss=eng.divergence(),
                         peak_allocated_bytes=torch.cuda.max_memory_allocated())
                out['rows'].append(t)
                print(json.dumps(t), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weighted_fit.json'))
    ap.add_argument('--item', choices=ITEMS, help='run ONE work item in this process and print its rows (the driver calls this)')
    a = ap.parse_args()
    if a.item:
        print('ITEM_RESULT ' + json.dumps(run_item(a.item)), flush=True)
        return 0
    res = dict(tool='tools/bench_weighted.py', shape=[N, C], ranks=list(RANKS), betas=list(BETAS), warmup=WARMUP,
               repeats=REPEATS, flop_per_iteration='12 N C R', fp32_mfma_peak=FP32_MFMA_PEAK, rows=[], failed=None)
    rc = 0
    for item in ITEMS:              # chained: the first failure ends the run, nothing is tried again
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--item', item], capture_output=True, text=True,
                               timeout=ITEM_LIMIT_S)
        except subprocess.TimeoutExpired:
            res['failed'], rc = dict(item=item, why=f'time limit of {ITEM_LIMIT_S} s'), 124
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('ITEM_RESULT ')]
        if p.returncode != 0 or not line:
            res['failed'], rc = dict(item=item, why=f'exit status {p.returncode}', stderr=p.stderr[-2000:]), p.returncode or 1
            break
        rows = json.loads(line[-1][len('ITEM_RESULT '):])['rows']
        res['rows'] += rows
        for r in rows:
            print(json.dumps(r), flush=True)
    if rc == 0:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
        # the density at which the fused dense kernel overtakes the gather kernel, per (rank, beta): linear in nnz between the
        # two measured densities that bracket the weighted time
        cross = []
        for R in RANKS:
            for beta in BETAS:
                w = next(r for r in res['rows'] if r['path'] == 'weighted' and r['weights'] == 'mask_0.5' and r['rank'] == R
                         and r['beta'] == beta)['median_ms']
                m = sorted((r['density'], r['median_ms']) for r in res['rows'] if r['path'] == 'masked' and r['rank'] == R
                           and r['beta'] == beta)
                at = None
                for (d0, t0), (d1, t1) in zip(m, m[1:]):
                    if t0 <= w <= t1:
                        at = d0 + (d1 - d0) * (w - t0) / (t1 - t0)
                cross.append(dict(rank=R, beta=beta, weighted_ms=w, masked_ms={f'{d:g}': t for d, t in m},
                                  crossover_density=at, note=None if at is not None else
                                  ('masked is faster at every measured density' if m[-1][1] < w else
                                   'weighted is faster at every measured density')))
        res['crossover'] = cross
        print(json.dumps(cross), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return rc


if __name__ == '__main__':
    sys.exit(main())
