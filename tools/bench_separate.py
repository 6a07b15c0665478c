#!/usr/bin/env python3
"""Time ``separation.separate`` beside the loop of torch ops a user writes without it, producing the same outputs:

    python tools/bench_separate.py [--out profiles/separate.json]

  torch    per group ``Y_g = H[:, idx] @ W[:, idx].T``, a power, a running sum, then per group a division and the product with V
  planes   ``separate(..., _route='planes')``: one ``nmfmu_reconstruct`` per group into the output, ``nmfmu_separate_planes`` in place
  fused    ``separate(..., _route='fused')``: one ``nmfmu_separate`` launch

Dense 4096 x 65536, rank 128, G in {2, 4, 16} groups of equal size, power in {1, 2}, V real fp32 and complex64; factors and V
uniform / normal, seeded.  Device events, 2 warm-up runs, then the median of 10 with min - max.  ``gbps`` counts the minimum
traffic (V once + S planes once) and ``fraction_of_hbm`` holds it against 8 TB/s; for ``fused``, ``tflops`` counts
``4 N C R'`` (two walks over the padded rank R') and ``fraction_of_fp32_mfma_peak`` holds it against 157.3 TFLOP/s;
``peak_allocated_bytes`` is torch's high-water mark over the contestant's runs, inputs included.  One ``NMFD`` line at
(1, 1025, 8192), rank 8, T = 400, two groups: the torch loop over ``NMFD.reconstruct`` against the library.

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

N, C, R = 4096, 65536, 128
GROUPS = (2, 4, 16)
POWERS = (1.0, 2.0)
KINDS = ('real', 'complex')
WARMUP, REPEATS = 2, 10
HBM_PEAK, FP32_MFMA_PEAK = 8.0e12, 157.3e12
ITEMS = [f'dense_G{G}_p{p:g}_{k}' for G in GROUPS for p in POWERS for k in KINDS] + ['nmfd']
ITEM_LIMIT_S = 240
EPS = 2.0 ** -23


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


def torch_loop(H, W, V, labels, power, recon):
    import torch
    G = max(labels) + 1
    idx = [torch.tensor([r for r, lab in enumerate(labels) if lab == g], device=H.device) for g in range(G)]
    Ys = [recon(H[:, i], W[:, i]) for i in idx]
    if power == 1.0:
        D = recon(H, W)
    else:
        D = Ys[0].pow(power)
        for y in Ys[1:]:
            D += y.pow(power)
    D += EPS
    return torch.stack([V * ((y if power == 1.0 else y.pow(power)) / D) for y in Ys])


def measure(name, fn, min_bytes, extra):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t = timed(fn)
    t.update(contestant=name, gbps=min_bytes / (t['median_ms'] * 1e-3) / 1e9,
             fraction_of_hbm=min_bytes / (t['median_ms'] * 1e-3) / HBM_PEAK,
             peak_allocated_bytes=torch.cuda.max_memory_allocated(), **extra)
    return t


def run_item(item):
    import torch
    from torchnmf_amd import _capi
    from torchnmf_amd.nmf import NMF, NMFD
    from torchnmf_amd.separation import group_tables, separate
    dev = torch.device('cuda:0')
    _capi.load()
    g = torch.Generator(device=dev).manual_seed(3)
    rows = []
    if item == 'nmfd':
        B, Cc, L, Rr, T, power = 1, 1025, 8192, 8, 400, 2.0
        H = torch.rand(B, Rr, L - T + 1, generator=g, device=dev) + 0.05
        W = torch.rand(Cc, Rr, T, generator=g, device=dev) + 0.05
        V = torch.randn(B, Cc, L, generator=g, device=dev)
        labels = [r % 2 for r in range(Rr)]
        min_bytes = 4 * B * Cc * L * 3
        extra = dict(model='NMFD', shape=[B, Cc, L], rank=Rr, taps=T, groups=2, power=power, mixture='real',
                     inputs_bytes=4 * (H.numel() + W.numel() + V.numel()))
        with torch.no_grad():
            rows.append(measure('torch', lambda: torch_loop(H, W, V, labels, power, NMFD.reconstruct), min_bytes, extra))
            rows.append(measure('library', lambda: separate(H, W, V, labels, power=power), min_bytes, extra))
    else:
        _, sG, sp, kind = item.split('_')
        G, power = int(sG[1:]), float(sp[1:])
        H = torch.rand(N, R, generator=g, device=dev) + 0.05
        W = torch.rand(C, R, generator=g, device=dev) + 0.05
        V = torch.randn(N, C, generator=g, device=dev)
        if kind == 'complex':
            V = torch.complex(V, torch.randn(N, C, generator=g, device=dev))
        labels = [r * G // R for r in range(R)]
        vw = 2 if kind == 'complex' else 1
        min_bytes = 4 * vw * N * C * (1 + G)
        cols = len(group_tables(labels)[2])
        extra = dict(model='NMF', shape=[N, C], rank=R, groups=G, power=power, mixture=kind, padded_rank=cols,
                     inputs_bytes=4 * (H.numel() + W.numel() + vw * N * C))
        with torch.no_grad():
            rows.append(measure('torch', lambda: torch_loop(H, W, V, labels, power, lambda h, w: h @ w.t()), min_bytes, extra))
            rows.append(measure('planes', lambda: separate(H, W, V, labels, power=power, _route='planes'), min_bytes, extra))
            t = measure('fused', lambda: separate(H, W, V, labels, power=power, _route='fused'), min_bytes, extra)
            flops = 4.0 * N * C * cols
            t.update(tflops=flops / (t['median_ms'] * 1e-3) / 1e12,
                     fraction_of_fp32_mfma_peak=flops / (t['median_ms'] * 1e-3) / FP32_MFMA_PEAK)
            rows.append(t)
            a = separate(H, W, V, labels, power=power, _route='fused')[G - 1]
            b = separate(H, W, V, labels, power=power, _route='planes')[G - 1]
            for r in rows:
                r['fused_vs_planes_max_abs_diff_last_plane'] = float((torch.view_as_real(a - b) if vw == 2 else a - b).abs().max())
    for r in rows:
        print(json.dumps(r), flush=True)
    return dict(item=item, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'separate.json'))
    ap.add_argument('--item', choices=ITEMS, help='run ONE work item in this process and print its rows (the driver calls this)')
    a = ap.parse_args()
    if a.item:
        print('ITEM_RESULT ' + json.dumps(run_item(a.item)), flush=True)
        return 0
    res = dict(tool='tools/bench_separate.py', shape=[N, C], rank=R, groups=list(GROUPS), powers=list(POWERS), warmup=WARMUP,
               repeats=REPEATS, min_traffic='V once + S planes once', hbm_peak=HBM_PEAK, flop_fused="4 N C R'",
               fp32_mfma_peak=FP32_MFMA_PEAK, rows=[], failed=None)
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
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return rc


if __name__ == '__main__':
    sys.exit(main())
