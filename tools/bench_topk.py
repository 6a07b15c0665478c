#!/usr/bin/env python3
"""Time ``scoring.topk_scores`` -- the k best unobserved columns of every row, the training target excluded -- beside the only
thing a user could do without it, in the same run on the same factors and target:

    python tools/bench_topk.py [--out profiles/topk.json]

  fused   scoring.topk_scores(H, W, k, exclude=T): nmfmu_topk (exact-fp32 MFMA GEMM fused with the selection)
  torch   on the device, in row chunks: ``H[chunk] @ W.T``, ``-inf`` written at the chunk's stored positions, ``torch.topk``
          (the chunk boundaries inside the coalesced index list are found once, outside the timed region)

Fixed inputs: 65 536 x 16 384, rank 64, the 10 M-entry power-law target of tools/bench_masked.py as ``exclude``, k in {10, 100},
all rows; factors uniform in [0.05, 1.05).  Device events, 2 warm-ups, then the median of 10 with min - max; the two paths
alternate.  Peak allocated bytes are taken per path from ``torch.cuda.max_memory_allocated`` above what is resident before the
call.  ``f32_matrix_fraction``: 2 N C R flops over the fused median, against the 155 TF measured f32 MFMA rate.

``score_pairs`` gets one line: the target's 10 M stored positions against ``(H[rows] * W[cols]).sum(1)``.
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
from torchnmf_amd import _capi, scoring  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from bench_masked import C, N, NNZ, R, REPEATS, WARMUP, make_target, summary  # noqa: E402

KS = (10, 100)
CHUNK = 4096                 # rows per baseline chunk: 4096 x 16384 fp32 = 268 MB
F32_MATRIX_TF = 155.0


def timed_with_peak(fns):
    """bench_masked.timed, plus the peak allocated bytes of each path above its starting level."""
    for _ in range(WARMUP):
        for f in fns:
            f()
    times, peaks = [[] for _ in fns], [0 for _ in fns]
    for _ in range(REPEATS):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
            peaks[i] = max(peaks[i], torch.cuda.max_memory_allocated() - base)
    return times, peaks


def overlap(a, b):
    return a['min_ms'] <= b['max_ms'] and b['min_ms'] <= a['max_ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    V = make_target(dev)
    T = SparseTarget(V)
    rows, cols = V.indices()[0].contiguous(), V.indices()[1].contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    H = torch.rand(N, R, generator=g, device=dev) + 0.05
    W = torch.rand(C, R, generator=g, device=dev) + 0.05
    starts = list(range(0, N, CHUNK))
    cuts = torch.searchsorted(rows, torch.tensor(starts + [N], device=dev)).tolist()      # coalesced: sorted by row
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    res = dict(tool='tools/bench_topk.py', device=torch.cuda.get_device_name(0), shape=[N, C], nnz=NNZ, rank=R, warmup=WARMUP,
               repeats=REPEATS, baseline_chunk_rows=CHUNK, nsplit=scoring.choose_nsplit(N, C, n_cu), ks={})

    for k in KS:
        out = {}

        def fused():
            out['fused'] = scoring.topk_scores(H, W, k, exclude=T)

        def torch_ops():
            vs, js = [], []
            for r0, p0, p1 in zip(starts, cuts[:-1], cuts[1:]):
                S = H[r0:r0 + CHUNK] @ W.T
                S[rows[p0:p1] - r0, cols[p0:p1]] = float('-inf')
                v, j = torch.topk(S, k, dim=1)
                vs.append(v)
                js.append(j)
            out['torch'] = (torch.cat(vs), torch.cat(js))
        (tf, tt), (pf, pt) = timed_with_peak([fused, torch_ops])
        fv, fi = out['fused']
        tv, ti = out['torch']
        sf, st = summary(tf), summary(tt)
        entry = dict(fused=sf, torch=st, fused_peak_bytes=pf, torch_peak_bytes=pt,
                     torch_over_fused=st['median_ms'] / sf['median_ms'], ranges_overlap=overlap(sf, st),
                     f32_matrix_fraction=2.0 * N * C * R / (sf['median_ms'] * 1e-3) / (F32_MATRIX_TF * 1e12),
                     same_indices_fraction=float((fi == ti).float().mean()),
                     max_abs_value_diff=float((fv - tv).abs().max()))
        res['ks'][str(k)] = entry
        print(f'k {k}', json.dumps(entry), flush=True)
        del out

    # the GEMM with next to no selection: k = 1, nothing excluded (informational)
    (t1,), _ = timed_with_peak([lambda: scoring.topk_scores(H, W, 1)])
    res['fused_k1_no_exclude'] = dict(summary(t1), f32_matrix_fraction=2.0 * N * C * R / (statistics.median(t1) * 1e-3)
                                      / (F32_MATRIX_TF * 1e12))
    print('k 1, no exclude', json.dumps(res['fused_k1_no_exclude']), flush=True)

    n_pairs = rows.numel()

    def pairs_fused():
        return scoring.score_pairs(H, W, rows, cols)

    def pairs_torch():
        return (H[rows] * W[cols]).sum(1)
    (tf, tt), (pf, pt) = timed_with_peak([pairs_fused, pairs_torch])
    sf, st = summary(tf), summary(tt)
    res['score_pairs'] = dict(n=n_pairs, fused=sf, torch=st, fused_peak_bytes=pf, torch_peak_bytes=pt,
                              torch_over_fused=st['median_ms'] / sf['median_ms'], ranges_overlap=overlap(sf, st),
                              max_abs_diff=float((pairs_fused() - pairs_torch()).abs().max()))
    print('score_pairs', json.dumps(res['score_pairs']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
