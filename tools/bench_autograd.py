"""Time the backward of NMF.reconstruct (nmfmu_reconstruct_backward) against the composition it replaces.

    python tools/bench_autograd.py [--rows 4096] [--cols 65536] [--rank 128] [--iters 10] [--out FILE]

Both sides run in the same process on the same inputs, each launch bracketed by hipEvents after warm-up:
  new          one nmfmu_reconstruct_backward call per gradient (grad_H alone, grad_W alone) and for both at once
  composition  what trainer.BetaMu._chain_step.back() does: NMF.reconstruct(G, W.t().contiguous()) for grad_H and
               NMF.reconstruct(G.t().contiguous(), H.t().contiguous()) for grad_W (the transposes are part of it)
Prints one JSON line: median / min milliseconds, the fraction of the fp32-MFMA floor 2 N C R / 155 TFLOP/s per gradient,
and the largest difference between the two sides' results.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pytorch-nmf_amd'))
from torchnmf_amd.nmf import NMF, _reconstruct_backward, reconstruct_backward_splits  # noqa: E402

PEAK_F32_MFMA = 155e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'iters': iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--cols', type=int, default=65536)
    ap.add_argument('--rank', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    N, C, R = a.rows, a.cols, a.rank
    g = torch.Generator(device=dev).manual_seed(0)
    G = torch.randn(N, C, device=dev, generator=g)
    H, W = torch.rand(N, R, device=dev, generator=g), torch.rand(C, R, device=dev, generator=g)
    keep = {}

    def new_h():
        keep['new_h'] = _reconstruct_backward(G, H, W, True, False)[0]

    def new_w():
        keep['new_w'] = _reconstruct_backward(G, H, W, False, True)[1]

    def new_both():
        keep['new_both'] = _reconstruct_backward(G, H, W, True, True)

    def old_h():
        keep['old_h'] = NMF.reconstruct(G, W.t().contiguous())

    def old_w():
        keep['old_w'] = NMF.reconstruct(G.t().contiguous(), H.t().contiguous())

    res = {}
    with torch.no_grad():
        for name, fn in (('new_grad_H', new_h), ('new_grad_W', new_w), ('new_both', new_both),
                         ('composition_grad_H', old_h), ('composition_grad_W', old_w)):
            res[name] = timed(fn, a.warmup, a.iters)
    floor_ms = 2.0 * N * C * R / PEAK_F32_MFMA * 1e3
    so, sp = reconstruct_backward_splits(N, C, R)
    out = {
        'tool': 'tools/bench_autograd.py', 'device': torch.cuda.get_device_name(0), 'shape': {'rows': N, 'cols': C, 'rank': R},
        'splits': {'grad_H': so, 'grad_W': sp}, 'floor_ms_per_gradient': floor_ms, 'timing': res,
        'fraction_of_floor': {'grad_H': floor_ms / res['new_grad_H']['median_ms'], 'grad_W': floor_ms / res['new_grad_W']['median_ms'],
                              'both': 2 * floor_ms / res['new_both']['median_ms']},
        'speedup_over_composition': {'grad_H': res['composition_grad_H']['median_ms'] / res['new_grad_H']['median_ms'],
                                     'grad_W': res['composition_grad_W']['median_ms'] / res['new_grad_W']['median_ms']},
        'max_abs_difference': {'grad_H': float((keep['new_h'] - keep['old_h']).abs().max()),
                               'grad_W': float((keep['new_w'] - keep['old_w']).abs().max())},
        'both_equals_single': bool(torch.equal(keep['new_both'][0], keep['new_h']) and torch.equal(keep['new_both'][1], keep['new_w'])),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
