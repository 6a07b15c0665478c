"""Time the batched Hoyer projection (hoyer.hoyer_project -> nmfmu_hoyer_project) against the per-slice torch-op loop it replaces.

    python tools/bench_hoyer.py [--warmup 20] [--iters 100] [--loop-warmup 3] [--loop-iters 20] [--out profiles/hoyer_project.json]

Shapes: W 65536 x 128 (dim 1: 128 slices of 65536 elements, streamed residency) and H 4096 x 128 (128 slices of 4096, LDS
residency), s = |randn|, every slice projected to sparseness 0.4 at its own L2 norm -- the projection of one constrained
half-step of sparse_fit / one try of SparsityProj.
  kernel      one hoyer_project call on the whole factor (targets are device tensors, no host sync inside)
  torch_loop  the same projection written as the sequence of torch ops a torchnmf user gets after .cuda(): a Python loop over
              the columns, each column's while-loop reading its step and its "any negative?" back to the host every pass
Both sides run in the same process on the same inputs; every timed call is bracketed by hipEvents after warm-up, the input is
restored before the first event.  The loop is timed over fewer calls (it takes tens of milliseconds per call and more).
Prints one JSON line: median / min / max milliseconds per call, the passes the kernel made, the speed-up (ratio of medians)
and the relative Frobenius difference between the two results.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pytorch-nmf_amd'))
from torchnmf_amd import hoyer  # noqa: E402

SIGMA = 0.4


def timed(fn, restore, warmup, iters):
    for _ in range(warmup):
        restore()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'iters': iters}


def torch_loop_project(x, k1, k2):
    """Column by column with torch ops on the device, host decisions as the eager formulation needs them."""
    k1, k2 = k1.tolist(), k2.tolist()
    for j in range(x.shape[1]):
        v = x[:, j].clone()
        n = v.numel()
        v += (k1[j] - v.sum()) / n
        fixed = torch.zeros(n, dtype=torch.bool, device=x.device)
        while True:
            mid = k1[j] / (n - fixed.count_nonzero())
            w = torch.where(fixed, v, v - mid)
            a, b, c = w @ w, 2 * (w @ v), v @ v - k2[j]
            alpha = (-b + (b * b - 4 * a * c).clamp_min(0).sqrt()) / (2 * a)
            v.add_(w, alpha=alpha.item())                  # host sync
            neg = v < 0
            if not bool(neg.any()):                        # host sync
                break
            fixed |= neg
            v.clamp_min_(0)
            v += (k1[j] - v.sum()) / (n - fixed.count_nonzero())
            v.clamp_min_(0)
        x[:, j] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--loop-warmup', type=int, default=3)
    ap.add_argument('--loop-iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/bench_hoyer.py', 'device': torch.cuda.get_device_name(0), 'sparsity': SIGMA, 'shapes': {}}
    for name, rows, cols in (('W_65536x128', 65536, 128), ('H_4096x128', 4096, 128)):
        g = torch.Generator(device=dev).manual_seed(rows)
        x0 = torch.randn(rows, cols, device=dev, generator=g).abs()
        norms = hoyer.slice_norms(x0, 1)
        k1, k2 = (rows ** 0.5 * (1 - SIGMA) + SIGMA) * norms, norms * norms
        x = x0.clone()
        keep = {}

        def restore():
            x.copy_(x0)

        def kernel():
            keep['status'] = hoyer.project_(x, k1, k2, 1)

        def loop():
            torch_loop_project(x, k1, k2)
        with torch.no_grad():
            res_k = timed(kernel, restore, a.warmup, a.iters)
            got_k = x.clone()
            res_l = timed(loop, restore, a.loop_warmup, a.loop_iters)
            got_l = x.clone()
            res_k2 = timed(kernel, restore, a.warmup, a.iters)          # again after the loop: the spread between two windows
        st = keep['status'].float()
        out['shapes'][name] = {
            'rows': rows, 'slices': cols,
            'residency': 'lds' if rows <= hoyer.LDS_MAX_ELEMS else 'streamed',
            'kernel': res_k, 'kernel_second_window': res_k2, 'torch_loop': res_l,
            'speedup': res_l['median_ms'] / res_k['median_ms'],
            'kernel_passes': {'min': int(st.min()), 'max': int(st.max()), 'mean': float(st.mean())},
            'rel_difference': float((got_k.double() - got_l.double()).norm() / got_l.double().norm()),
        }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
