"""Time the backward of the PLCA reconstructions (nmfmu_plca_backward / nmfmu_conv_plca_backward) against the composition that
was available before them.

    python tools/bench_plca_autograd.py [--shapes plca,siplca] [--iters 10] [--out profiles/plca_autograd_backward.json]

Shapes: plca = target 4096 x 65536, rank 128;  siplca = target (1, 1025, 8192), rank 8, T = 400.  G is randn of the target's
shape, the factors are rand, Z is rand.

Both sides run in the same process on the same inputs through the C ABI, every call bracketed by hipEvents after warm-up,
outputs and scratch allocated outside the timed region:
  new          ONE call for all three gradients; also grad_H alone, grad_W alone and grad_H + grad_W (no grad_Z)
  composition  nmfmu_reconstruct_backward / nmfmu_conv_backward for the unscaled products (both, and each half alone), then
               torch: rawH * Z, rawW * Z, (rawW * W).sum(all but the rank axis)
Prints one JSON line: median / min / max milliseconds and, per half, the bytes the finishing kernel moves (parts + the factor
when it feeds grad_Z, read; the gradient, written) with
  finish_minus_slab_sum_ms = new(half alone) - old entry(half alone): the finishing pass IN PLACE of the old slab-sum pass (a
  half in one part had no slab-sum pass: there the difference is the finishing kernel itself, and bytes / difference is its
  rate, reported as a fraction of 8 TB/s).  Differences of medians of whole calls: exact per-kernel times come from a
  kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_plca_autograd.py).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pytorch-nmf_amd'))
from torchnmf_amd import _capi  # noqa: E402

HBM_PEAK = 8e12

# name -> (H shape, W shape)
SHAPES = {'plca': ((4096, 128), (65536, 128)),
          'siplca': ((1, 8, 8192 - 400 + 1), (1025, 8, 400))}


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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    def __init__(self, hs, ws, dev):
        self.lib = _capi.load()
        g = torch.Generator(device=dev).manual_seed(0)
        self.H, self.W = torch.rand(*hs, device=dev, generator=g), torch.rand(*ws, device=dev, generator=g)
        self.Z = torch.rand(hs[1], device=dev, generator=g)
        self.dense = len(hs) == 2
        if self.dense:
            gs = (hs[0], ws[0])
        else:
            gs = (hs[0], ws[0]) + tuple(a + t - 1 for a, t in zip(hs[2:], ws[2:]))
            self.nd = len(hs) - 2
            self.lh, self.taps = (C.c_int32 * self.nd)(*hs[2:]), (C.c_int32 * self.nd)(*ws[2:])
        self.G = torch.randn(*gs, device=dev, generator=g)
        self.gH, self.gW, self.gZ = torch.empty_like(self.H), torch.empty_like(self.W), torch.empty_like(self.Z)
        self.rawH, self.rawW = torch.empty_like(self.H), torch.empty_like(self.W)
        self.zv = self.Z.view(1, -1, *([1] * (self.W.dim() - 2)))
        self.sum_dims = [d for d in range(self.W.dim()) if d != 1]
        self.info = (C.c_int * 5)()
        n_new = self.new_ws(1, 1, 1, self.info)
        n_old = self.old_ws(1, 1)
        self.ws = torch.empty(max(n_new, n_old, 1), dtype=torch.float32, device=dev)

    def new_ws(self, h, w, z, info=None):
        if self.dense:
            return self.lib.nmfmu_plca_backward_ws(self.H.shape[0], self.W.shape[0], self.H.shape[1], h, w, z, info)
        return self.lib.nmfmu_conv_plca_backward_ws(self.H.shape[0], self.W.shape[0], self.H.shape[1], self.nd, self.lh, self.taps,
                                                    h, w, z, info)

    def old_ws(self, h, w):
        if self.dense:
            return self.lib.nmfmu_reconstruct_backward_ws(self.H.shape[0], self.W.shape[0], self.H.shape[1], h, w, None)
        return self.lib.nmfmu_conv_backward_ws(self.H.shape[0], self.W.shape[0], self.H.shape[1], self.nd, self.lh, self.taps, h, w,
                                               None)

    def new(self, h, w, z):
        gh, gw, gz = (self.gH if h else None), (self.gW if w else None), (self.gZ if z else None)
        if self.dense:
            m, k, R = self.H.shape[0], self.W.shape[0], self.H.shape[1]
            _capi.check(self.lib.nmfmu_plca_backward(self.G.data_ptr(), k, m, k, self.H.data_ptr(), self.W.data_ptr(),
                                                     self.Z.data_ptr(), R, _ptr(gh), _ptr(gw), _ptr(gz), self.ws.data_ptr(),
                                                     _stream()), 'nmfmu_plca_backward')
        else:
            _capi.check(self.lib.nmfmu_conv_plca_backward(self.G.data_ptr(), self.W.data_ptr(), self.H.data_ptr(), self.Z.data_ptr(),
                                                          self.H.shape[0], self.W.shape[0], self.H.shape[1], self.nd, self.lh,
                                                          self.taps, _ptr(gh), _ptr(gw), _ptr(gz), self.ws.data_ptr(), _stream()),
                        'nmfmu_conv_plca_backward')

    def old(self, h, w):
        rh, rw = (self.rawH if h else None), (self.rawW if w else None)
        if self.dense:
            m, k, R = self.H.shape[0], self.W.shape[0], self.H.shape[1]
            _capi.check(self.lib.nmfmu_reconstruct_backward(self.G.data_ptr(), k, m, k, self.H.data_ptr(), self.W.data_ptr(), R,
                                                            _ptr(rh), _ptr(rw), self.ws.data_ptr(), _stream()),
                        'nmfmu_reconstruct_backward')
        else:
            _capi.check(self.lib.nmfmu_conv_backward(self.G.data_ptr(), self.W.data_ptr(), self.H.data_ptr(), self.H.shape[0],
                                                     self.W.shape[0], self.H.shape[1], self.nd, self.lh, self.taps, _ptr(rh),
                                                     _ptr(rw), self.ws.data_ptr(), _stream()), 'nmfmu_conv_backward')

    def composition(self):
        self.old(1, 1)
        self.cH = self.rawH * (self.Z if self.dense else self.zv)
        self.cW = self.rawW * (self.Z if self.dense else self.zv)
        self.cZ = (self.rawW * self.W).sum(self.sum_dims)


def run_shape(name, warmup, iters, dev):
    hs, ws = SHAPES[name]
    c = Case(hs, ws, dev)
    res = {}
    with torch.no_grad():
        for tag, fn in (('new_all', lambda: c.new(1, 1, 1)), ('composition_all', c.composition),
                        ('new_grad_H', lambda: c.new(1, 0, 0)), ('new_grad_W', lambda: c.new(0, 1, 0)),
                        ('new_grad_H_grad_W', lambda: c.new(1, 1, 0)), ('new_grad_W_grad_Z', lambda: c.new(0, 1, 1)),
                        ('old_products_both', lambda: c.old(1, 1)), ('old_product_H', lambda: c.old(1, 0)),
                        ('old_product_W', lambda: c.old(0, 1))):
            res[tag] = timed(fn, warmup, iters)
        c.composition()
        c.new(1, 1, 1)
        torch.cuda.synchronize()
        diff = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in (('grad_H', c.gH, c.cH), ('grad_W', c.gW, c.cW),
                                                                               ('grad_Z', c.gZ, c.cZ))}
    parts_h, parts_w, blocks_h, blocks_w, z_half = list(c.info)
    med = lambda k: res[k]['median_ms']
    halves = {}
    for half, parts, blocks, plane, new_k, old_k, with_z in (('H', parts_h, blocks_h, c.H.numel(), 'new_grad_H', 'old_product_H', None),
                                                            ('W', parts_w, blocks_w, c.W.numel(), 'new_grad_W', 'old_product_W',
                                                             'new_grad_W_grad_Z')):
        d_ms = med(new_k) - med(old_k)
        entry = {'parts': parts, 'finishing_workgroups': blocks, 'bytes_gradient_only': 4 * plane * (parts + 1),
                 'bytes_with_grad_Z': 4 * plane * (parts + 2), 'finish_minus_slab_sum_ms': d_ms}
        if parts == 1 and d_ms > 0:
            entry['finish_rate_fraction_of_8TBps'] = entry['bytes_gradient_only'] / (d_ms * 1e-3) / HBM_PEAK
        if with_z:
            dz = med(with_z) - med(old_k)
            entry['finish_with_grad_Z_minus_slab_sum_ms'] = dz
            if parts == 1 and dz > 0:
                entry['finish_with_grad_Z_rate_fraction_of_8TBps'] = entry['bytes_with_grad_Z'] / (dz * 1e-3) / HBM_PEAK
        halves[half] = entry
    return {'H_shape': list(hs), 'W_shape': list(ws), 'G_shape': list(c.G.shape), 'grad_Z_half': 'HW'[z_half - 1], 'timing': res,
            'speedup_over_composition': med('composition_all') / med('new_all'), 'halves': halves,
            'max_rel_difference_to_composition': diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='plca,siplca')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/bench_plca_autograd.py', 'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': HBM_PEAK,
           'shapes': {}}
    for name in a.shapes.split(','):
        out['shapes'][name] = run_shape(name, a.warmup, a.iters, dev)
        print(f'# {name} done', file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
