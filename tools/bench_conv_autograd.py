"""Time the backward of the convolutive reconstruction (nmfmu_conv_backward) against the composition of existing entries.

    python tools/bench_conv_autograd.py [--shapes nmfd,nmf2d] [--iters 10] [--out FILE]

Shapes (bench.py's convolutive workloads): nmfd = target (1, 1025, 8192), rank 8, T = 400;  nmf2d = target (1, 64, 256, 512),
rank 8, kernel 8 x 16.  G is randn of the target's shape, the factors are rand.

Both sides run in the same process on the same inputs, every call bracketed by hipEvents after warm-up, buffers allocated
outside the timed region:
  new          one nmfmu_conv_backward call per gradient (grad_H alone, grad_W alone) and for both at once
  composition  what the C ABI offered before, in its fp32-grade mode (split bf16):
               grad_W: nmfmu_pack2d(G -> [c][(b,l)] planes), nmfmu_conv(nd)_unfold(H -> [(r,t)][(b,l)] planes), nmfmu_gemm,
                       slice of the [c_pad][rt_pad] product into W's layout
               grad_H: nmfmu_pack2d(G -> [(b,l)][c] planes), nmfmu_pack2d(W -> [(r,t)][c] planes), nmfmu_gemm into
                       Y[(r,t)][(b,l)], nmfmu_convnd_fold
Prints one JSON line: median / min / max milliseconds, the fraction of the fp32-MFMA floor 2 B C R prod(T) prod(L) / 155 TFLOP/s
per gradient, and the largest difference between the two sides' results (the composition rounds its operands to split bf16).
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
from torchnmf_amd.nmf import _conv_reconstruct_backward, conv_backward_splits  # noqa: E402
from torchnmf_amd.nmfd_engine import _Planes, _pad128, _ptr, _stream  # noqa: E402

PEAK_F32_MFMA = 155e12      # the figure of tools/bench_autograd.py / profiles/autograd_backward.json

# name -> (H shape, W shape)
SHAPES = {'nmfd': ((1, 8, 8192 - 400 + 1), (1025, 8, 400)),
          'nmf2d': ((1, 8, 256 - 8 + 1, 512 - 16 + 1), (64, 8, 8, 16))}


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


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


class Composition:
    """grad_H and grad_W of the convolutive reconstruction from nmfmu_pack2d / unfold / nmfmu_gemm / fold."""

    def __init__(self, G, H, W):
        self.lib = _capi.load()
        self.G, self.H, self.W = G, H, W
        dev = G.device
        self.B, self.R, self.Cc = H.shape[0], H.shape[1], W.shape[0]
        self.lh, self.taps = tuple(H.shape[2:]), tuple(W.shape[2:])
        self.nd = len(self.lh)
        self.PL, self.T = _prod(G.shape[2:]), _prod(self.taps)
        self.cp, self.blp, self.rpp = _pad128(self.Cc), _pad128(self.B * self.PL), _pad128(self.R * self.T)
        self.g_c = _Planes(self.cp, self.blp, True, dev)        # [c][(b,l)]
        self.g_bl = _Planes(self.blp, self.cp, True, dev)       # [(b,l)][c]
        self.hu = _Planes(self.blp, self.rpp, True, dev)
        self.hut = _Planes(self.rpp, self.blp, True, dev)       # [(r,t)][(b,l)]
        self.wmt = _Planes(self.rpp, self.cp, True, dev)        # [(r,t)][c]
        self.out_w = torch.empty(self.cp, self.rpp, dtype=torch.float32, device=dev)
        self.y = torch.empty(self.rpp, self.blp, dtype=torch.float32, device=dev)
        self.flat_h = torch.empty(H.numel(), dtype=torch.float32, device=dev)
        self.lh_arr, self.t_arr = (C.c_int32 * self.nd)(*self.lh), (C.c_int32 * self.nd)(*self.taps)

    def _pack(self, src, rows, cols, ri, ros, ris, ci, cos, cis, planes):
        _capi.check(self.lib.nmfmu_pack2d(src.data_ptr(), rows, cols, ri, ros, ris, ci, cos, cis, planes.rows_pad, planes.cols_pad,
                                          None, _ptr(planes.hi), _ptr(planes.lo), None, _stream()), 'nmfmu_pack2d')

    def _gemm(self, a, b, out):
        d = _capi.GemmDesc(_ptr(a.hi), _ptr(a.lo), _ptr(b.hi), _ptr(b.lo), a.rows_pad, b.rows_pad, a.cols_pad, _capi.PREC_BF16X3,
                           2.0, None, None, None, None, None, out.data_ptr(), 0, 0, _capi.OPS_PLANES, 0, 0, 0, 0)
        _capi.check(self.lib.nmfmu_gemm(C.byref(d), _capi.EPI_F32, _stream()), 'nmfmu_gemm')

    def grad_w(self):
        B, R, Cc, PL, T = self.B, self.R, self.Cc, self.PL, self.T
        self._pack(self.G, Cc, B * PL, 1, PL, 0, PL, Cc * PL, 1, self.g_c)
        if self.nd == 1:
            _capi.check(self.lib.nmfmu_conv_unfold(self.H.data_ptr(), B, R, self.lh[0], T, _ptr(self.hu.hi), _ptr(self.hu.lo),
                                                   _ptr(self.hut.hi), _ptr(self.hut.lo), self.blp, self.rpp, _stream()),
                        'nmfmu_conv_unfold')
        else:
            _capi.check(self.lib.nmfmu_convnd_unfold(self.H.data_ptr(), B, R, self.nd, self.lh_arr, self.t_arr, _ptr(self.hu.hi),
                                                     _ptr(self.hu.lo), _ptr(self.hut.hi), _ptr(self.hut.lo), self.blp, self.rpp,
                                                     _stream()), 'nmfmu_convnd_unfold')
        self._gemm(self.g_c, self.hut, self.out_w)
        return self.out_w[:Cc, :R * T].reshape(self.W.shape).contiguous()

    def grad_h(self):
        B, R, Cc, PL, T = self.B, self.R, self.Cc, self.PL, self.T
        self._pack(self.G, B * PL, Cc, PL, Cc * PL, 1, 1, PL, 0, self.g_bl)
        self._pack(self.W, R * T, Cc, 1, 1, 0, 1, R * T, 0, self.wmt)
        self._gemm(self.wmt, self.g_bl, self.y)
        _capi.check(self.lib.nmfmu_convnd_fold(self.flat_h.data_ptr(), B, R, self.nd, self.lh_arr, self.t_arr, self.y.data_ptr(),
                                               self.blp, _stream()), 'nmfmu_convnd_fold')
        return self.flat_h.view(self.H.shape)


def run_shape(name, warmup, iters, dev):
    hs, ws = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(0)
    H, W = torch.rand(*hs, device=dev, generator=g), torch.rand(*ws, device=dev, generator=g)
    ls = tuple(a + t - 1 for a, t in zip(hs[2:], ws[2:]))
    G = torch.randn(hs[0], ws[0], *ls, device=dev, generator=g)
    comp = Composition(G, H, W)
    keep = {}

    def new_h():
        keep['new_h'] = _conv_reconstruct_backward(G, H, W, True, False)[0]

    def new_w():
        keep['new_w'] = _conv_reconstruct_backward(G, H, W, False, True)[1]

    def new_both():
        keep['new_both'] = _conv_reconstruct_backward(G, H, W, True, True)

    def old_h():
        keep['old_h'] = comp.grad_h()

    def old_w():
        keep['old_w'] = comp.grad_w()

    res = {}
    with torch.no_grad():
        for tag, fn in (('new_grad_H', new_h), ('new_grad_W', new_w), ('new_both', new_both),
                        ('composition_grad_H', old_h), ('composition_grad_W', old_w)):
            res[tag] = timed(fn, warmup, iters)
    B, R, Cc = hs[0], hs[1], ws[0]
    floor_ms = 2.0 * B * Cc * R * _prod(ws[2:]) * _prod(ls) / PEAK_F32_MFMA * 1e3
    sh, sw = conv_backward_splits(hs, ws)
    return {
        'H_shape': list(hs), 'W_shape': list(ws), 'G_shape': list(G.shape), 'splits': {'grad_H': sh, 'grad_W': sw},
        'rank_tile': 32 if R <= 32 else 128, 'floor_ms_per_gradient': floor_ms, 'timing': res,
        'fraction_of_floor': {'grad_H': floor_ms / res['new_grad_H']['median_ms'], 'grad_W': floor_ms / res['new_grad_W']['median_ms'],
                              'both': 2 * floor_ms / res['new_both']['median_ms']},
        'speedup_over_composition': {'grad_H': res['composition_grad_H']['median_ms'] / res['new_grad_H']['median_ms'],
                                     'grad_W': res['composition_grad_W']['median_ms'] / res['new_grad_W']['median_ms']},
        'max_abs_difference': {'grad_H': float((keep['new_h'] - keep['old_h']).abs().max()),
                               'grad_W': float((keep['new_w'] - keep['old_w']).abs().max())},
        'max_abs_value': {'grad_H': float(keep['new_h'].abs().max()), 'grad_W': float(keep['new_w'].abs().max())},
        'both_equals_single': bool(torch.equal(keep['new_both'][0], keep['new_h']) and torch.equal(keep['new_both'][1], keep['new_w'])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='nmfd,nmf2d')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'tool': 'tools/bench_conv_autograd.py', 'device': torch.cuda.get_device_name(0), 'peak_f32_mfma_flops': PEAK_F32_MFMA,
           'shapes': {}}
    for name in a.shapes.split(','):
        out['shapes'][name] = run_shape(name, a.warmup, a.iters, dev)
        print(f'# {name} done', file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
