#!/usr/bin/env python3
"""Time one NTF half-step per mode (``nmfmu_ntf_step``) beside the two routes a user has without it, in the same run:

    python tools/bench_ntf.py [--out profiles/ntf.json]

  ntf           one nmfmu_ntf_step on the row-major tensor in place (the fused kernel + the finishing kernel)
  materialised  nmfmu_wmu_step on the mode's unfolding: the Khatri-Rao panel is materialised ([contraction, R] floats), mode 1
                takes a permuted copy of V (and of M), and an unweighted problem needs a ones tensor for M; ``build_ms`` is the
                time to make those, ``kernel_ms`` the wmu step alone, ``total_ms`` both
  torch         an fp32 loop of torch ops for the same half-step (einsum reconstruction, seeds, einsum contraction, update)

Workloads: 8 x 1025 x 8192 at rank 32 and 512 x 512 x 512 at rank 64, beta in {1, 0.5}, unweighted and weighted (weights in
[0.25, 4) with 30 % zeros).  Device events; per (workload, beta, weights, mode) every route is called twice to warm up (its peak
memory is read there), then the routes are timed in turn, round by round, 10 rounds: median with min - max.  The owner is restored
before every call.  ``fraction_of_hbm`` counts V (and M) once against 8 TB/s, ``fraction_of_fp32_mfma_peak`` 6 I J K R flop (y, num,
den) against 157.3 TFLOP/s, both over the whole ntf step; ``peak_bytes`` is torch's high-water mark of the route above what
V, M and the factors hold.

``--short`` times the 32-row tile instead (``nmfmu_ntf_short_step``, csrc/nmfmu_ntf_short.hip) on the short owner modes it is
for, beside the forced 128-row tile and the torch loop, and sweeps the contraction length at 8 rows for the automatic rule of
``nmfmu_ntf_tile``; same method, same rounds.  Its output goes to profiles/ntf_short.json:

    python tools/bench_ntf.py --short

  short   one nmfmu_ntf_short_step (the 32-row tile + the finishing kernel)
  wide    one nmfmu_ntf_step (the 128-row tile) on the same mode
  torch   the fp32 torch loop above (the workloads only, not the sweep)

Every workload runs in a child process of its own under its own time limit; the first that fails ends the run (no retries).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))

WORKLOADS = {'8x1025x8192_r32': ((8, 1025, 8192), 32), '512x512x512_r64': ((512, 512, 512), 64)}
# --short: (shape, rank) of tensors whose mode 0 is short; the sweep is 8 x (c / 128) x 128 at every padded rank
SHORT_WORKLOADS = {'8x1025x8192_r32': ((8, 1025, 8192), 32), '8x1025x8192_r128': ((8, 1025, 8192), 128),
                   '2x1025x8192_r32': ((2, 1025, 8192), 32), '24x4096x4096_r64': ((24, 4096, 4096), 64)}
SWEEP = 'sweep_8_rows'
SWEEP_RANKS, SWEEP_LOG2 = (32, 64, 128, 256), range(10, 21)
BETAS = (1.0, 0.5)
WARMUP, REPEATS = 2, 10
HBM_PEAK, FP32_MFMA_PEAK = 8e12, 157.3e12
ITEM_LIMIT_S = 400


def one(call, before=None):
    import torch
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def run_item(name):
    import torch
    from torchnmf_amd import _capi
    from torchnmf_amd.constants import eps
    from torchnmf_amd.engine import mu_gamma
    shape, R = WORKLOADS[name]
    I, J, K = shape
    dev, lib = torch.device('cuda:0'), _capi.load()
    g = torch.Generator(device=dev).manual_seed(3)
    start = [torch.rand(d, R, generator=g, device=dev) + 0.25 for d in shape]
    V = torch.rand(shape, generator=g, device=dev) + 0.1
    Mw = (torch.rand(shape, generator=g, device=dev) * 3.75 + 0.25) * (torch.rand(shape, generator=g, device=dev) > 0.3)
    r_pad, stream = lib.nmfmu_pad_rank(R), torch.cuda.current_stream().cuda_stream
    rows_out = []
    for weighted in (False, True):
        M = Mw if weighted else None
        for beta in BETAS:
            step = (0.0, 0.0, mu_gamma(beta))
            for mode in range(3):
                fs = [f.clone() for f in start]
                rows, contraction = shape[mode], I * J * K // shape[mode]
                pa, pb = (f for n, f in enumerate(fs) if n != mode)
                sub = ('ijk,jr,kr->ir', 'ijk,ir,kr->jr', 'ijk,ir,jr->kr')[mode]
                n, c, side = ((contraction, rows, 1) if mode == 2 else (rows, contraction, 0))
                ws = torch.empty(max(lib.nmfmu_ntf_ws(rows, contraction, r_pad, 0), lib.nmfmu_wmu_ws(rows, contraction, r_pad, 0)),
                                 dtype=torch.float32, device=dev)
                held = {}

                def restore():
                    fs[mode].copy_(start[mode])

                def ntf_step():
                    _capi.check(lib.nmfmu_ntf_step(V.data_ptr(), None if M is None else M.data_ptr(), I, J, K, mode,
                                                   fs[mode].data_ptr(), pa.data_ptr(), pb.data_ptr(), R, r_pad, beta, *step, 0,
                                                   ws.data_ptr(), stream), 'nmfmu_ntf_step')

                def build():        # the Khatri-Rao panel, mode 1's permuted copies, an unweighted problem's ones
                    held.clear()
                    held['P'] = (pa[:, None, :] * pb[None, :, :]).reshape(contraction, R)
                    M2 = Mw if weighted else torch.ones(shape, device=dev)
                    if mode == 1:
                        held['V'], held['M'] = V.permute(1, 0, 2).contiguous(), M2.permute(1, 0, 2).contiguous()
                    else:
                        held['V'], held['M'] = V, M2

                def wmu_step():
                    _capi.check(lib.nmfmu_wmu_step(held['V'].data_ptr(), held['M'].data_ptr(), c, n, c, side, fs[mode].data_ptr(),
                                                   held['P'].data_ptr(), R, r_pad, beta, *step, 0, ws.data_ptr(), stream),
                                'nmfmu_wmu_step')

                def torch_step():
                    y = torch.einsum('ir,jr,kr->ijk', *fs)
                    if beta == 1.0:
                        gn, gp = V / (y + eps), torch.ones_like(y)
                    else:
                        p2 = (y + eps).pow(beta - 2)
                        gn, gp = p2 * V, p2 * (y + eps)
                    if weighted:
                        gn, gp = torch.where(Mw > 0, Mw * gn, 0.0), torch.where(Mw > 0, Mw * gp, 0.0)
                    num, den = torch.einsum(sub, gn, pa, pb), torch.einsum(sub, gp, pa, pb)
                    fs[mode].mul_(((num.clamp_min(0) + eps) / (den.clamp_min(0) + eps)).pow(step[2]))
                routes = dict(ntf=(ntf_step, restore), build=(build, None), wmu=(wmu_step, restore), torch=(torch_step, restore))
                peak, result = {}, {}
                base = torch.cuda.memory_allocated()
                for name_, (call, before) in routes.items():      # warm-up; build stays held for wmu (its peak counts both)
                    if name_ == 'torch':
                        held.clear()
                    if name_ != 'wmu':
                        torch.cuda.reset_peak_memory_stats()
                    for _ in range(WARMUP):
                        one(call, before)
                    peak[name_], result[name_] = torch.cuda.max_memory_allocated() - base, fs[mode].clone()
                ts = {k: [] for k in routes}
                for _ in range(REPEATS):                           # the routes in turn, round by round
                    for name_, (call, before) in routes.items():
                        ts[name_].append(one(call, before))
                held.clear()
                t = {k: stats(v) for k, v in ts.items()}

                def diff(k):
                    return float(((result[k] - result['ntf']).abs() / result['ntf']).max())
                ms = t['ntf']['median_ms'] * 1e-3
                row = dict(workload=name, rank=R, beta=beta, weighted=weighted, mode=mode, rows=rows, contraction=contraction,
                           ntf=dict(t['ntf'], parts=lib.nmfmu_ntf_nsplit(rows, contraction, r_pad),
                                    peak_bytes=peak['ntf'] + 4 * lib.nmfmu_ntf_ws(rows, contraction, r_pad, 0),
                                    fraction_of_hbm=4.0 * I * J * K * (2 if weighted else 1) / ms / HBM_PEAK,
                                    fraction_of_fp32_mfma_peak=6.0 * I * J * K * R / ms / FP32_MFMA_PEAK),
                           materialised=dict(build_ms=t['build']['median_ms'], kernel_ms=t['wmu']['median_ms'],
                                             kernel_min_ms=t['wmu']['min_ms'], kernel_max_ms=t['wmu']['max_ms'],
                                             total_ms=t['build']['median_ms'] + t['wmu']['median_ms'],
                                             parts=lib.nmfmu_wmu_nsplit(rows, contraction, r_pad),
                                             peak_bytes=peak['wmu'] + 4 * lib.nmfmu_wmu_ws(rows, contraction, r_pad, 0),
                                             max_rel_diff_to_ntf=diff('wmu')),
                           torch=dict(t['torch'], peak_bytes=peak['torch'], max_rel_diff_to_ntf=diff('torch')))
                rows_out.append(row)
                print(json.dumps(row), flush=True)
                del ws
    return dict(item=name, device=torch.cuda.get_device_name(0), rows=rows_out)


def run_short_item(name):
    """Mode 0 of one --short workload (or the sweep): the routes in turn, round by round, as run_item does."""
    import torch
    from torchnmf_amd import _capi
    from torchnmf_amd.constants import eps
    from torchnmf_amd.engine import mu_gamma
    dev, lib = torch.device('cuda:0'), _capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(3)
    sweep = name == SWEEP
    cases = ([((8, (1 << k) // 128, 128), R) for R in SWEEP_RANKS for k in SWEEP_LOG2] if sweep else [SHORT_WORKLOADS[name]])
    rows_out = []
    for shape, R in cases:
        I, J, K = shape
        start = [torch.rand(d, R, generator=g, device=dev) + 0.25 for d in shape]
        V = torch.rand(shape, generator=g, device=dev) + 0.1
        Mw = (torch.rand(shape, generator=g, device=dev) * 3.75 + 0.25) * (torch.rand(shape, generator=g, device=dev) > 0.3)
        r_pad, contraction = lib.nmfmu_pad_rank(R), J * K
        ws = torch.empty(max(lib.nmfmu_ntf_ws(I, contraction, r_pad, 0), lib.nmfmu_ntf_short_ws(I, contraction, r_pad, 0)),
                         dtype=torch.float32, device=dev)
        for weighted, beta in (((False, 1.0), (True, 0.5)) if sweep else [(w, b) for w in (False, True) for b in BETAS]):
            M = Mw if weighted else None
            step = (0.0, 0.0, mu_gamma(beta))
            fs = [f.clone() for f in start]

            def restore():
                fs[0].copy_(start[0])

            def entry(fn, what):
                def call():
                    _capi.check(fn(V.data_ptr(), None if M is None else M.data_ptr(), I, J, K, 0, fs[0].data_ptr(), fs[1].data_ptr(),
                                   fs[2].data_ptr(), R, r_pad, beta, *step, 0, ws.data_ptr(), stream), what)
                return call

            def torch_step():
                y = torch.einsum('ir,jr,kr->ijk', *fs)
                if beta == 1.0:
                    gn, gp = V / (y + eps), torch.ones_like(y)
                else:
                    p2 = (y + eps).pow(beta - 2)
                    gn, gp = p2 * V, p2 * (y + eps)
                if weighted:
                    gn, gp = torch.where(Mw > 0, Mw * gn, 0.0), torch.where(Mw > 0, Mw * gp, 0.0)
                num, den = torch.einsum('ijk,jr,kr->ir', gn, fs[1], fs[2]), torch.einsum('ijk,jr,kr->ir', gp, fs[1], fs[2])
                fs[0].mul_(((num.clamp_min(0) + eps) / (den.clamp_min(0) + eps)).pow(step[2]))
            routes = dict(short=entry(lib.nmfmu_ntf_short_step, 'nmfmu_ntf_short_step'), wide=entry(lib.nmfmu_ntf_step, 'nmfmu_ntf_step'))
            if not sweep:
                routes['torch'] = torch_step
            result = {}
            for k, call in routes.items():
                for _ in range(WARMUP):
                    one(call, restore)
                result[k] = fs[0].clone()
            ts = {k: [] for k in routes}
            for _ in range(REPEATS):                               # the routes in turn, round by round
                for k, call in routes.items():
                    ts[k].append(one(call, restore))
            ms = statistics.median(ts['short']) * 1e-3
            row = dict(workload=name, shape=list(shape), rank=R, r_pad=r_pad, beta=beta, weighted=weighted, mode=0, rows=I,
                       contraction=contraction, auto_tile=lib.nmfmu_ntf_tile(I, contraction, r_pad),
                       short=dict(stats(ts['short']), parts=lib.nmfmu_ntf_short_nsplit(I, contraction, r_pad),
                                  fraction_of_hbm=4.0 * I * J * K * (2 if weighted else 1) / ms / HBM_PEAK,
                                  fraction_of_fp32_mfma_peak=6.0 * I * J * K * R / ms / FP32_MFMA_PEAK),
                       wide=dict(stats(ts['wide']), parts=lib.nmfmu_ntf_nsplit(I, contraction, r_pad)),
                       max_rel_diff_short_to_wide=float(((result['short'] - result['wide']).abs() / result['wide']).max()))
            if not sweep:
                row['torch'] = dict(stats(ts['torch']),
                                    max_rel_diff_to_short=float(((result['torch'] - result['short']).abs() / result['short']).max()))
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del ws, V, Mw
    return dict(item=name, device=torch.cuda.get_device_name(0), rows=rows_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--short', action='store_true', help='the 32-row tile on short modes and the sweep for nmfmu_ntf_tile')
    ap.add_argument('--out', help='default: profiles/ntf.json, with --short profiles/ntf_short.json')
    ap.add_argument('--item', help='run ONE workload in this process (the driver calls this)')
    a = ap.parse_args()
    items = list(SHORT_WORKLOADS) + [SWEEP] if a.short else list(WORKLOADS)
    a.out = a.out or os.path.join(ROOT, 'profiles', 'ntf_short.json' if a.short else 'ntf.json')
    if a.item:
        assert a.item in items, items
        print('ITEM_RESULT ' + json.dumps((run_short_item if a.short else run_item)(a.item)), flush=True)
        return 0
    res = dict(tool='tools/bench_ntf.py', betas=list(BETAS), warmup=WARMUP, repeats=REPEATS, hbm_peak=HBM_PEAK,
               fp32_mfma_peak=FP32_MFMA_PEAK, flop_per_half_step='6 I J K R', rows=[], failed=None)
    rc = 0
    for item in items:              # chained: the first failure ends the run, nothing is tried again
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--item', item] + ['--short'] * a.short,
                               capture_output=True, text=True,
                               timeout=ITEM_LIMIT_S)
        except subprocess.TimeoutExpired:
            res['failed'], rc = dict(item=item, why=f'time limit of {ITEM_LIMIT_S} s'), 124
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('ITEM_RESULT ')]
        if p.returncode != 0 or not line:
            res['failed'], rc = dict(item=item, why=f'exit status {p.returncode}', stderr=p.stderr[-2000:]), p.returncode or 1
            break
        got = json.loads(line[-1][len('ITEM_RESULT '):])
        res['device'] = got['device']
        res['rows'] += got['rows']
        for r in got['rows']:
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return rc


if __name__ == '__main__':
    sys.exit(main())
