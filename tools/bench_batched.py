#!/usr/bin/env python3
"""Time many small fits (or many restarts of one fit) as ONE ``BatchedNMF.fit`` beside the loops of ``NMF.fit`` calls a user
has without it:

    python tools/bench_batched.py [--out profiles/batched.json]

  shapes   512 targets of 513 x 128 at rank 16; 4096 targets of 64 x 64 at rank 8; 32 restarts of ONE 5168 x 1025 target at
           rank 88 (the reference's published shape) -- the shared-target form
  arms     batched        BatchedNMF.fit on the whole batch
           loop_auto      one NMF.fit per problem at its default precision ('auto')
           loop_bf16x3    one NMF.fit(precision='bf16x3') per problem
           loop_weighted  one NMF.fit(weights=ones) per problem: the sequential form of the same exact-fp32 arithmetic

Every fit runs a fixed 100 iterations (tol = 0 would stop nothing that still improves; tol = -1e9 is used so that no rounding
can) for beta in {1, 2}; targets uniform in [0.1, 1.1), starts drawn like the constructors draw them.  Within one run the arms
alternate (batched, loop_auto, loop_bf16x3, loop_weighted, three times over) after one warm-up pass of each; a pass is timed
with device events from its first enqueue to its last kernel.  The batched arm fits the whole batch; a loop arm fits
LOOP_FITS problems of it (a loop's time per fit does not depend on how many fits it holds), module construction included --
the loop a user writes.  Reported per (shape, beta, arm): ms per fit (median, min - max of the three repeats), the
12 N C R flop of an iteration over that time, and -- from one profiled 20-iteration fit per arm, when torch.profiler can see
the device -- kernel launches per iteration and the flop rate over summed kernel time (null when it cannot).

Every shape runs in a child process of its own under its own time limit; the shapes run one after the other, the first that
fails ends the run (no retries), and what finished is still written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))

# name -> (batch, N, C, R, shared target)
SHAPES = {'clips_513x128_r16': (512, 513, 128, 16, False), 'tiny_64x64_r8': (4096, 64, 64, 8, False),
          'restarts_5168x1025_r88': (32, 5168, 1025, 88, True)}
BETAS = (1.0, 2.0)
ARMS = ('batched', 'loop_auto', 'loop_bf16x3', 'loop_weighted')
ITERATIONS, REPEATS, LOOP_FITS, PROFILED_ITERATIONS = 100, 3, 16, 20
NEVER = -1e9
ITEM_LIMIT_S = 420


def run_shape(name):
    import torch
    from torchnmf_amd import _capi
    from torchnmf_amd.batched import BatchedNMF
    from torchnmf_amd.nmf import NMF
    B, N, C, R, shared = SHAPES[name]
    dev = torch.device('cuda:0')
    _capi.load()
    g = torch.Generator(device=dev).manual_seed(3)
    V = torch.rand((N, C) if shared else (B, N, C), generator=g, device=dev) + 0.1
    torch.manual_seed(1)
    W0, H0 = torch.randn(B, C, R).abs(), torch.randn(B, N, R).abs()
    ones = torch.ones(N, C, device=dev)
    n_loop = min(B, LOOP_FITS)

    def target(b):
        return V if shared else V[b]

    def fits(arm, beta, max_iter):
        """enqueue the arm's pass; returns the number of fits it holds"""
        if arm == 'batched':
            m = BatchedNMF(W=W0, H=H0).to(dev)
            n = m.fit(V, beta=beta, tol=NEVER, max_iter=max_iter)
            assert n.tolist() == [max_iter] * B
            return B
        kw = {'loop_auto': {}, 'loop_bf16x3': dict(precision='bf16x3'), 'loop_weighted': dict(weights=ones)}[arm]
        for b in range(n_loop):
            m = NMF(W=W0[b], H=H0[b]).to(dev)
            assert m.fit(target(b), beta=beta, tol=NEVER, max_iter=max_iter, **kw) == max_iter
        return n_loop

    def timed(arm, beta):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        n = fits(arm, beta, ITERATIONS)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    def profiled(arm, beta):
        """(kernel launches per iteration and fit, summed kernel ms per fit) of one short pass, or (None, None)"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                n = fits(arm, beta, PROFILED_ITERATIONS)
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if getattr(e, 'device_type', None) is not None and 'CUDA' in str(e.device_type)
                  and not e.name.startswith('Memcpy') and not e.name.startswith('Memset')]
            if not ev:
                return None, None
            per_problem = n if arm != 'batched' else 1          # a batched launch serves every problem
            return len(ev) / PROFILED_ITERATIONS / per_problem, sum(e.device_time for e in ev) * 1e-3 / n
        except Exception as exc:      # the profiler is an extra: its absence must not cost the timings
            print(f'profiler unavailable for {arm}: {exc!r}', file=sys.stderr)
            return None, None

    flop_it = 12.0 * N * C * R
    rows = []
    for beta in BETAS:
        times = {arm: [] for arm in ARMS}
        for arm in ARMS:                 # warm-up: every kernel of every arm loaded, every allocation cached
            fits(arm, beta, 10)
        torch.cuda.synchronize()
        for _ in range(REPEATS):         # alternating arms
            for arm in ARMS:
                times[arm].append(timed(arm, beta))
        for arm in ARMS:
            t = times[arm]
            launches, kernel_ms = profiled(arm, beta)
            row = dict(shape=name, batch=B, n=N, c=C, rank=R, shared_target=shared, beta=beta, arm=arm,
                       fits_timed=B if arm == 'batched' else n_loop, iterations=ITERATIONS,
                       ms_per_fit=statistics.median(t), ms_per_fit_min=min(t), ms_per_fit_max=max(t),
                       tflops_over_elapsed=flop_it * ITERATIONS / (statistics.median(t) * 1e-3) / 1e12,
                       launches_per_iteration=launches,
                       tflops_over_kernel_time=(flop_it * PROFILED_ITERATIONS / (kernel_ms * 1e-3) / 1e12
                                                if kernel_ms else None))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return dict(shape=name, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batched.json'))
    ap.add_argument('--shape', choices=list(SHAPES), help='run ONE shape in this process and print its rows (the driver calls '
                    'this)')
    a = ap.parse_args()
    if a.shape:
        print('ITEM_RESULT ' + json.dumps(run_shape(a.shape)), flush=True)
        return 0
    res = dict(tool='tools/bench_batched.py', shapes={k: list(v) for k, v in SHAPES.items()}, betas=list(BETAS),
               iterations=ITERATIONS, repeats=REPEATS, loop_fits=LOOP_FITS, flop_per_iteration='12 N C R', rows=[], failed=None)
    rc = 0
    for name in SHAPES:              # chained: the first failure ends the run, nothing is tried again
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', name], capture_output=True, text=True,
                               timeout=ITEM_LIMIT_S)
        except subprocess.TimeoutExpired:
            res['failed'], rc = dict(shape=name, why=f'time limit of {ITEM_LIMIT_S} s'), 124
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('ITEM_RESULT ')]
        if p.returncode != 0 or not line:
            res['failed'], rc = dict(shape=name, why=f'exit status {p.returncode}', stderr=p.stderr[-2000:]), p.returncode or 1
            break
        rows = json.loads(line[-1][len('ITEM_RESULT '):])['rows']
        res['rows'] += rows
        for r in rows:
            print(json.dumps(r), flush=True)
    if rc == 0:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
        # the speed-up of the batched form over every loop, per (shape, beta): > 1 means the batch wins
        res['speedup'] = []
        for name in SHAPES:
            for beta in BETAS:
                pick = {r['arm']: r['ms_per_fit'] for r in res['rows'] if r['shape'] == name and r['beta'] == beta}
                res['speedup'].append(dict(shape=name, beta=beta, **{f'over_{k}': pick[k] / pick['batched'] for k in ARMS[1:]}))
        print(json.dumps(res['speedup']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return rc


if __name__ == '__main__':
    sys.exit(main())
