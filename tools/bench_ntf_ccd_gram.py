#!/usr/bin/env python3
"""Time the normal-equations route of ``ntf.ntf_ccd_sweep(gram_rows=)`` (``nmfmu_sp_ntf_ccd_gram``) beside the maintained-residual
sweep and the 'missing' multiplicative half-step of the same mode, from the same scaled factors, in the same run:

    python tools/bench_ntf_ccd_gram.py [--out profiles/ntf_ccd_gram.json]

  recommender  65 536 x 16 384 x 24 with 10 M stored entries, rank 64 (the target of tools/bench_ntf_ccd.py).  Per mode: the
               sweep, the new route for every row (``gram_rows=0``) and ``nmfmu_sp_ntf_step`` at beta = 2, 'missing'; the
               parts, the part length and the bytes and flops the parts kernel needs by its shapes.  Then the fit: the loss
               after 200 MU iterations, and the iterations and seconds CCD needs to get below it with ``gram_rows=None`` and
               with ``gram_rows`` set so that only the 24-row mode takes the new route (host clock around iterations that end in
               a device synchronise, losses outside it).
  cube_1pct    512^3 at 1 %, rank 64: the three modes, no fit.
  crossover    modes of equal rows (``rows x 4096 x 4096``, 2 M entries in all) of 512 .. 65 536 entries at ranks 32, 64, 128,
               256: the sweep against the new route.

Device events around 5 back-to-back calls, reported per call; every route is called twice to warm up, then the routes are
timed in turn, round by round, 10 rounds: median with min - max.  The owner is restored before every window.  Every workload
runs in a child process of its own under its own time limit; the first that fails ends the run (no retries).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

RANK, MU_ITERS, CCD_MAX, ONLY_SHORT_MODE = 64, 200, 60, 100_000
ITEM_LIMIT_S = 400
WORKLOADS = ['recommender', 'cube_1pct', 'crossover']


def _mode_rows(ntf, T, start, rank, mode, with_mu):
    """One mode: the sweep, the new route for every row with entries, the MU half-step -> a result row."""
    import torch
    from bench_ntf_ccd import timed
    from torchnmf_amd.engine import mu_gamma
    fs = [f.clone() for f in start]
    counts = torch.diff(T.modes[mode]['rowptr'])
    plan = ntf._gram_plan(T, mode, 0, 0, rank)
    ws = torch.empty(plan['ws'], dtype=torch.float32, device=T.device)
    scratch = torch.empty(max(T.nnz, 4), dtype=torch.float32, device=T.device)
    order = ntf._ccd_order(T.modes[mode])
    routes = {'sweep': lambda: ntf._ccd_call(T, fs, mode, 0.0, 0.0, order, scratch),
              'gram': lambda: ntf._gram_call(T, fs, mode, 0.0, 0.0, plan, ws)}
    if with_mu:
        routes['mu_missing'] = lambda: ntf._sparse_call(T, fs, mode, 2.0, 'missing', step=(0.0, 0.0, mu_gamma(2.0)))
    result = {}
    t = timed(routes, lambda: fs[mode].copy_(start[mode]), lambda k: result.__setitem__(k, fs[mode].clone()))
    r_pad = 32 if rank <= 32 else 64 if rank <= 64 else 128 if rank <= 128 else 256
    nb, n_parts = r_pad // 32, sum(b[4] for b in plan['batches'])
    return dict(shape=list(T.shape), nnz=T.nnz, rank=rank, mode=mode, rows=T.shape[mode], longest_row=int(counts.max()),
                part=plan['part'], parts=n_parts, batches=len(plan['batches']), workspace_floats=plan['ws'],
                gram_vs_sweep_max_rel=float(((result['gram'] - result['sweep']).abs() / result['sweep']).max()),
                sweep_over_gram=t['sweep']['median_ms'] / t['gram']['median_ms'],
                # by the shapes: two panel rows, two indices and a value per entry; the upper blocks of 32-entry tiles
                gather_bytes=T.nnz * (2 * 4 * rank + 12), parts_write_bytes=n_parts * 4 * (nb * (nb + 1) // 2 * 1024 + r_pad),
                mfma_flops=2 * 32 * 32 * (nb * (nb + 1) // 2) * 32 * int(((counts + 31) // 32).sum()), **t)


def _target(ntf, shape, nnz, rank, idx=None):
    import torch
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(3)
    if idx is None:
        idx = torch.stack([torch.randint(0, d, (nnz,), generator=g, device=dev) for d in shape])
    T = ntf.SparseNtfTarget(torch.sparse_coo_tensor(idx, torch.rand(idx.shape[1], generator=g, device=dev) + 0.1, shape).coalesce())
    eng = ntf._CcdNtf(T, [torch.rand(d, rank, generator=g, device=dev) + 0.25 for d in shape], (True,) * 3, 0.0, 0.0)
    eng.divergence()                                 # the once-only scale: every route starts from the scaled factors
    return T, [f.clone() for f in eng.fs]


def run(item, emit):
    import torch
    from torchnmf_amd import ntf
    from torchnmf_amd.engine import mu_gamma
    if item == 'crossover':
        for rank in (32, 64, 128, 256):
            for length in (512, 2048, 8192, 32768, 65536):
                rows = (1 << 21) // length
                own = torch.arange(rows, device='cuda').repeat_interleave(length)
                flat = torch.cat([torch.randperm(1 << 24, device='cuda')[:length] for _ in range(min(rows, 8))])
                flat = flat.repeat(-(-rows // 8))[:rows * length]      # distinct (a, b) within a row
                T, start = _target(ntf, (rows, 4096, 4096), 0, rank, torch.stack([own, flat // 4096, flat % 4096]))
                emit(dict(crossover=True, row_length=length, **_mode_rows(ntf, T, start, rank, 0, False)))
        return
    shape, nnz = ((65536, 16384, 24), 10_000_000) if item == 'recommender' else ((512, 512, 512), 512 ** 3 // 100)
    T, start = _target(ntf, shape, nnz, RANK)
    for mode in range(3):
        emit(_mode_rows(ntf, T, start, RANK, mode, True))
    if item != 'recommender':
        return

    def iterate(half_step, fs, n_max, until=None):
        """(losses after every iteration, seconds of the iterations alone)"""
        losses, spent = [], 0.0
        for _ in range(n_max):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for mode in range(3):
                half_step(mode)
            torch.cuda.synchronize()
            spent += time.perf_counter() - t0
            losses.append(float(ntf._sparse_loss(T, fs, 2.0, 'missing').item()))
            if until is not None and losses[-1] <= until:
                break
        return losses, spent
    fs = [f.clone() for f in start]
    step = (0.0, 0.0, mu_gamma(2.0))
    mu_losses, mu_s = iterate(lambda mode: ntf._sparse_call(T, fs, mode, 2.0, 'missing', step=step), fs, MU_ITERS)
    out = dict(shape=list(shape), nnz=T.nnz, rank=RANK, fit=True, mu_iterations=MU_ITERS, mu_loss=mu_losses[-1], mu_seconds=mu_s)
    for name, gram_rows in (('ccd_sweep', None), ('ccd_gram', ONLY_SHORT_MODE), ('ccd_sweep_again', None),
                            ('ccd_gram_again', ONLY_SHORT_MODE)):
        eng = ntf._CcdNtf(T, [f.clone() for f in start], (True,) * 3, 0.0, 0.0, gram_rows)
        eng._scaled = True                           # (start is already scaled)
        eng.half_step(2), torch.cuda.synchronize()   # warm: code objects, the plan
        for f, s in zip(eng.fs, start):
            f.copy_(s)
        losses, secs = iterate(eng.half_step, eng.fs, CCD_MAX, until=mu_losses[-1])
        out[name] = dict(gram_rows=gram_rows, iterations=len(losses), loss=losses[-1], seconds=secs,
                         reached_mu_loss=losses[-1] <= mu_losses[-1], mu_seconds_over_seconds=mu_s / secs,
                         long_rows_per_mode=[sum(b[3] for b in p['batches']) if p else 0 for p in eng.plans])
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ntf_ccd_gram.json'))
    ap.add_argument('--item', choices=WORKLOADS, help='run ONE workload in this process (the driver calls this)')
    ap.add_argument('--only', choices=WORKLOADS, action='append', help='the workloads to run (default: all)')
    a = ap.parse_args()
    if a.item:
        import torch
        rows = []
        run(a.item, rows.append)
        print('ITEM_RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rows=rows)), flush=True)
        return 0
    res = dict(tool='tools/bench_ntf_ccd_gram.py', warmup=2, repeats=10, calls_per_window=5, rows=[], failed=None)
    rc = 0
    for item in a.only or WORKLOADS:          # chained: the first failure ends the run, nothing is tried again
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
        got = json.loads(line[-1][len('ITEM_RESULT '):])
        res['device'] = got['device']
        res['rows'] += got['rows']
        for r in got['rows']:
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out, 'failed:', res['failed'])
    return rc


if __name__ == '__main__':
    sys.exit(main())
