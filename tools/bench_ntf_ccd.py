#!/usr/bin/env python3
"""Time the CCD sweep of ``NTF.fit(solver='ccd')`` (``nmfmu_sp_ntf_ccd_sweep``) per mode beside the 'missing' multiplicative
half-step of the same mode from the same factors, in the same run:

    python tools/bench_ntf_ccd.py [--out profiles/ntf_ccd.json]

  (a) recommender-shaped: 65 536 x 16 384 x 24 with 10 M stored entries (drawn uniformly; duplicates coalesce), rank 64 -- the
      target of tools/bench_sparse_ntf.py.  Per mode: the sweep with ``vec`` 1 (4-byte gathers), 2 (16-byte gathers, four
      coordinates per gather pair) and 0 (the library's rule), and ``nmfmu_sp_ntf_step`` at beta = 2, 'missing'; the mode's share
      of a CCD iteration; ``vec1_equals_vec2`` (the updated factor, bit for bit, from the warm-up calls).  Then the fit: the
      loss after 200 MU iterations from the scaled start, and the CCD iterations and seconds to reach it (at most 200), both
      timed by a host clock around iterations that end in a device synchronise, the loss evaluations outside the clock.
  (b) 512^3 at 1 % density, rank 64: the same three modes, no fit.

Device events around 5 back-to-back calls, reported per call; every route is called twice to warm up, then the routes are
timed in turn, round by round, 10 rounds: median with min - max.  The owner is restored before every window.

Every workload runs in a child process of its own under its own time limit; the first that fails ends the run (no retries).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))

WARMUP, REPEATS, CALLS, RANK, MU_ITERS, CCD_MAX = 2, 10, 5, 64, 200, 200
ITEM_LIMIT_S = 420
WORKLOADS = {'recommender': dict(shape=(65536, 16384, 24), nnz=10_000_000, fit=True),
             'cube_1pct': dict(shape=(512, 512, 512), nnz=512 ** 3 // 100, fit=False)}


def one(call, before):
    import torch
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


def timed(routes, before, keep):
    """{name: median / min / max ms per call}: two warm-up calls each (``keep(name)`` after the second: one call from the
    restored owner), then the routes in turn, round by round."""
    for k, call in routes.items():
        for _ in range(WARMUP):
            before()
            call()
        keep(k)
    ts = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, call in routes.items():
            ts[k].append(one(call, before))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def run(shape, nnz, fit, emit):
    import torch
    from torchnmf_amd import ntf
    from torchnmf_amd.engine import mu_gamma
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(3)
    idx = torch.stack([torch.randint(0, d, (nnz,), generator=g, device=dev) for d in shape])
    T = ntf.SparseNtfTarget(torch.sparse_coo_tensor(idx, torch.rand(nnz, generator=g, device=dev) + 0.1, shape).coalesce())
    start = [torch.rand(d, RANK, generator=g, device=dev) + 0.25 for d in shape]
    eng = ntf._CcdNtf(T, [f.clone() for f in start], (True,) * 3, 0.0, 0.0)
    eng.divergence()                                 # the once-only scale: both solvers start from the scaled factors
    start = [f.clone() for f in eng.fs]
    step = (0.0, 0.0, mu_gamma(2.0))
    rows = []
    for mode in range(3):
        fs = [f.clone() for f in start]
        counts = torch.diff(T.modes[mode]['rowptr'])

        def restore():
            fs[mode].copy_(start[mode])
        routes = {f'ccd_vec{v}': (lambda v=v: ntf._ccd_call(T, fs, mode, 0.0, 0.0, eng.orders[mode], eng.scratch, vec=v))
                  for v in (1, 2, 0)}
        routes['mu_missing'] = lambda: ntf._sparse_call(T, fs, mode, 2.0, 'missing', step=step)
        result = {}
        t = timed(routes, restore, lambda k: result.__setitem__(k, fs[mode].clone()))
        rows.append(dict(shape=list(shape), nnz=T.nnz, rank=RANK, mode=mode, rows=shape[mode], longest_row=int(counts.max()),
                         workgroup_rows=int((counts > 512).sum()), scratch_rows=int((counts > 512 * 16).sum()),
                         vec1_equals_vec2=bool(torch.equal(result['ccd_vec1'], result['ccd_vec2'])),
                         ccd_over_mu=t['ccd_vec0']['median_ms'] / t['mu_missing']['median_ms'],
                         vec2_over_vec1=t['ccd_vec2']['median_ms'] / t['ccd_vec1']['median_ms'], **t))
    total = sum(r['ccd_vec0']['median_ms'] for r in rows)
    for r in rows:
        r['share_of_ccd_iteration'] = r['ccd_vec0']['median_ms'] / total
        emit(r)
    if not fit:
        return

    def iterate(half_step, loss, fs, n_max, until=None):
        """(losses after every iteration, seconds of the iterations alone)"""
        losses, spent = [], 0.0
        for _ in range(n_max):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for mode in range(3):
                half_step(fs, mode)
            torch.cuda.synchronize()
            spent += time.perf_counter() - t0
            losses.append(loss(fs))
            if until is not None and losses[-1] <= until:
                break
        return losses, spent

    def loss(fs):
        return float(ntf._sparse_loss(T, fs, 2.0, 'missing').item())
    mu_losses, mu_s = iterate(lambda fs, mode: ntf._sparse_call(T, fs, mode, 2.0, 'missing', step=step), loss,
                              [f.clone() for f in start], MU_ITERS)
    ccd_losses, ccd_s = iterate(lambda fs, mode: ntf._ccd_call(T, fs, mode, 0.0, 0.0, eng.orders[mode], eng.scratch), loss,
                                [f.clone() for f in start], CCD_MAX, until=mu_losses[-1])
    reached = ccd_losses[-1] <= mu_losses[-1]
    emit(dict(shape=list(shape), nnz=T.nnz, rank=RANK, fit=True, loss_start=loss(start), mu_iterations=MU_ITERS,
              mu_loss=mu_losses[-1], mu_seconds=mu_s, ccd_reached_mu_loss=reached, ccd_iterations=len(ccd_losses),
              ccd_loss=ccd_losses[-1], ccd_seconds=ccd_s, mu_seconds_over_ccd_seconds=mu_s / ccd_s if reached else None,
              ccd_losses=ccd_losses[:20], mu_losses_every_20=mu_losses[19::20]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ntf_ccd.json'))
    ap.add_argument('--item', choices=list(WORKLOADS), help='run ONE workload in this process (the driver calls this)')
    a = ap.parse_args()
    if a.item:
        import torch
        rows = []
        run(**WORKLOADS[a.item], emit=rows.append)
        print('ITEM_RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rows=rows)), flush=True)
        return 0
    res = dict(tool='tools/bench_ntf_ccd.py', warmup=WARMUP, repeats=REPEATS, calls_per_window=CALLS, rows=[], failed=None)
    rc = 0
    for item in WORKLOADS:          # chained: the first failure ends the run, nothing is tried again
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
