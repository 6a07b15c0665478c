#!/usr/bin/env python3
"""Time the sparse NTF half-step per mode (``nmfmu_sp_ntf_step``) beside what a user has without it, in the same run:

    python tools/bench_sparse_ntf.py [--out profiles/sparse_ntf.json]

  (a) recommender-shaped: 65 536 x 16 384 x 24 with 10 M stored entries (drawn uniformly; duplicates coalesce), rank 64,
      beta in {1, 2}, both ``unstored`` values.  Per mode: the half-step with ``stage`` forced to 1 (no panel in LDS), to 2
      (every panel that fits) and left to the library's rule (0); the same step as a torch loop (``index_select`` x 2,
      multiply, ``index_add_``; 'missing' only); and ``nmfmu_sp_masked_step`` on a 65 536 x 16 384 matrix of the same nnz and
      rank -- the price of the second gather.  ``bytes_per_entry`` counts 12 bytes of indices and value plus one rank row of
      4 R bytes per gather that goes to memory (a staged panel's does not); ``fraction_of_hbm`` is that times nnz, plus the
      owner read and written once, over the median time against 8 TB/s.
  (b) 512^3 at 1 % density, rank 64: the sparse half-step against the dense weighted ``nmfmu_ntf_step`` on the densified tensor
      with the stored mask as weights.

Device events around 5 back-to-back calls, reported per call; every route is called twice to warm up, then the kernel
routes are timed in turn, round by round, 10 rounds: median with min - max.  The torch loop has rounds of its own after them,
so its 2.5 GB temporaries do not sit in front of a kernel route.  The owner is restored before every window.  A 'zero'
half-step includes its small per-factor terms.  ``stage0`` is whatever the library's rule chooses; its bytes are not counted
here.  From the warm-up calls: ``stage1_equals_stage2`` (the updated factor and the loss, bit for bit) and the torch loop's
largest relative difference to the kernel.

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

WARMUP, REPEATS, CALLS, HBM_PEAK, RANK = 2, 10, 5, 8e12, 64
ITEM_LIMIT_S = 240
WORKLOADS = {'recommender': dict(shape=(65536, 16384, 24), nnz=10_000_000, dense_too=False, masked_too=True),
             'cube_1pct': dict(shape=(512, 512, 512), nnz=512 ** 3 // 100, dense_too=True, masked_too=False)}
CASES = (('missing', 1.0), ('missing', 2.0), ('zero', 1.0), ('zero', 2.0))


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


def timed(routes, before, keep=None):
    """{name: median / min / max ms per call}: two warm-up calls each (``keep(name)`` after the second: one call from the
    restored owner), then the routes in turn, round by round."""
    for k, call in routes.items():
        for _ in range(WARMUP):
            before()
            call()
        if keep is not None:
            keep(k)
    ts = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, call in routes.items():
            ts[k].append(one(call, before))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def random_sparse(shape, nnz, gen, dev):
    import torch
    idx = torch.stack([torch.randint(0, d, (nnz,), generator=gen, device=dev) for d in shape])
    return torch.sparse_coo_tensor(idx, torch.rand(nnz, generator=gen, device=dev) + 0.1, shape).coalesce()


def run(shape, nnz, dense_too, masked_too, emit):
    import torch
    from torchnmf_amd import _capi, ntf
    from torchnmf_amd import sparse_autograd as SA
    from torchnmf_amd.constants import eps
    from torchnmf_amd.engine import mu_gamma
    dev, lib = torch.device('cuda:0'), _capi.load()
    g = torch.Generator(device=dev).manual_seed(3)
    V = random_sparse(shape, nnz, g, dev)
    T = ntf.SparseNtfTarget(V)
    start = [torch.rand(d, RANK, generator=g, device=dev) + 0.25 for d in shape]
    cap, r_pad = lib.nmfmu_sp_ntf_lds_rows(RANK), lib.nmfmu_pad_rank(RANK)
    if dense_too:
        D = ntf.NtfTarget(V.to_dense(), torch.sparse_coo_tensor(V.indices(), torch.ones_like(V.values()), shape).to_dense())
    if masked_too:
        M2 = SA.SparseTarget(random_sparse(shape[:2], T.nnz, g, dev))
    for unstored, beta in CASES:
        step = (0.0, 0.0, mu_gamma(beta))
        for mode in range(3):
            fs = [f.clone() for f in start]
            m = T.modes[mode]
            pa, pb = (f for n, f in enumerate(fs) if n != mode)
            own = torch.repeat_interleave(torch.arange(shape[mode], device=dev), torch.diff(m['rowptr']).long())
            ia, ib = m['idx_a'].long(), m['idx_b'].long()

            def restore():
                fs[mode].copy_(start[mode])

            def torch_step():
                kr = pa.index_select(0, ia) * pb.index_select(0, ib)
                s = (fs[mode].index_select(0, own) * kr).sum(1)
                gn, gp = (m['vals'] / (s + eps), torch.ones_like(s)) if beta == 1.0 else (m['vals'], s)
                num = torch.zeros_like(fs[mode]).index_add_(0, own, gn[:, None] * kr)
                den = torch.zeros_like(fs[mode]).index_add_(0, own, gp[:, None] * kr)
                fs[mode].mul_((num.clamp_min(0) + eps) / (den.clamp_min(0) + eps))
            routes = {f'stage{s}': (lambda s=s: ntf._sparse_call(T, fs, mode, beta, unstored, step=step, stage=s)) for s in (1, 2, 0)}
            if unstored == 'missing' and dense_too:
                routes['dense_weighted'] = lambda: ntf._ntf_call(D, fs, mode, beta, step=step)
            result = {}

            def keep(k):
                result[k] = fs[mode].clone()
            t = timed(routes, restore, keep)
            if unstored == 'missing':
                t.update(timed(dict(torch=torch_step), restore, keep))
            losses = [float(ntf._sparse_loss(T, start, beta, unstored, stage=s).item()) for s in (1, 2)]
            staged = [rows <= cap for rows in (pa.shape[0], pb.shape[0])]
            row = dict(shape=list(shape), nnz=T.nnz, rank=RANK, unstored=unstored, beta=beta, mode=mode, rows=shape[mode],
                       segments=int(m['seg'].shape[0]), panels_that_fit_lds=staged,
                       stage1_equals_stage2=bool(torch.equal(result['stage1'], result['stage2'])) and losses[0] == losses[1],
                       **t)
            if 'torch' in result:
                row['torch']['max_rel_diff_to_kernel'] = float(((result['torch'] - result['stage1']).abs() / result['stage1']).max())
            for s, st in (('stage1', [False, False]), ('stage2', staged)):
                per = 12 + 4 * RANK * (2 - sum(st))
                row[s].update(bytes_per_entry=per, fraction_of_hbm=(per * T.nnz + 8.0 * RANK * shape[mode]) /
                              (t[s]['median_ms'] * 1e-3) / HBM_PEAK)
            emit(row)
        if masked_too and unstored == 'missing':
            for side, owner, panel in (('h', 0, 1), ('w', 1, 0)):
                fs = [f.clone() for f in start[:2]]
                t = timed(dict(masked=lambda: SA._masked_call(M2, side, fs[owner], fs[panel], beta, step=step)),
                          lambda: fs[owner].copy_(start[owner]))
                emit(dict(shape=list(shape[:2]), nnz=M2.nnz, rank=RANK, unstored='missing', beta=beta, side=side,
                          rows=shape[owner], one_gather=dict(t['masked'], bytes_per_entry=8 + 4 * RANK)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_ntf.json'))
    ap.add_argument('--item', choices=list(WORKLOADS), help='run ONE workload in this process (the driver calls this)')
    a = ap.parse_args()
    if a.item:
        import torch
        rows = []
        run(**WORKLOADS[a.item], emit=rows.append)
        print('ITEM_RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rows=rows)), flush=True)
        return 0
    res = dict(tool='tools/bench_sparse_ntf.py', warmup=WARMUP, repeats=REPEATS, calls_per_window=CALLS, hbm_peak=HBM_PEAK,
               rows=[], failed=None)
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
