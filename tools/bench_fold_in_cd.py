#!/usr/bin/env python3
"""Time fold-in by coordinate descent -- ``fold_in_cd(solver='ccd' | 'hals')``: every iteration of every new row in ONE launch of
``nmfmu_fold_in_cd`` -- beside the route that existed before it, in the same run on the same rows:

    python tools/bench_fold_in_cd.py [--out profiles/fold_in_cd.json]

  cd       metrics.fold_in_cd(W, T, 2, 50, tol=0, unstored=..., solver=..., H0=H0): the set-up (a sort of the row counts; one
           nmfmu_gram for omega > 0) and the one launch
  chained  50 H-side sweeps of the kernels ``fit`` drives, W frozen, everything a sweep does not need built beforehand:
           ``wccd._WSide.wsweep`` with the Gram matrix given (0.05), ``ccd._Side.sweep`` ('missing'), ``hals.hals_sweep`` with
           ``A = V_new W`` and ``G = W^T W`` given ('zero').  Two launches per sweep (one for 'zero'); d_k and the row's W rows
           fetched again by every sweep
  mu       for context, metrics.fold_in(..., beta=2) in the two modes it has

Fixed inputs: the target of tools/bench_fold_in.py -- 65 536 new rows x 16 384, 10 M stored entries with power-law degrees --
rank 64, 50 iterations; then its first 256 rows (one of them stores 4 092 entries) and one row of median length alone.
Device events, 2 warm-ups, then the median of 10 with min - max; the arms alternate.

With ``tol = 1e-4`` and max_iter = 200 on the 65 536 rows: the time and the distribution of the per-row iteration counts, CD
beside MU -- the same stop rule on both.
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
from bench_fold_in import take_rows, timed  # noqa: E402
from bench_masked import C, R, make_target, summary  # noqa: E402
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.ccd import _Side  # noqa: E402
from torchnmf_amd.fold_in import fold_in, fold_in_cd  # noqa: E402
from torchnmf_amd.hals import hals_sweep  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from torchnmf_amd.wccd import _WSide  # noqa: E402

ITERS = 50
OMEGA = 0.05
MODES = (OMEGA, 'missing', 'zero')
SIZES = (65536, 256, 1)


def paths(counts, block, long_rows):
    """Which rows the kernel stages (the W rows fetched once) and which gather at every use."""
    share = torch.where(counts > long_rows, (counts + 3) // 4, counts)
    staged = share <= block
    return dict(block=block, long_rows=long_rows, rows_on_a_workgroup=int((counts > long_rows).sum()),
                rows_staged=int(staged.sum()), rows_gathering=int((~staged).sum()),
                entries_staged=int(counts[staged].sum()), entries_gathering=int(counts[~staged].sum()))


def quantiles(cnt):
    q = torch.tensor([0.0, 0.1, 0.5, 0.9, 0.99, 1.0], device=cnt.device)
    cnt = cnt.float()
    return dict(count_quantiles_0_10_50_90_99_100=torch.quantile(cnt, q).tolist(), count_mean=float(cnt.mean()),
                rows_at_max_iter=int((cnt == 200).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fold_in_cd.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = _capi.load()
    block, long_rows = lib.nmfmu_fold_in_cd_block(R), lib.nmfmu_fold_in_cd_long_rows(R)
    V_all = make_target(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    H_all = torch.rand(V_all.shape[0], R, generator=g, device=dev) + 0.05
    W = torch.rand(C, R, generator=g, device=dev) + 0.05
    G = (W.double().t() @ W.double()).float().contiguous()
    res = dict(tool='tools/bench_fold_in_cd.py', device=torch.cuda.get_device_name(0), columns=C, rank=R, iterations=ITERS,
               omega=OMEGA, warmup=2, repeats=10, sizes={})
    for n in SIZES:
        start = 0
        if n == 1:
            c_all = torch.bincount(V_all.indices()[0], minlength=V_all.shape[0]).float()
            start = int((c_all - c_all.median()).abs().argmin())
        V = take_rows(V_all, start, n)
        T = SparseTarget(V)
        H0 = H_all[start:start + n].contiguous()
        counts = torch.diff(T.csr[0].long())
        entry = dict(rows=n, nnz=T.nnz, count_max=int(counts.max()), count_median=float(counts.float().median()),
                     paths=paths(counts, block, long_rows), cases={})
        for mode in MODES:
            solver = 'hals' if mode == 'zero' else 'ccd'
            Hc = H0.clone()
            if mode == 'zero':
                A = torch.sparse.mm(V, W).contiguous()

                def sweep():
                    hals_sweep(Hc, A, G)
            elif mode == 'missing':
                side = _Side(T, 'h', R)

                def sweep():
                    side.sweep(Hc, W, 0.0, 0.0)
            else:
                side = _WSide(T, 'h', R)

                def sweep():
                    side.wsweep(Hc, W, G, OMEGA, 0.0, 0.0)

            def run_cd():
                return fold_in_cd(W, T, 2, ITERS, 0.0, unstored=mode, solver=solver, H0=H0)

            def run_chained():
                Hc.copy_(H0)
                for _ in range(ITERS):
                    sweep()
            run_chained()
            got = run_cd()
            arms, names = [run_cd, run_chained], ['cd', 'chained']
            if mode != OMEGA:
                def run_mu():
                    return fold_in(W, T, 2, ITERS, 0.0, unstored=mode, H0=H0)
                arms.append(run_mu)
                names.append('mu')
            ts = timed(arms)
            case = {k: summary(t) for k, t in zip(names, ts)}
            case['chained_over_cd'] = statistics.median(ts[1]) / statistics.median(ts[0])
            if mode != OMEGA:
                case['mu_over_cd'] = statistics.median(ts[2]) / statistics.median(ts[0])
            case['rel_diff_cd_vs_chained_after_50'] = float((got - Hc).norm() / Hc.norm())
            if n == SIZES[0]:                    # every row stopped on its own: CD beside MU under the same rule
                def tol_cd():
                    return fold_in_cd(W, T, 2, 200, 1e-4, unstored=mode, solver=solver, H0=H0, return_n_iter=True)
                arms, names = [tol_cd], ['cd']
                if mode != OMEGA:
                    def tol_mu():
                        return fold_in(W, T, 2, 200, 1e-4, unstored=mode, H0=H0, return_n_iter=True)
                    arms.append(tol_mu)
                    names.append('mu')
                tt = timed(arms)
                case['tol_1e-4_max_iter_200'] = {k: dict(summary(t), **quantiles(f()[1])) for k, t, f in zip(names, tt, arms)}
            entry['cases'][str(mode)] = case
            print(n, mode, json.dumps(case), flush=True)
        res['sizes'][str(n)] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
