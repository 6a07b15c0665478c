#!/usr/bin/env python3
"""Time ``fold_in`` -- new rows folded into a fitted model, every iteration of every row in ONE launch -- beside the two
routes a user had before it, in the same run on the same rows:

    python tools/bench_fold_in.py [--out profiles/fold_in.json]

  fold_in  metrics.fold_in(W, T, beta, 50, tol=0, unstored=..., H0=H0): the set-up (a sort of the row counts; the column
           sums of W under 'zero') and one nmfmu_fold_in launch
  loop     50 calls of MaskedMU.h_step ('missing') / SparseMU.h_step ('zero') with W frozen, the engine built beforehand
  fit      NMF(W=W, H=H0, trainable_W=False).fit(V_new, beta, max_iter=50, unstored=...), module and engine built inside the
           timed region (what the call costs a user), loss checkpoints every tenth iteration as ``fit`` has them (with a
           ``tol`` that cannot fire, so that all 50 iterations run)

Fixed inputs: the target of tools/bench_masked.py -- 65 536 new rows x 16 384, 10 M stored entries with power-law degrees --
rank 64, 50 iterations; beta = 1 in both modes, beta = 2 and 0.5 under 'missing'; then the first 256 rows and one row of
median length alone (serving latency).  Device events, 2 warm-ups, then the median of 10 with min - max; the arms alternate.

``gather``: bytes of index + value + W row (8 + 4 R per stored entry) the kernel fetches -- once for the rows whose entries fit
one LDS block (``staged``), and per iteration for the longer ones (``restaged``).  With ``tol = 1e-4`` and max_iter = 200: the
time and the distribution of the per-row iteration counts.
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
from bench_masked import C, R, make_target, summary  # noqa: E402
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.fold_in import fold_in  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from torchnmf_amd.nmf import NMF  # noqa: E402
from torchnmf_amd.sparse_engine import MaskedMU, SparseMU  # noqa: E402

ITERS = 50
CASES = (('missing', 1.0), ('zero', 1.0), ('missing', 2.0), ('missing', 0.5))
SIZES = (65536, 256, 1)
WARMUP, REPEATS = 2, 10


def timed(fns):
    for _ in range(WARMUP):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(REPEATS):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return times


def take_rows(V, start, n):
    idx, vals = V.indices(), V.values()
    keep = (idx[0] >= start) & (idx[0] < start + n)
    sub = idx[:, keep].clone()
    sub[0] -= start
    return torch.sparse_coo_tensor(sub, vals[keep], (n, V.shape[1])).coalesce()


def gather_bytes(counts, block):
    per = 8 + 4 * R
    # one wave keeps a row of <= block entries, a workgroup (rows above block) one of <= 4 * block: ceil(count / 4) per wave
    fits = (counts <= block) | ((counts + 3) // 4 <= block)
    staged = counts[fits].sum().item()
    rest = counts[~fits].sum().item()
    return dict(block=block, long_rows=block, rows_staged=int(fits.sum()), rows_restaged=int((~fits).sum()),
                rows_on_a_workgroup=int((counts > block).sum()), staged_once_bytes=int(staged * per),
                restaged_bytes_per_iteration=int(rest * per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fold_in.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = _capi.load()
    block = lib.nmfmu_fold_in_block(R)
    V_all = make_target(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    H_all = torch.rand(V_all.shape[0], R, generator=g, device=dev) + 0.05
    W = torch.rand(C, R, generator=g, device=dev) + 0.05
    res = dict(tool='tools/bench_fold_in.py', device=torch.cuda.get_device_name(0), columns=C, rank=R, iterations=ITERS,
               warmup=WARMUP, repeats=REPEATS, sizes={})
    for n in SIZES:
        # the first n rows; the single row is one of median length
        start = 0
        if n == 1:
            c_all = torch.bincount(V_all.indices()[0], minlength=V_all.shape[0]).float()
            start = int((c_all - c_all.median()).abs().argmin())
        V = take_rows(V_all, start, n)
        T = SparseTarget(V)
        H0 = H_all[start:start + n].contiguous()
        counts = torch.diff(T.csr[0].long())
        entry = dict(rows=n, nnz=T.nnz, count_max=int(counts.max()), count_median=float(counts.float().median()),
                     gather=gather_bytes(counts, block), cases={})
        for mode, beta in CASES:
            Hl = H0.clone()
            Eng = MaskedMU if mode == 'missing' else SparseMU
            eng = Eng(T if mode == 'missing' else V, W.clone(), Hl, beta, update_W=False)

            def run_fold():
                return fold_in(W, T, beta, ITERS, 0.0, unstored=mode, H0=H0)

            def run_loop():
                for _ in range(ITERS):
                    eng.h_step()

            def run_fit():
                m = NMF(W=W, H=H0, trainable_W=False).to(dev)
                m.fit(V, beta=beta, tol=-1e9, max_iter=ITERS, unstored=mode)
                return m
            # the three routes compute the same 50 iterations
            Hl.copy_(H0)
            run_loop()
            got = run_fold()
            agree = dict(loop=float((got - Hl).norm() / Hl.norm()),
                         fit=float((got - run_fit().H.data).norm() / Hl.norm()))
            tf, tl, tt = timed([run_fold, run_loop, run_fit])
            med = statistics.median(tf)
            case = dict(fold_in=summary(tf), loop=summary(tl), fit=summary(tt), loop_over_fold_in=statistics.median(tl) / med,
                        fit_over_fold_in=statistics.median(tt) / med, rel_diff_after_50=agree)
            if (mode, beta) == ('missing', 1.0):      # every row stopped on its own
                def run_tol():
                    return fold_in(W, T, beta, 200, 1e-4, unstored=mode, H0=H0, return_n_iter=True)
                cnt = run_tol()[1].float()
                q = torch.tensor([0.0, 0.1, 0.5, 0.9, 0.99, 1.0], device=dev)
                case['tol_1e-4_max_iter_200'] = dict(fold_in=summary(timed([run_tol])[0]),
                                                     count_quantiles_0_10_50_90_99_100=torch.quantile(cnt, q).tolist(),
                                                     count_mean=float(cnt.mean()), rows_at_max_iter=int((cnt == 200).sum()))
            entry['cases'][f'{mode}_b{beta:g}'] = case
            print(n, mode, beta, json.dumps(case), flush=True)
            del eng
        res['sizes'][str(n)] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
