#!/usr/bin/env python3
"""Time ``scoring.rank_scores`` -- the rank of every held-out pair among all columns the training set does not store -- beside
the only thing a user could do without it, in the same run on the same factors and split:

    python tools/bench_rank.py [--out profiles/rank.json]

  fused   scoring.rank_scores(H, W, heldout, exclude=train): nmfmu_rank_pairs (extract pass, count pass, merge)
  torch   on the device, in row chunks: ``H[chunk] @ W.T``, the held-out scores gathered, ``-inf`` written at the chunk's
          train positions, and per block of held-out pairs the comparison of the pair's row of scores against the pair's score
          under the same (score, column) order, summed (chunk and block boundaries are found outside the timed region)

Fixed inputs: 65 536 x 16 384, rank 64, the 10 M-entry power-law target of tools/bench_masked.py split 80 / 20 into ``exclude``
(train) and ``heldout``, all rows; factors uniform in [0.05, 1.05).  Device events, 2 warm-ups, then the median of 10 with
min - max; the two paths alternate.  Peak allocated bytes per path above what is resident before the call.

Also timed, each alone: the three passes of the fused path; the count pass with the ballot form, the scan form and the
per-row choice on all rows, and with other thresholds between the forms (SWEEP); the two forms on the rows ABOVE
scoring.RANK_SCAN_ABOVE held-out pairs only.
``f32_matrix_fraction``: the two tile passes' 2 x 2 n_rows C R flops over their time, against the 155 TF measured f32 MFMA rate.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from torchnmf_amd import _capi, scoring  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from bench_masked import C, N, NNZ, R, REPEATS, WARMUP, make_target, summary  # noqa: E402
from bench_topk import F32_MATRIX_TF, overlap, timed_with_peak  # noqa: E402

CHUNK = 4096                 # rows per baseline chunk: 4096 x 16384 fp32 = 268 MB
PAIR_BLOCK = 8192            # held-out pairs per comparison block: 8192 x 16384 fp32 = 537 MB gathered
TRAIN_FRACTION = 0.8
SWEEP = (8, 16, 32, 48, 64)   # count pass with the scan form above this many held-out pairs (nmfmu_rank_pass form > 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = _capi.load()
    V = make_target(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    train = torch.rand(NNZ, generator=g, device=dev) < TRAIN_FRACTION
    idx, vals = V.indices(), V.values()
    Vtrain = torch.sparse_coo_tensor(idx[:, train], vals[train], (N, C)).coalesce()
    Vtest = torch.sparse_coo_tensor(idx[:, ~train], vals[~train], (N, C)).coalesce()
    Ttrain, Ttest = SparseTarget(Vtrain), SparseTarget(Vtest)
    H = torch.rand(N, R, generator=g, device=dev) + 0.05
    W = torch.rand(C, R, generator=g, device=dev) + 0.05
    tr, tc = Vtrain.indices()[0].contiguous(), Vtrain.indices()[1].contiguous()
    hr, hc = Vtest.indices()[0].contiguous(), Vtest.indices()[1].contiguous()
    starts = list(range(0, N, CHUNK))
    bounds = torch.tensor(starts + [N], device=dev)
    tcut = torch.searchsorted(tr, bounds).tolist()      # coalesced: sorted by row
    hcut = torch.searchsorted(hr, bounds).tolist()
    colv = torch.arange(C, device=dev)

    per_row = torch.diff(Ttest.csr[0]).long()
    plan = scoring._RankPlan(H, W, Ttest, Ttrain)
    n_pairs, n_rows = plan.n, plan.n_rows
    res = dict(tool='tools/bench_rank.py', device=torch.cuda.get_device_name(0), shape=[N, C], nnz=NNZ, rank=R,
               train_entries=int(train.sum()), heldout_pairs=n_pairs, rows_with_heldout=n_rows, nsplit=plan.nsplit,
               heldout_per_row=dict(max=int(per_row.max()), median=float(per_row.float().median()),
                                    mean=float(per_row.float().mean())),
               scan_above=scoring.RANK_SCAN_ABOVE, rows_above=int((per_row > scoring.RANK_SCAN_ABOVE).sum()),
               pairs_in_rows_above=int(per_row[per_row > scoring.RANK_SCAN_ABOVE].sum()),
               warmup=WARMUP, repeats=REPEATS, baseline_chunk_rows=CHUNK, baseline_pair_block=PAIR_BLOCK)
    out = {}

    def fused():
        out['fused'] = scoring.rank_scores(H, W, Ttest, Ttrain)

    def torch_ops():
        ranks = []
        for r0, t0, t1, h0, h1 in zip(starts, tcut[:-1], tcut[1:], hcut[:-1], hcut[1:]):
            S = H[r0:r0 + CHUNK] @ W.T
            lr, lc = hr[h0:h1] - r0, hc[h0:h1]
            s = S[lr, lc]
            S[tr[t0:t1] - r0, tc[t0:t1]] = float('-inf')
            for b0 in range(0, h1 - h0, PAIR_BLOCK):
                rows_b, cb, sb = S[lr[b0:b0 + PAIR_BLOCK]], lc[b0:b0 + PAIR_BLOCK, None], s[b0:b0 + PAIR_BLOCK, None]
                ranks.append(((rows_b > sb) | ((rows_b == sb) & (colv < cb))).sum(1))
        out['torch'] = torch.cat(ranks)
    (tf, tt), (pf, pt) = timed_with_peak([fused, torch_ops])
    sf, st = summary(tf), summary(tt)
    valid = out['fused'].ranks >= 0      # (the baseline leaves a pair that the training set stores with some count)
    res['full'] = dict(fused=sf, torch=st, fused_peak_bytes=pf, torch_peak_bytes=pt,
                       torch_over_fused=st['median_ms'] / sf['median_ms'], ranges_overlap=overlap(sf, st),
                       same_ranks_fraction=float((out['fused'].ranks[valid] == out['torch'][valid]).float().mean()),
                       pairs_excluded=int((~valid).sum()))
    print('full', json.dumps(res['full']), flush=True)
    del out

    # the passes of the fused path, each alone (the plan's buffers hold a complete answer from the call above)
    stream = torch.cuda.current_stream().cuda_stream

    def one(p, form, pl):
        return lambda: _capi.check(lib.nmfmu_rank_pass(p, form, *pl.args, stream), 'nmfmu_rank_pass')
    _capi.check(lib.nmfmu_rank_pairs(*plan.args, stream), 'nmfmu_rank_pairs')
    names = ['extract', 'count_auto', 'count_ballot', 'count_scan', 'merge'] + [f'count_scan_above_{t}' for t in SWEEP]
    fns = [one(0, 0, plan), one(1, 0, plan), one(1, 1, plan), one(1, 2, plan), one(2, 0, plan)] + [one(1, t, plan) for t in SWEEP]
    times, _ = timed_with_peak(fns)
    res['passes'] = {nm: summary(t) for nm, t in zip(names, times)}
    tiles_ms = res['passes']['extract']['median_ms'] + res['passes']['count_auto']['median_ms']
    res['passes']['f32_matrix_fraction'] = 2 * 2.0 * n_rows * C * R / (tiles_ms * 1e-3) / (F32_MATRIX_TF * 1e12)
    res['passes']['extract_f32_matrix_fraction'] = (2.0 * n_rows * C * R / (res['passes']['extract']['median_ms'] * 1e-3)
                                                    / (F32_MATRIX_TF * 1e12))
    print('passes', json.dumps(res['passes']), flush=True)

    # the two forms of the count on the rows above the threshold only
    above = per_row > scoring.RANK_SCAN_ABOVE
    if bool(above.any()):
        keep = above[hr]
        Vab = torch.sparse_coo_tensor(Vtest.indices()[:, keep], Vtest.values()[keep], (N, C)).coalesce()
        pl = scoring._RankPlan(H, W, SparseTarget(Vab), Ttrain)
        _capi.check(lib.nmfmu_rank_pairs(*pl.args, stream), 'nmfmu_rank_pairs')
        times, _ = timed_with_peak([one(1, 1, pl), one(1, 2, pl), one(0, 0, pl)])
        res['rows_above_only'] = dict(rows=pl.n_rows, pairs=pl.n, nsplit=pl.nsplit, count_ballot=summary(times[0]),
                                      count_scan=summary(times[1]), extract=summary(times[2]))
        res['rows_above_only']['ballot_over_scan'] = (res['rows_above_only']['count_ballot']['median_ms']
                                                      / res['rows_above_only']['count_scan']['median_ms'])
        print('rows above', json.dumps(res['rows_above_only']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
