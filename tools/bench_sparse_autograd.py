#!/usr/bin/env python3
"""Time ``sparse_beta_div`` forward + backward against the composition the library offered before it for the same gradients,
on an evenly loaded and on a skewed (Zipf row and column degrees) sparse target of the same nnz, and sweep ``chunk``.

    python tools/bench_sparse_autograd.py [--n 32768] [--density 0.01] [--rank 64] [--out profiles/sparse_autograd.json]

  new          loss = sparse_beta_div(H, W, T, beta); loss.backward()       (both gradients; segments of `chunk` entries)
  composition  nmfmu_sp_loss_neg + 2 x nmfmu_sp_partial (one wave per whole owner row) + nmfmu_rank_sums (beta 1) or
               nmfmu_gram / nmfmu_rowmat (beta 2) + the torch subtraction -- the same loss and gradients from the entries the
               sparse MU engine is built on
Both run in the same process, alternating, timed with device events: 2 warm-up calls, then the median of 10 with min - max.

Bytes (``traffic_bytes``): per stored entry the forward reads index + value (8 B) and one panel row (4 R), and at beta == 1
writes s (4 B); each backward side reads index + value (8 B), at beta == 1 s (4 B) and on the W side perm (4 B), and one
panel row (4 R); the outputs are (N + C) r_pad floats (beta == 2: their pos planes are written and read once more).  The
achieved rate is to be read against the register-gather rates of random whole rows on this chip (5.5 - 5.8 TB/s from
HBM, more from the caches: a factor of 32768 x 64 floats is 8 MiB).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.metrics import SparseTarget, sparse_beta_div  # noqa: E402

WARMUP, REPEATS = 2, 10


def make_pattern(kind, n, nnz, dev, seed):
    """A coalesced sparse n x n tensor with exactly nnz stored entries.  'even': uniform positions.  'skewed': row and column
    degrees proportional to rank^-1/2 of a random order (a top row near n entries against a median of a few hundred)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if kind == 'even':
        lin = torch.randint(n * n, (int(nnz * 1.05),), generator=g, device=dev)
    else:
        w = torch.arange(1, n + 1, device=dev, dtype=torch.float32).pow(-0.5)
        draw = int(nnz * 1.6)
        rows = torch.randperm(n, generator=g, device=dev)[torch.multinomial(w, draw, replacement=True, generator=g)]
        cols = torch.randperm(n, generator=g, device=dev)[torch.multinomial(w, draw, replacement=True, generator=g)]
        lin = rows * n + cols
    lin = torch.unique(lin)
    assert lin.numel() >= nnz, (kind, lin.numel(), nnz)
    lin = lin[torch.randperm(lin.numel(), generator=g, device=dev)[:nnz]]
    vals = torch.rand(nnz, generator=g, device=dev) + 0.1
    return torch.sparse_coo_tensor(torch.stack([lin // n, lin % n]), vals, (n, n)).coalesce()


def degree_stats(T):
    out = {}
    for name, ptr in (('row', T.csr[0]), ('col', T.csc[0])):
        d = torch.diff(ptr.long()).float()
        out[name] = dict(max=int(d.max()), median=float(d.median()), mean=float(d.mean()))
    return out


def traffic_bytes(n_rows, n_cols, nnz, rank, r_pad, beta):
    fwd = nnz * (8 + 4 * rank + (4 if beta == 1 else 0))
    bwd = nnz * (2 * (8 + 4 * rank) + (4 + 4 + 4 if beta == 1 else 0))
    out = (n_rows + n_cols) * r_pad * 4 * (3 if beta == 2 else 1)
    return fwd + bwd + out


def timed(fns, repeats=REPEATS, warmup=WARMUP):
    """Alternates the callables; returns per callable the list of times in ms."""
    for _ in range(warmup):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return times


def summary(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def new_path(H, W, T, beta):
    def run():
        H.grad = W.grad = None
        sparse_beta_div(H, W, T, beta).backward()
    return run


def composition(H, W, T, beta):
    """The parent's entries for the same loss and gradients (whole owner rows per wave)."""
    lib = _capi.load()
    Hc, Wc = H.detach(), W.detach()
    N, R = Hc.shape
    C = Wc.shape[0]
    r_pad = lib.nmfmu_pad_rank(R)
    dev = Hc.device
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def run():
        part = torch.empty((N + 3) // 4, dtype=torch.float64, device=dev)
        neg = torch.empty(1, dtype=torch.float64, device=dev)
        rp, ci, v = T.csr
        _capi.check(lib.nmfmu_sp_loss_neg(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), N, Hc.data_ptr(), Wc.data_ptr(), R,
                                          float(beta), part.data_ptr(), neg.data_ptr(), s()), 'nmfmu_sp_loss_neg')
        small = []
        if beta == 1:
            sp = torch.empty(R * 128, dtype=torch.float32, device=dev)
            for f in (Hc, Wc):
                cs = torch.empty(R, dtype=torch.float32, device=dev)
                _capi.check(lib.nmfmu_rank_sums(f.data_ptr(), f.shape[0], R, 1, sp.data_ptr(), cs.data_ptr(), s()), 'rank_sums')
                small.append(cs)
            pos = small[0].double() @ small[1].double()
        else:
            gp = torch.empty(lib.nmfmu_gram_part_bytes(R) // 4, dtype=torch.float32, device=dev)
            for f in (Hc, Wc):
                g = torch.empty(R * R, dtype=torch.float32, device=dev)
                _capi.check(lib.nmfmu_gram(f.data_ptr(), f.shape[0], R, gp.data_ptr(), g.data_ptr(), s()), 'nmfmu_gram')
                small.append(g)
            pos = 0.5 * (small[0].double() @ small[1].double())
        loss = (T.v_norm(float(beta)) + pos - neg[0]).float()
        grads = []
        for (ptr, idx, vals), own, pan, sm in ((T.csr, Hc, Wc, small[1]), (T.csc, Wc, Hc, small[0])):
            rows = own.shape[0]
            num = torch.empty(rows, r_pad, dtype=torch.float32, device=dev)
            _capi.check(lib.nmfmu_sp_partial(ptr.data_ptr(), idx.data_ptr(), vals.data_ptr(), rows, own.data_ptr(),
                                             pan.data_ptr(), R, float(beta), num.data_ptr(), r_pad, s()), 'nmfmu_sp_partial')
            if beta == 1:
                grads.append(sm[None, :] - num[:, :R])
            else:
                den = torch.empty(rows, r_pad, dtype=torch.float32, device=dev)
                _capi.check(lib.nmfmu_rowmat(own.data_ptr(), rows, R, sm.data_ptr(), den.data_ptr(), r_pad, s()), 'nmfmu_rowmat')
                grads.append((den - num)[:, :R])
        return loss, grads
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32768)
    ap.add_argument('--density', type=float, default=0.01)
    ap.add_argument('--rank', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_autograd.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = _capi.load()
    n, R = a.n, a.rank
    nnz = int(a.density * n * n)
    r_pad = lib.nmfmu_pad_rank(R)
    g = torch.Generator(device=dev).manual_seed(1)
    H = (torch.rand(n, R, generator=g, device=dev) + 0.05).requires_grad_()
    W = (torch.rand(n, R, generator=g, device=dev) + 0.05).requires_grad_()
    res = dict(device=torch.cuda.get_device_name(0), n=n, nnz=nnz, rank=R, r_pad=r_pad, warmup=WARMUP, repeats=REPEATS,
               patterns={}, chunk_sweep={})
    targets = {}
    for kind in ('even', 'skewed'):
        V = make_pattern(kind, n, nnz, dev, seed=2)
        targets[kind] = V
        T = SparseTarget(V)
        entry = dict(degrees=degree_stats(T), chunk=T.chunk, segments=dict(h=T.seg_h.shape[0], w=T.seg_w.shape[0]),
                     split_rows=dict(h=T.multi_h.shape[0], w=T.multi_w.shape[0]))
        for beta in (1, 2):
            # the two paths give the same gradients (checked once, outside the timing)
            loss_c, (gh, gw) = composition(H, W, T, beta)()
            new_path(H, W, T, beta)()
            agree = dict(H=float((H.grad - gh).norm() / gh.norm()), W=float((W.grad - gw).norm() / gw.norm()))
            tn, tc = timed([new_path(H, W, T, beta), composition(H, W, T, beta)])
            by = traffic_bytes(n, n, nnz, R, r_pad, beta)
            entry[f'beta{beta}'] = dict(new=summary(tn), composition=summary(tc), new_over_composition=statistics.median(tn) /
                                        statistics.median(tc), bytes=by, new_tb_per_s=by / statistics.median(tn) / 1e9,
                                        gradients_rel_diff=agree)
            print(kind, beta, json.dumps(entry[f'beta{beta}']), flush=True)
        res['patterns'][kind] = entry
    for beta in (1, 2):
        res[f'skew_over_even_beta{beta}'] = {
            k: res['patterns']['skewed'][f'beta{beta}'][k]['median_ms'] / res['patterns']['even'][f'beta{beta}'][k]['median_ms']
            for k in ('new', 'composition')}
    print(json.dumps({k: v for k, v in res.items() if k.startswith('skew_over')}), flush=True)
    for beta in (1, 2):
        Ts = {str(c): SparseTarget(targets['skewed'], chunk=c) for c in (256, 512, 2048, None)}
        ts = timed([new_path(H, W, T, beta) for T in Ts.values()])
        res['chunk_sweep'][f'beta{beta}'] = {('unsplit' if k == 'None' else k): dict(summary(t), segments_h=T.seg_h.shape[0])
                                             for (k, T), t in zip(Ts.items(), ts)}
        print('chunk sweep beta', beta, json.dumps(res['chunk_sweep'][f'beta{beta}']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
