#!/usr/bin/env python3
"""Time ``model_selection.cross_validate`` beside the loop a user had without it, the unweighted batch beside the parent
commit's, and the weighted batch beside the unweighted one:

    python tools/bench_cross_validate.py [--parent-tree <checkout of the parent commit, library built>] [--out profiles/cross_validate.json]

  cv          cross_validate(V, ranks (8, 16, 32), 5 folds, 2 starts, 100 iterations, beta 1) on a 5168 x 1025 target (the
              reference's published shape) and on a 513 x 128 one, against the same 30 fits as a Python loop of
              ``NMF.fit(V, weights=train_k)`` + ``weighted_beta_div(H, W, V, test_k)`` on the same masks
  unweighted  the three shapes of tools/bench_batched.py, ``BatchedNMF.fit`` without weights, beta 1: this tree against the
              parent tree (skipped without --parent-tree), each pass in a process of its own, the trees alternating.  The
              parent tree is passed TWICE per repeat (arms ``parent`` and ``parent_again``): the same code against itself
              is the measured run-to-run spread that a difference has to be read against
  weighted    512 targets of 513 x 128 at rank 16: ``fit(V, weights=M)`` with (B, N, C) weights against ``fit(V)``

As in tools/bench_batched.py: every fit runs a fixed number of iterations (tol = -1e9), the arms alternate, three repeats after
one warm-up pass of each, a pass is timed with device events from its first enqueue to its last kernel; reported are medians
with min - max.  Every item runs in a child process under its own time limit, one after the other; the first that fails ends
the run (no retries) and what finished is still written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_SHAPES = {'published_5168x1025': (5168, 1025), 'clip_513x128': (513, 128)}
CV_RANKS, CV_FOLDS, CV_STARTS, CV_BETA = (8, 16, 32), 5, 2, 1.0
BATCH_SHAPES = {'clips_513x128_r16': (512, 513, 128, 16, False), 'tiny_64x64_r8': (4096, 64, 64, 8, False),
                'restarts_5168x1025_r88': (32, 5168, 1025, 88, True)}      # tools/bench_batched.py
ITERATIONS, REPEATS = 100, 3
NEVER = -1e9
ITEM_LIMIT_S = 400


def _events(torch):
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _timed(torch, fn):
    a, b = _events(torch)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _summary(t):
    return dict(ms=statistics.median(t), ms_min=min(t), ms_max=max(t))


def run_cv(name):
    import torch
    from torchnmf_amd.metrics import weighted_beta_div
    from torchnmf_amd.model_selection import cross_validate, draw_starts, holdout_masks, problem_layout
    from torchnmf_amd.nmf import NMF
    N, C = CV_SHAPES[name]
    dev = torch.device('cuda:0')
    V = torch.rand(N, C, generator=torch.Generator(device=dev).manual_seed(3), device=dev) + 0.1
    B = CV_FOLDS * CV_STARTS
    _, k_of, _ = problem_layout(1, CV_FOLDS, CV_STARTS)

    def batched(max_iter):
        res = cross_validate(V, CV_RANKS, beta=CV_BETA, folds=CV_FOLDS, n_init=CV_STARTS, tol=NEVER, max_iter=max_iter,
                             generator=torch.Generator().manual_seed(7))
        assert bool((res.n_iter == max_iter).all())
        return res.test_loss

    def loop(max_iter):
        g = torch.Generator().manual_seed(7)
        train, test = holdout_masks((N, C), CV_FOLDS, g, device=dev)
        out = torch.empty(len(CV_RANKS), 1, CV_FOLDS, CV_STARTS, dtype=torch.float64)
        for i, R in enumerate(CV_RANKS):
            W0, H0 = draw_starts(B, N, C, R, g)
            for b in range(B):
                k = int(k_of[b])
                m = NMF(W=W0[b], H=H0[b]).to(dev)
                assert m.fit(V, beta=CV_BETA, tol=NEVER, max_iter=max_iter, weights=train[k]) == max_iter
                out[i, 0, k, b % CV_STARTS] = float(weighted_beta_div(m.H.data, m.W.data, V, test[k], CV_BETA))
        return out
    arms = {'cross_validate': batched, 'loop': loop}
    first = {arm: fn(10) for arm, fn in arms.items()}       # warm-up; the two arms fit the same problems from the same starts
    agree = float(((first['loop'] - first['cross_validate']) / first['cross_validate']).abs().max())
    times = {arm: [] for arm in arms}
    for _ in range(REPEATS):
        for arm, fn in arms.items():
            times[arm].append(_timed(torch, lambda: fn(ITERATIONS)))
    rows = [dict(part='cv', shape=name, n=N, c=C, ranks=list(CV_RANKS), folds=CV_FOLDS, n_init=CV_STARTS, beta=CV_BETA,
                 iterations=ITERATIONS, fits=len(CV_RANKS) * B, arm=arm, **_summary(t)) for arm, t in times.items()]
    rows.append(dict(part='cv', shape=name, arm='ratio', loop_over_cross_validate=rows[1]['ms'] / rows[0]['ms'],
                     test_loss_worst_relative_difference_after_10_iterations=agree))
    return rows


def run_batch_pass(tree):
    """ONE timed pass per shape (after one warm-up pass) of the unweighted batch of the tree at ``tree``; beta 1."""
    sys.path.insert(0, os.path.join(tree, 'pytorch-nmf_amd'))
    import torch
    from torchnmf_amd.batched import BatchedNMF
    dev = torch.device('cuda:0')
    rows = []
    for name, (B, N, C, R, shared) in BATCH_SHAPES.items():
        V = torch.rand((N, C) if shared else (B, N, C), generator=torch.Generator(device=dev).manual_seed(3), device=dev) + 0.1
        torch.manual_seed(1)
        W0, H0 = torch.randn(B, C, R).abs(), torch.randn(B, N, R).abs()

        def fit(max_iter):
            m = BatchedNMF(W=W0, H=H0).to(dev)
            assert m.fit(V, beta=1.0, tol=NEVER, max_iter=max_iter).tolist() == [max_iter] * B
        fit(10)
        rows.append(dict(shape=name, ms_per_fit=_timed(torch, lambda: fit(ITERATIONS)) / B))
        del V
    return rows


def run_weighted():
    import torch
    from torchnmf_amd.batched import BatchedNMF
    B, N, C, R, _ = BATCH_SHAPES['clips_513x128_r16']
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(3)
    V = torch.rand(B, N, C, generator=g, device=dev) + 0.1
    M = (torch.rand(B, N, C, generator=g, device=dev) * 3.75 + 0.25) * (torch.rand(B, N, C, generator=g, device=dev) < 0.7)
    torch.manual_seed(1)
    W0, H0 = torch.randn(B, C, R).abs(), torch.randn(B, N, R).abs()

    def fit(max_iter, **kw):
        m = BatchedNMF(W=W0, H=H0).to(dev)
        assert m.fit(V, beta=1.0, tol=NEVER, max_iter=max_iter, **kw).tolist() == [max_iter] * B
    arms = {'unweighted': {}, 'weighted': dict(weights=M)}
    for kw in arms.values():
        fit(10, **kw)
    times = {arm: [] for arm in arms}
    for _ in range(REPEATS):
        for arm, kw in arms.items():
            times[arm].append(_timed(torch, lambda: fit(ITERATIONS, **kw)) / B)
    rows = [dict(part='weighted', shape='clips_513x128_r16', batch=B, n=N, c=C, rank=R, beta=1.0, iterations=ITERATIONS, arm=arm,
                 unit='ms per fit', **_summary(t)) for arm, t in times.items()]
    rows.append(dict(part='weighted', shape='clips_513x128_r16', arm='ratio', weighted_over_unweighted=rows[1]['ms'] / rows[0]['ms']))
    return rows


def _child(args, limit=ITEM_LIMIT_S):
    """The rows an item prints from a process of its own; (None, why) when it fails."""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, dict(item=args, why=f'time limit of {limit} s', rc=124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('ITEM_RESULT ')]
    if p.returncode != 0 or not line:
        return None, dict(item=args, why=f'exit status {p.returncode}', stderr=p.stderr[-2000:], rc=p.returncode or 1)
    return json.loads(line[-1][len('ITEM_RESULT '):]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cross_validate.json'))
    ap.add_argument('--parent-tree', help='a checkout of the parent commit with its library built')
    ap.add_argument('--item', nargs='+', help='run ONE item in this process and print its rows (the driver calls this)')
    a = ap.parse_args()
    if a.item:
        kind = a.item[0]
        if kind != 'batch_pass':
            sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
        rows = run_cv(a.item[1]) if kind == 'cv' else run_batch_pass(a.item[1]) if kind == 'batch_pass' else run_weighted()
        print('ITEM_RESULT ' + json.dumps(rows), flush=True)
        return 0
    res = dict(tool='tools/bench_cross_validate.py', iterations=ITERATIONS, repeats=REPEATS, rows=[], failed=None)

    def finish(rc):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print('wrote', a.out)
        return rc
    items = [['cv', name] for name in reversed(list(CV_SHAPES))] + [['weighted']]
    for item in items:               # chained: the first failure ends the run, nothing is tried again
        rows, why = _child(['--item'] + item)
        if why:
            res['failed'] = why
            return finish(why['rc'])
        res['rows'] += rows
        for r in rows:
            print(json.dumps(r), flush=True)
    if a.parent_tree:
        trees = {'parent': os.path.abspath(a.parent_tree), 'child': ROOT, 'parent_again': os.path.abspath(a.parent_tree)}
        t = {(tree, shape): [] for tree in trees for shape in BATCH_SHAPES}
        for _ in range(REPEATS):     # alternating trees, a process per pass
            for tree, path in trees.items():
                rows, why = _child(['--item', 'batch_pass', path])
                if why:
                    res['failed'] = why
                    return finish(why['rc'])
                for r in rows:
                    t[(tree, r['shape'])].append(r['ms_per_fit'])
        for shape in BATCH_SHAPES:
            p, c, again = t[('parent', shape)], t[('child', shape)], t[('parent_again', shape)]
            for tree, v in (('parent', p), ('child', c), ('parent_again', again)):
                res['rows'].append(dict(part='unweighted', shape=shape, arm=tree, beta=1.0, iterations=ITERATIONS,
                                        unit='ms per fit', passes=v, **_summary(v)))
            # the child's median within the parent's min - max, widened on either side by the run-to-run spread measured
            # in this session: max - min over the six passes of the parent's code
            spread = max(p + again) - min(p + again)
            row = dict(part='unweighted', shape=shape, arm='verdict', same_code_spread_ms=spread,
                       child_over_parent=statistics.median(c) / statistics.median(p),
                       child_median_within_widened_parent_range=min(p) - spread <= statistics.median(c) <= max(p) + spread)
            res['rows'].append(row)
        for r in res['rows']:
            if r['part'] == 'unweighted':
                print(json.dumps(r), flush=True)
    import torch
    res['device'] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    return finish(0)


if __name__ == '__main__':
    sys.exit(main())
