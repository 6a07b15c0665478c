"""Time and iterations for solver='hals' to reach the loss solver='mu' has after 200 iterations, same |randn| start; the share of a
HALS iteration spent in the Gram and sweep launches.  Dense 512^3 rank 64 in both precisions of the MTTKRP; sparse 65536 x 16384 x 24, 10 M stored, 'zero'."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-nmf_amd')]
import torch  # noqa: E402
from torchnmf_amd import _capi, ntf  # noqa: E402
from torchnmf_amd.hals import _sweep  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


def events(fn, reps=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def run(name, V, T, kw, loss, shape, R, out, precision='fp32'):
    g = torch.Generator().manual_seed(3)
    start = [torch.randn(d, R, generator=g).abs() for d in shape]
    lib = _capi.load()
    m = ntf.NTF(factors=start).cuda()
    m.fit(V, beta=2, tol=-1e9, max_iter=2, **kw)      # warm-up of every kernel
    m = ntf.NTF(factors=start).cuda()
    _, mu_ms = timed(lambda: m.fit(V, beta=2, tol=-1e9, max_iter=200, **kw))
    mu_loss = loss([f.data for f in m.factors])
    h = ntf.NTF(factors=start).cuda()
    h.fit(V, beta=2, tol=-1e9, max_iter=1, solver='hals', precision=precision, **kw)      # warm-up
    h = ntf.NTF(factors=start).cuda()
    fs = [f.data for f in h.factors]
    eng = ntf._HalsNtf(T, fs, (True, True, True), 0.0, 0.0, precision=precision)
    _, scale_ms = timed(eng._ensure_scaled)
    trace, iters, hals_ms = [loss(fs)], 0, scale_ms
    while trace[-1] > mu_loss and iters < 200:
        _, ms = timed(lambda: [eng.half_step(n) for n in range(3)])
        hals_ms += ms
        iters += 1
        trace.append(loss(fs))
    # the parts of one iteration, per mode: numerator, Gram x 2 + product, sweep
    parts = {'numerator': 0.0, 'gram': 0.0, 'sweep': 0.0}
    for n in range(3):
        pa, pb = (f for k, f in enumerate(fs) if k != n)
        parts['numerator'] += events(lambda: eng._numerator(n))
        parts['gram'] += events(lambda: ntf._gram(lib, pa) * ntf._gram(lib, pb))
        num, G, own = eng._numerator(n), ntf._gram(lib, pa) * ntf._gram(lib, pb), fs[n].clone()
        parts['sweep'] += events(lambda: _sweep(own, num, num.stride(0), G, 0.0, 0.0))
    tot = sum(parts.values())
    res = dict(case=name, precision=precision, shape=shape, rank=R, mu_200_ms=mu_ms, mu_200_loss=mu_loss, hals_iterations=iters, hals_ms=hals_ms,
               hals_scale_ms=scale_ms, hals_loss=trace[-1], hals_trace=trace[:12], iteration_parts_ms=parts,
               gram_and_sweep_share=(parts['gram'] + parts['sweep']) / tot, hals_fit_loss_tracked=eng.divergence())
    print(json.dumps(res), flush=True)
    out.append(res)


def main():
    out = []
    g = torch.Generator(device='cuda').manual_seed(2)
    shape, R = (512, 512, 512), 64
    pf = [torch.rand(d, R, device='cuda', generator=g) for d in shape]
    V = torch.einsum('ir,jr,kr->ijk', *pf) * (0.9 + 0.2 * torch.rand(shape, device='cuda', generator=g))
    T = ntf.NtfTarget(V)
    for precision in ('fp32', 'bf16x3'):      # the loss is nmfmu_ntf_loss in either: float64 sums over the reconstruction
        run('dense', V, T, {}, lambda fs: float(ntf._ntf_loss(T, fs, 2.0).item()), shape, R, out, precision)
    del V, T
    shape, nnz = (65536, 16384, 24), 10_000_000
    idx = torch.stack([torch.randint(0, d, (nnz,), device='cuda', generator=g) for d in shape])
    pf = [torch.rand(d, 8, device='cuda', generator=g) for d in shape]
    vals = (pf[0][idx[0]] * pf[1][idx[1]] * pf[2][idx[2]]).sum(1) + 0.01
    Ts = ntf.SparseNtfTarget(torch.sparse_coo_tensor(idx, vals, shape))
    run('sparse_zero', Ts, Ts, {'unstored': 'zero'}, lambda fs: float(ntf._sparse_loss(Ts, fs, 2.0, 'zero').item()), shape, R, out)
    if len(sys.argv) > 1:      # python tools/bench_ntf_hals.py [OUT.json]
        json.dump(out, open(sys.argv[1], 'w'), indent=1)


main()
