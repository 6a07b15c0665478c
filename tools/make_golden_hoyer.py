#!/usr/bin/env python3
"""Generate the Hoyer fixtures under tests/golden/ by RUNNING the reference (torchnmf 0.3.5), like tools/make_golden.py:
the reference is imported (from the directory NMF_REFERENCE names, else as installed), fed seeded inputs through its public entry points, and
only inputs and outputs are stored as plain arrays.

    NMF_REFERENCE=<checkout of pytorch-NMF> python tools/make_golden_hoyer.py       # rewrites g15 / g16 / g17 and tests/golden/PROVENANCE_hoyer.txt

  g15_hoyer_proj     the projection itself (nmf.py:21-49) on s = |randn|, k1 = (sqrt(n)(1 - sigma) + sigma) |s|, k2 = |s|^2 (both
                     rounded to fp32, so that every implementation sees the same targets), sigma in {0.2, 0.4, 0.8} x
                     n in {2, 3, 63, 64, 65, 255, 257, 1000, 5000}: the fp32 result and, per case, the reference's own fp32
                     error against a float64 run of the same function (e_ref, relative Frobenius; a case with
                     e_ref = 0 is refused)
  g16_sparsity_proj  trainer.SparsityProj (sparsity 0.3, beta = 2) on W and on H of an NMF 64 x 96 rank 8: the factors after
                     steps 1 and 10, lr after every step
  g17_sparse_fit     sparse_fit, 20 iterations, (sW, sH) in {(0.4, None), (None, 0.4), (0.3, 0.3)}: NMF 64 x 96 r8 at beta = 2
                     and 1, NMFD (1, 33, 50) r4 T = 3 and NMF2D (1, 6, 20, 18) r3 kernel (3, 2) at beta = 2: initial and final
                     factors, returned count

Every end-to-end case (g16, g17) is SCREENED and refused when it fails: the reference runs in fp32 and in fp64 from the same
initial factors; the two runs must make the same number of loss evaluations (SparsityProj: the same lr sequence too) and end
within 1e-5 (relative Frobenius) on both factors.  This is a condition on the fixture, not a tolerance of any test: it keeps
a line-search decision that sits on a rounding error out of the fixtures.
"""
import copy
import os
import sys

import numpy as np
import torch

if os.environ.get('NMF_REFERENCE'):
    sys.path.insert(0, os.environ['NMF_REFERENCE'])
import torchnmf  # noqa: E402
from torchnmf import nmf as ref_nmf  # noqa: E402
from torchnmf import trainer as ref_trainer  # noqa: E402
from torchnmf.metrics import beta_div as ref_beta_div  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
SCREEN = 1e-5

SIGMAS = (0.2, 0.4, 0.8)
SIZES = (2, 3, 63, 64, 65, 255, 257, 1000, 5000)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def g15_hoyer_proj():
    out = dict(sigma=[], n=[], k1=[], k2=[], e_ref=[])
    g = torch.Generator().manual_seed(15)
    for sigma in SIGMAS:
        for n in SIZES:
            i = len(out['n'])
            s = torch.randn(n, generator=g).abs()
            nrm = float(s.double().norm())
            k1 = float(np.float32((n ** 0.5 * (1 - sigma) + sigma) * nrm))
            k2 = float(np.float32(nrm * nrm))
            p32 = ref_nmf._proj_func(s.clone(), k1, k2)
            p64 = ref_nmf._proj_func(s.double().clone(), k1, k2)
            assert bool(((p32 == 0) == (p64 == 0)).all()), (sigma, n, 'fp32 and fp64 zero patterns differ')
            if rel(p32, p64) == 0:         # e_ref is the unit of the tests' bounds: a case that measures none cannot carry one
                raise SystemExit(f'g15 sigma {sigma} n {n}: refused, fp32 and fp64 runs agree to the last bit (e_ref = 0)')
            out[f's_{i}'] = s.numpy()
            out[f'p_{i}'] = p32.numpy()
            for k, v in (('sigma', sigma), ('n', n), ('k1', k1), ('k2', k2), ('e_ref', rel(p32, p64))):
                out[k].append(v)
    for k in ('sigma', 'k1', 'k2', 'e_ref'):
        out[k] = np.asarray(out[k], dtype=np.float64)
    out['n'] = np.asarray(out['n'], dtype=np.int64)
    print(f"g15: {len(out['n'])} cases, e_ref max {out['e_ref'].max():.2e} min {out['e_ref'].min():.2e}")
    return out


class _Count:
    """Counts the loss evaluations of sparse_fit: the reference's nmf module calls its global beta_div for every one."""

    def __enter__(self):
        self.n = 0
        self.orig = ref_nmf.beta_div

        def tap(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        ref_nmf.beta_div = tap
        return self

    def __exit__(self, *a):
        ref_nmf.beta_div = self.orig
        return False


def g16_sparsity_proj():
    out = {}
    torch.manual_seed(16)
    V = torch.rand(64, 96)
    W0, H0 = torch.randn(96, 8).abs(), torch.randn(64, 8).abs()
    out.update(V=V.numpy(), W0=W0.numpy(), H0=H0.numpy())
    for attr in ('W', 'H'):
        runs = []
        for dt in (torch.float32, torch.float64):
            m = ref_nmf.NMF(W=W0, H=H0).to(dt)
            Vd = V.to(dt)
            tr = ref_trainer.SparsityProj([getattr(m, attr)], 0.3)
            evals = [0]

            def closure():
                tr.zero_grad()
                evals[0] += 1
                return ref_beta_div(m(), Vd, 2)
            lrs, snaps = [], {}
            for step in range(1, 11):
                tr.step(closure)
                lrs.append(float(tr.param_groups[0]['lr']))
                if step in (1, 10):
                    snaps[step] = (m.W.detach().clone(), m.H.detach().clone())
            runs.append((lrs, evals[0], snaps))
        (lr32, ev32, s32), (lr64, ev64, s64) = runs
        errs = [rel(s32[10][k], s64[10][k]) for k in (0, 1)]
        if lr32 != lr64 or ev32 != ev64 or max(errs) > SCREEN:
            raise SystemExit(f'g16 {attr}: refused by the screen (lr {lr32} vs {lr64}, evaluations {ev32} vs {ev64}, '
                             f'fp32-fp64 {errs})')
        print(f'g16 {attr}: {ev32} evaluations, lr[-1] {lr32[-1]:.6g}, fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e}')
        out[f'{attr}_lr'] = np.asarray(lr32, dtype=np.float64)
        for step in (1, 10):
            out[f'{attr}_W{step}'] = s32[step][0].numpy()
            out[f'{attr}_H{step}'] = s32[step][1].numpy()
    return out


G17_MODELS = (('nmf', ref_nmf.NMF, (64, 96), dict(rank=8), (2, 1)),
              ('nmfd', ref_nmf.NMFD, (1, 33, 50), dict(rank=4, T=3), (2,)),
              ('nmf2d', ref_nmf.NMF2D, (1, 6, 20, 18), dict(rank=3, kernel_size=(3, 2)), (2,)))
G17_PAIRS = ((0.4, None), (None, 0.4), (0.3, 0.3))


def g17_sparse_fit():
    out, names = {}, []
    for tag, cls, shape, kw, betas in G17_MODELS:
        torch.manual_seed(0)
        V = torch.rand(*shape)
        m0 = cls(shape, **kw)
        out[f'{tag}_V'] = V.numpy()
        out[f'{tag}_W0'] = m0.W.detach().numpy().copy()
        out[f'{tag}_H0'] = m0.H.detach().numpy().copy()
        for beta in betas:
            for sW, sH in G17_PAIRS:
                res = []
                for dt in (torch.float32, torch.float64):
                    m = copy.deepcopy(m0).to(dt)
                    with _Count() as c:
                        n = m.sparse_fit(V.to(dt), beta=beta, max_iter=20, sW=sW, sH=sH)
                    res.append((m, n, c.n))
                (m32, n32, e32), (m64, n64, e64) = res
                errs = (rel(m32.W, m64.W), rel(m32.H, m64.H))
                name = f'{tag}_b{beta}_w{sW}_h{sH}'
                if e32 != e64 or n32 != n64 or max(errs) > SCREEN:
                    raise SystemExit(f'g17 {name}: refused by the screen (evaluations {e32} vs {e64}, fp32-fp64 {errs})')
                print(f'g17 {name}: n_iter {n32}, {e32} evaluations, fp32-fp64 W {errs[0]:.1e} H {errs[1]:.1e}')
                names.append(name)
                out[f'{name}_W'] = m32.W.detach().numpy().copy()
                out[f'{name}_H'] = m32.H.detach().numpy().copy()
                out[f'{name}_n'] = np.asarray(n32, dtype=np.int64)
    out['cases'] = np.asarray(names)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    for fn in (g15_hoyer_proj, g16_sparsity_proj, g17_sparse_fit):
        data = fn()
        path = os.path.join(OUT, fn.__name__ + '.npz')
        np.savez_compressed(path, **data)
        print('wrote', os.path.relpath(path), os.path.getsize(path), 'bytes')
    with open(os.path.join(OUT, 'PROVENANCE_hoyer.txt'), 'w') as f:
        f.write(f'g15_hoyer_proj g16_sparsity_proj g17_sparse_fit: generated by `python tools/make_golden_hoyer.py'
                f'{"".join(" " + a for a in sys.argv[1:])}` from torchnmf {torchnmf.__version__} (the reference, imported), '
                f'torch {torch.__version__}, CPU, 1 thread; fp32 results, every g16 / g17 case screened against an fp64 run of the '
                f'reference from the same initial factors (same number of loss evaluations, same lr sequence, final factors '
                f'within {SCREEN:g})\n')
