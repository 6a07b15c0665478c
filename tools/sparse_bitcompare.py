"""Bit-compare two builds of the library on everything the sparse kernels compute (a refactor of nmfmu_sparse*.hip against
its parent), in two fresh processes:
    NMFMU_LIB=.../parent/libnmfmu.so python tools/sparse_bitcompare.py --save /tmp/ref.pt
    python tools/sparse_bitcompare.py --compare /tmp/ref.pt
Target: seeded 48 x 301, values on the 2^-10 grid in (0, 1]; rows 0 .. 10 hold 0, 1, 3, 4, 5, 63, 64, 65, 67, 130 and 300
entries (group tails, the 64-entry block edge, rows that split), the other rows a tenth of the columns; column 7 is empty and
column 11 has one entry.  (The longest row stores every column but the empty one: a row of 301 would leave no column empty.)
Factors rand + 0.05; ranks 3, 33, 100, 200 (RL 1, 1, 2, 4); chunks 8, 64, 512 for the segment kernels.  Compared on raw bits:
  SparseMU            beta 0.5, 1, 2      W, H and divergence() after one w_step + h_step
  sparse_beta_div     beta 1, 2           value, grad_H, grad_W
  missing data        beta 0, 0.5, 1, 2   nmfmu_sp_masked_terms (num, den), nmfmu_sp_masked_step (owner) of both sides and
                                          nmfmu_sp_masked_loss
Exit status 1 when any tensor differs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-nmf_amd')):
    sys.path.insert(0, p)
import numpy as np
import torch

from torchnmf_amd import sparse_autograd as SA
from torchnmf_amd.engine import mu_gamma
from torchnmf_amd.sparse_engine import SparseMU

N, C = 48, 301
ROW_LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 67, 130, 300]
EMPTY_COL, ONE_ENTRY_COL = 7, 11
RANKS = [3, 33, 100, 200]
CHUNKS = [8, 64, 512]


def target():
    g = np.random.default_rng(20)
    free = np.setdiff1d(np.arange(C), [EMPTY_COL, ONE_ENTRY_COL])
    mask = np.zeros((N, C), dtype=bool)
    for row in range(N):
        n = ROW_LENGTHS[row] if row < len(ROW_LENGTHS) else None
        if n == 300:
            mask[row] = True
        elif n is not None:
            mask[row, g.choice(free, size=n, replace=False)] = True
        else:
            mask[row, free] = g.random(len(free)) < 0.1
    mask[:, EMPTY_COL] = False
    rc, cc = mask.sum(1), mask.sum(0)
    assert list(rc[:len(ROW_LENGTHS)]) == ROW_LENGTHS and cc[EMPTY_COL] == 0 and cc[ONE_ENTRY_COL] == 1
    idx = np.stack(np.nonzero(mask)).astype(np.int64)
    vals = ((np.floor(g.random(idx.shape[1]) * 1024) + 1) / 1024).astype(np.float32)
    return torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), (N, C))


def bits(x):
    if not isinstance(x, torch.Tensor):
        x = torch.tensor([x], dtype=torch.float64)
    x = x.detach().cpu().contiguous()
    return x.view(torch.int64 if x.dtype == torch.float64 else torch.int32).clone()


def run(dev):
    out = {}
    V = target().to(dev).coalesce()
    targets = {chunk: SA.SparseTarget(V, chunk=chunk) for chunk in CHUNKS}
    for R in RANKS:
        g = torch.Generator().manual_seed(100 + R)
        H0, W0 = torch.rand(N, R, generator=g) + 0.05, torch.rand(C, R, generator=g) + 0.05
        for beta in (0.5, 1.0, 2.0):
            W, H = W0.clone().to(dev), H0.clone().to(dev)
            eng = SparseMU(V, W, H, beta)
            eng.w_step()
            eng.h_step()
            torch.cuda.synchronize()
            key = f'SparseMU R{R} beta{beta:g}'
            out[key + ' W'], out[key + ' H'], out[key + ' divergence'] = bits(W), bits(H), bits(eng.divergence())
        for chunk, T in targets.items():
            for beta in (1.0, 2.0):
                H, W = H0.to(dev).requires_grad_(), W0.to(dev).requires_grad_()
                loss = SA.sparse_beta_div(H, W, T, beta)
                loss.backward()
                key = f'sparse_beta_div R{R} chunk{chunk} beta{beta:g}'
                out[key + ' value'], out[key + ' grad_H'], out[key + ' grad_W'] = bits(loss), bits(H.grad), bits(W.grad)
            for beta in (0.0, 0.5, 1.0, 2.0):
                Hc, Wc = H0.to(dev), W0.to(dev)
                key = f'masked R{R} chunk{chunk} beta{beta:g}'
                out[key + ' loss'] = bits(SA._masked_loss(Hc, Wc, T, beta))
                for side, owner, panel in (('h', Hc, Wc), ('w', Wc, Hc)):
                    num, den = SA._masked_call(T, side, owner, panel, beta)
                    out[f'{key} {side} num'], out[f'{key} {side} den'] = bits(num), bits(den)
                    stepped = owner.clone()
                    SA._masked_call(T, side, stepped, panel, beta, step=(0.0, 0.0, mu_gamma(beta)))
                    out[f'{key} {side} step'] = bits(stepped)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--save')
    ap.add_argument('--compare')
    a = ap.parse_args()
    out = run(torch.device('cuda', 0))
    print(f'{len(out)} tensors from {SA._capi.LIB_PATH}')
    if a.save:
        torch.save(out, a.save)
    if a.compare:
        ref = torch.load(a.compare)
        assert set(ref) == set(out), sorted(set(ref) ^ set(out))
        bad = [k for k in out if out[k].shape != ref[k].shape or not torch.equal(out[k], ref[k])]
        for k in bad:
            print(f'DIFFERS: {k}: {int((out[k] != ref[k]).sum())} of {out[k].numel()} elements')
        print(f'{len(out) - len(bad)} of {len(out)} tensors bit-identical')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
