"""Bit-compare two builds of the library on everything the exact-fp32 tile kernels compute (a refactor of nmfmu_wmu.hip,
nmfmu_bmu.hip, nmfmu_ntf.hip and nmfmu_wmu_tile.h against its parent), in two fresh processes:
    NMFMU_LIB=.../parent/libnmfmu.so python tools/tile_bitcompare.py --save /tmp/ref.pt
    python tools/tile_bitcompare.py --compare /tmp/ref.pt
Seeded inputs on the 2^-10 grid in (0, 1], factors rand + 0.05.  Recorded per case: the terms (num, den), the stepped owner and
the loss (double), each as (shape, SHA-256 of its raw bytes) -- the cases are many and small.

  dense   nmfmu_wmu_*, nmfmu_bmu_* and nmfmu_bwmu_* (B = 3, active = [1, 0, 1], m_index = [1, 0, 1] over two weight matrices,
          the per-problem `reg` step) on both sides: n in {1, 127, 129} (row-tile edge) x c in {31, 33, 161} (a short stage, a
          stage boundary, a last part shorter than the others) x ld in {c, c + 3} (scalar loads; 16-byte loads where ld % 4 == 0)
          x rank in {3, 33, 100, 200} (every WmuCfg) x beta in {0, 0.5, 1, 2} (every KIND) x nsplit in {0, 1, 3}.  The weights
          hold exact zeros with NaN in V under them; the unweighted batch reads the same V without the NaNs.
  NTF     (I, J, K) in {(3, 7, 5), (130, 6, 9)} (quads across slice boundaries and at unaligned offsets) x mode in {0, 1, 2} x
          M in {NULL, given} x rank in {3, 100} x beta in {1, 0.5}, nsplit 0; and one forced split into 12 parts of mode 0 of a
          (2, 24, 16) tensor: the finish kernel's 8-at-a-time loop runs its unrolled trip and its tail.
Exit status 1 when any tensor differs.  A mismatch names the case; `--case TEXT --dump FILE` (under either library) runs again
and saves the raw tensors of every case whose name holds TEXT, for an element-wise look."""
import argparse
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
import torch

from torchnmf_amd import _capi
from torchnmf_amd.engine import mu_gamma

B = 3
NS, CS, RANKS, BETAS, NSPLITS = (1, 127, 129), (31, 33, 161), (3, 33, 100, 200), (0.0, 0.5, 1.0, 2.0), (0, 1, 3)
L1, L2 = 0.01, 0.02
REG = [[0.01, 0.0], [0.0, 0.02], [0.03, 0.01]]
NTF_SHAPES, NTF_RANKS, NTF_BETAS = ((3, 7, 5), (130, 6, 9)), (3, 100), (1.0, 0.5)
NTF_SPLIT_SHAPE, NTF_SPLIT_PARTS = (2, 24, 16), 12


def grid(shape, g):
    return (torch.floor(torch.rand(shape, generator=g) * 1024) + 1) / 1024


def digest(x):
    return x.detach().cpu().contiguous()


class Record(dict):
    """name -> (shape, SHA-256 of the raw bytes); the raw tensors of the names that hold `case` beside them"""

    def __init__(self, case=None):
        super().__init__()
        self.case, self.raw = case, {}

    def __setitem__(self, key, x):
        if self.case and self.case in key:
            self.raw[key] = x.clone()
        super().__setitem__(key, (tuple(x.shape), hashlib.sha256(x.numpy().tobytes()).hexdigest()))


def ptr(t):
    return None if t is None else t.data_ptr()


def run(dev, case=None):
    lib, out = _capi.load(), Record(case)
    stream = torch.cuda.current_stream().cuda_stream
    f32 = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)

    def ok(rc, what):
        _capi.check(rc, what)

    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    m_index = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    reg = torch.tensor(REG, **f32)
    for n, c, pad in itertools.product(NS, CS, (0, 3)):
        ld = c + pad
        g = torch.Generator().manual_seed(1000 * n + 10 * c + pad)
        Vb, Mb = torch.zeros(B, n, ld), torch.zeros(2, n, ld)
        Vb[:, :, :c] = grid((B, n, c), g)
        Mb[:, :, :c] = grid((2, n, c), g) * 4 * (torch.rand(2, n, c, generator=g) > 0.3)
        Vn = Vb.clone()                                   # NaN wherever a problem's weights are zero
        for b in range(B):
            Vn[b][Mb[int(m_index[b])] == 0] = float('nan')
        Vb, Vn, Mb = Vb.to(dev), Vn.to(dev), Mb.to(dev)
        vstride = mstride = n * ld
        for R in RANKS:
            r_pad = lib.nmfmu_pad_rank(R)
            H0, W0 = (torch.rand(B, n, R, generator=g) + 0.05).to(dev), (torch.rand(B, c, R, generator=g) + 0.05).to(dev)
            for beta in BETAS:
                gamma = mu_gamma(beta)
                key = f'n{n} c{c} ld{ld} R{R} beta{beta:g}'
                # losses: one problem against its weights; the batch, unweighted and weighted
                part = torch.zeros(lib.nmfmu_wmu_loss_parts(n, c), **f64)
                res = torch.zeros(1, **f64)
                ok(lib.nmfmu_wmu_loss(Vn[0].data_ptr(), Mb[1].data_ptr(), ld, n, c, H0[0].data_ptr(), W0[0].data_ptr(), R, beta,
                                      0.25, part.data_ptr(), res.data_ptr(), stream), 'nmfmu_wmu_loss')
                out[f'wmu {key} loss'] = digest(res)
                for name, V, M in (('bmu', Vb, None), ('bwmu', Vn, Mb)):
                    vt, res = torch.zeros(B, **f64), torch.zeros(B, **f64)
                    part = torch.zeros(B * lib.nmfmu_bmu_loss_parts(n, c), **f64)
                    ok(lib.nmfmu_bwmu_v_term(V.data_ptr(), vstride, ptr(M), mstride, ptr(M) and m_index.data_ptr(), ld, B, n, c,
                                             beta, vt.data_ptr(), stream), 'nmfmu_bwmu_v_term')
                    ok(lib.nmfmu_bwmu_loss(V.data_ptr(), vstride, ptr(M), mstride, ptr(M) and m_index.data_ptr(), ld, B, n, c,
                                           H0.data_ptr(), W0.data_ptr(), R, beta, vt.data_ptr(), active.data_ptr(),
                                           part.data_ptr(), res.data_ptr(), stream), f'nmfmu_{name}_loss')
                    out[f'{name} {key} v_term'], out[f'{name} {key} loss'] = digest(vt), digest(res)
                for nsplit, side in itertools.product(NSPLITS, (0, 1)):
                    rows, contraction = (c, n) if side else (n, c)
                    own0, pan = (W0, H0) if side else (H0, W0)
                    k2 = f'{key} nsplit{nsplit} side{side}'
                    ws = torch.zeros(lib.nmfmu_bmu_ws(B, rows, contraction, r_pad, nsplit), **f32)
                    # one problem
                    num, den, own = torch.zeros(rows, r_pad, **f32), torch.zeros(rows, r_pad, **f32), own0[0].clone()
                    ok(lib.nmfmu_wmu_terms(Vn[0].data_ptr(), Mb[1].data_ptr(), ld, n, c, side, own.data_ptr(), pan[0].data_ptr(), R,
                                           r_pad, beta, nsplit, ws.data_ptr(), num.data_ptr(), den.data_ptr(), stream),
                       'nmfmu_wmu_terms')
                    ok(lib.nmfmu_wmu_step(Vn[0].data_ptr(), Mb[1].data_ptr(), ld, n, c, side, own.data_ptr(), pan[0].data_ptr(), R,
                                          r_pad, beta, L1, L2, gamma, nsplit, ws.data_ptr(), stream), 'nmfmu_wmu_step')
                    out[f'wmu {k2} num'], out[f'wmu {k2} den'], out[f'wmu {k2} step'] = digest(num), digest(den), digest(own)
                    # the batch: unweighted, weighted, weighted with per-problem (l1, l2)
                    for name, V, M, rg in (('bmu', Vb, None, None), ('bwmu', Vn, Mb, None), ('bwmu_reg', Vn, Mb, reg)):
                        mi = ptr(M) and m_index.data_ptr()
                        num, den, own = torch.zeros(B, rows, r_pad, **f32), torch.zeros(B, rows, r_pad, **f32), own0.clone()
                        if rg is None:
                            ok(lib.nmfmu_bwmu_terms(V.data_ptr(), vstride, ptr(M), mstride, mi, ld, B, n, c, side, own.data_ptr(),
                                                    pan.data_ptr(), R, r_pad, beta, nsplit, active.data_ptr(), ws.data_ptr(),
                                                    num.data_ptr(), den.data_ptr(), stream), f'nmfmu_{name}_terms')
                            out[f'{name} {k2} num'], out[f'{name} {k2} den'] = digest(num), digest(den)
                        ok(lib.nmfmu_bwmu_step(V.data_ptr(), vstride, ptr(M), mstride, mi, ld, B, n, c, side, own.data_ptr(),
                                               pan.data_ptr(), R, r_pad, beta, L1, L2, ptr(rg), gamma, nsplit, active.data_ptr(),
                                               ws.data_ptr(), stream), f'nmfmu_{name}_step')
                        out[f'{name} {k2} step'] = digest(own)
    # NTF
    cases = [(s, mode, wt, R, beta, 0) for s in NTF_SHAPES for mode in range(3) for wt in (False, True) for R in NTF_RANKS
             for beta in NTF_BETAS]
    cases += [(NTF_SPLIT_SHAPE, 0, wt, 3, 1.0, NTF_SPLIT_PARTS) for wt in (False, True)]
    for shape, mode, weighted, R, beta, nsplit in cases:
        I, J, K = shape
        g = torch.Generator().manual_seed(7000 + 100 * I + 10 * mode + R)
        V = grid(shape, g)
        M = (grid(shape, g) * 4 * (torch.rand(shape, generator=g) > 0.3)) if weighted else None
        if weighted:
            V[M == 0] = float('nan')
        V, M = V.to(dev), None if M is None else M.to(dev)
        fs = [(torch.rand(d, R, generator=g) + 0.05).to(dev) for d in shape]
        r_pad, rows, contraction = lib.nmfmu_pad_rank(R), shape[mode], I * J * K // shape[mode]
        pa, pb = (f for m, f in enumerate(fs) if m != mode)
        key = f'ntf {I}x{J}x{K} mode{mode} M{int(weighted)} R{R} beta{beta:g} nsplit{nsplit}'
        ws = torch.zeros(lib.nmfmu_ntf_ws(rows, contraction, r_pad, nsplit), **f32)
        if nsplit:
            assert lib.nmfmu_ntf_ws(rows, contraction, r_pad, nsplit) == nsplit * 2 * rows * r_pad, 'the forced split'
        num, den, own = torch.zeros(rows, r_pad, **f32), torch.zeros(rows, r_pad, **f32), fs[mode].clone()
        ok(lib.nmfmu_ntf_terms(V.data_ptr(), ptr(M), I, J, K, mode, own.data_ptr(), pa.data_ptr(), pb.data_ptr(), R, r_pad, beta,
                               nsplit, ws.data_ptr(), num.data_ptr(), den.data_ptr(), stream), 'nmfmu_ntf_terms')
        ok(lib.nmfmu_ntf_step(V.data_ptr(), ptr(M), I, J, K, mode, own.data_ptr(), pa.data_ptr(), pb.data_ptr(), R, r_pad, beta,
                              L1, L2, mu_gamma(beta), nsplit, ws.data_ptr(), stream), 'nmfmu_ntf_step')
        out[f'{key} num'], out[f'{key} den'], out[f'{key} step'] = digest(num), digest(den), digest(own)
        if mode == 0 and not nsplit:
            part, res = torch.zeros(lib.nmfmu_ntf_loss_parts(I, J, K), **f64), torch.zeros(1, **f64)
            ok(lib.nmfmu_ntf_loss(V.data_ptr(), ptr(M), I, J, K, fs[0].data_ptr(), fs[1].data_ptr(), fs[2].data_ptr(), R, beta,
                                  0.25, part.data_ptr(), res.data_ptr(), stream), 'nmfmu_ntf_loss')
            out[f'{key} loss'] = digest(res)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--save')
    ap.add_argument('--compare')
    ap.add_argument('--case')
    ap.add_argument('--dump')
    a = ap.parse_args()
    out = run(torch.device('cuda', 0), a.case)
    print(f'{len(out)} tensors from {_capi.LIB_PATH}')
    if a.dump:
        torch.save(out.raw, a.dump)
        print(f'{len(out.raw)} raw tensors to {a.dump}')
    if a.save:
        torch.save(dict(out), a.save)
    if a.compare:
        ref = torch.load(a.compare)
        assert set(ref) == set(out), sorted(set(ref) ^ set(out))
        bad = [k for k in out if out[k] != ref[k]]
        for k in bad:
            print(f'DIFFERS: {k}')
        print(f'{len(out) - len(bad)} of {len(out)} tensors bit-identical')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
