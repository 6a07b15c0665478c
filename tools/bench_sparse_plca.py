#!/usr/bin/env python3
"""Time one EM iteration of ``PLCA.fit`` on a sparse-COO target (plca._SparsePlcaEM) beside the dense path on the densified
target and, for scale, the missing-data NMF iteration on the same pattern -- in one process, on the target of
tools/bench_masked.py:

    python tools/bench_sparse_plca.py [--out profiles/sparse_plca.json]

  sparse   _SparsePlcaEM.em_step: nmfmu_sp_plca_estep + nmfmu_sp_plca_gather (plus the finishing kernel of the split rows) and
           the M-step kernels; the two E-step kernels and the M-step are also timed alone
  dense    _PlcaEM.em_step on V.to_dense() (65 536 x 16 384 fp32 and its packed images), default precision
  masked   sparse_engine.MaskedMU at beta = 1: w_step + h_step on the same pattern (another model: for scale only)

Fixed inputs: 65 536 x 16 384, 10 M stored entries whose row and column degrees follow a power law, rank 64; values uniform in
[0.1, 1.1), factors uniform in [0.05, 1.05) and normalised as PLCA normalises them.  Device events, 2 warm-up iterations, then the
median of 10 with min - max; the paths alternate.

Bytes, by this tool's count: the E-step reads index + value (8 B), writes g (4 B) and reads ONE panel row (4 R B) per stored
entry -- the row feeds the dot product and the accumulator from registers -- and reads its owner row and writes its numerator row
(8 R B per row of V); the gather reads index + perm + g (12 B) and one panel row per stored entry and writes a numerator row
(4 R B per column of V).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_masked import C, N, NNZ, R, REPEATS, WARMUP, degree_stats, make_target, summary, timed  # noqa: E402
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.metrics import SparseTarget  # noqa: E402
from torchnmf_amd.plca import _PlcaEM, _SparsePlcaEM  # noqa: E402
from torchnmf_amd.sparse_engine import MaskedMU  # noqa: E402


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_plca.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _capi.load()
    V = make_target(dev)
    T = SparseTarget(V)
    norm = T.vals.sum()
    vals_n = T.vals / norm
    g = torch.Generator(device=dev).manual_seed(1)
    H0 = torch.rand(N, R, generator=g, device=dev) + 0.05
    W0 = torch.rand(C, R, generator=g, device=dev) + 0.05
    Z0 = torch.rand(R, generator=g, device=dev) + 0.05
    H0, W0, Z0 = H0 / H0.sum(0), W0 / W0.sum(0), Z0 / Z0.sum()
    estep_bytes = NNZ * (12 + 4 * R) + N * R * 8
    gather_bytes = NNZ * (12 + 4 * R) + C * R * 4
    res = dict(tool='tools/bench_sparse_plca.py', device=torch.cuda.get_device_name(0), shape=[N, C], nnz=NNZ, rank=R,
               warmup=WARMUP, repeats=REPEATS, chunk=T.chunk, degrees=degree_stats(T),
               segments=dict(h=T.seg_h.shape[0], w=T.seg_w.shape[0]), split_rows=dict(h=T.multi_h.shape[0], w=T.multi_w.shape[0]),
               estep_bytes=estep_bytes, gather_bytes=gather_bytes)
    train = (True, True, True, 1.0, 1.0, 1.0)
    # one iteration from the same factors on both paths
    Ws, Hs, Zs = W0.clone(), H0.clone(), Z0.clone()
    es = _SparsePlcaEM(T, vals_n, Ws, Hs, Zs)
    Wd, Hd, Zd = W0.clone(), H0.clone(), Z0.clone()
    ed = _PlcaEM((V.to_dense() / norm).contiguous(), Wd, Hd, Zd, None)
    res['dense_precision'] = ed.precision_name
    loss0 = dict(sparse=es.divergence(), dense=ed.divergence())
    es.em_step(*train)
    ed.em_step(*train)
    res['one_iteration_rel_diff_sparse_vs_dense'] = dict(W=rel(Ws, Wd), H=rel(Hs, Hd), Z=rel(Zs, Zd))
    res['loss_initial'] = loss0
    res['loss_after_one'] = dict(sparse=es.divergence(), dense=ed.divergence())
    # for scale: the missing-data NMF iteration on the same pattern
    Hm, Wm = torch.rand(N, R, generator=g, device=dev) + 0.05, torch.rand(C, R, generator=g, device=dev) + 0.05
    em = MaskedMU(T, Wm, Hm, 1.0)

    def sparse():
        es.em_step(*train)

    def dense():
        ed.em_step(*train)

    def masked():
        em.w_step()
        em.h_step()

    # the parts of the sparse iteration alone (the factors stand still: the work does not depend on the values)
    es.z_old[:R].copy_(es.Z)
    lib, st = es.lib, es._s
    seg_h, multi_h, nm_h, colidx = es._lists('h')
    seg_w, multi_w, nm_w, rowidx = es._lists('w')

    def estep():
        _capi.check(lib.nmfmu_sp_plca_estep(seg_h.data_ptr(), seg_h.shape[0], multi_h, nm_h, colidx, es.vals_n.data_ptr(),
                                            es.H.data_ptr(), es.z_old.data_ptr(), es.W.data_ptr(), R, es.g.data_ptr(),
                                            es.ws_h.data_ptr(), es.num_h.data_ptr(), es.r_pad, st()), 'nmfmu_sp_plca_estep')

    def gather():
        _capi.check(lib.nmfmu_sp_plca_gather(seg_w.data_ptr(), seg_w.shape[0], multi_w, nm_w, rowidx, T.perm.data_ptr(),
                                             es.g.data_ptr(), es.H.data_ptr(), R, es.ws_w.data_ptr(), es.num_w.data_ptr(),
                                             es.r_pad, st()), 'nmfmu_sp_plca_gather')
    Wk, Hk, Zk = es.W.clone(), es.H.clone(), es.Z.clone()

    def m_step():
        es._m_step((es.num_w, 1, C), (es.num_h, 1, N), es.z_old, *train)
    ts, td, tm = timed([sparse, dense, masked])
    te, tg = timed([estep, gather])
    tms, = timed([m_step])
    for dst, src in ((es.W, Wk), (es.H, Hk), (es.Z, Zk)):
        dst.copy_(src)
    med = statistics.median
    res.update(sparse=summary(ts), dense=summary(td), masked_nmf_beta1=summary(tm), estep=summary(te), gather=summary(tg),
               m_step=summary(tms), dense_over_sparse=med(td) / med(ts), sparse_over_masked_nmf=med(ts) / med(tm),
               estep_tb_per_s=estep_bytes / med(te) / 1e9, gather_tb_per_s=gather_bytes / med(tg) / 1e9,
               bounding_kernel='estep' if med(te) >= med(tg) else 'gather')
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
