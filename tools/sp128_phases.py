"""Per-phase cycles of the rank-128 software-pipelined MU kernel (csrc/nmfmu_sp128.h) from a diagnostic build:

    make -C pytorch-nmf_amd/csrc VARIANT=_ph0 EXTRA="-DNMFMU_SP128_PHASE_STAMPS -DNMFMU_SP128_RB=0" VUNITS=nmfmu_inst_sp128
    NMFMU_LIB=pytorch-nmf_amd/torchnmf_amd/libnmfmu_ph0.so python tools/sp128_phases.py [--rows 4096 --cols 65536 --rank 128]

Wave 0 of workgroup 0 sums the shader clock (s_memtime) over its phases A (GEMM1 of the next tile + what the build leaves of
the ratio stage) and B (GEMM2 + the loads + the moved reciprocals) separately and leaves the sums behind the product stamps
(nmfmu_step.stamps: words 16 = phase A cycles over nt - 1 phases, 17 = phase B cycles over nt phases -- the last tile's
un-hidden ratio stage counts as phase B --, 18 = nt).  Every boundary drains the LDS counter for its clock read, so the
build shows how a tile's cycles split between the phases, not what the product loop costs: the loop's own cycles per tile
(product stamps, words 0 and 4) are printed next to the sum for that reason.  32 MFMAs per phase and SIMD = 1 024 cycles.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))
from torchnmf_amd import _capi  # noqa: E402
from torchnmf_amd.engine import DenseMU  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=4096)
ap.add_argument('--cols', type=int, default=65536)
ap.add_argument('--rank', type=int, default=128)
ap.add_argument('--iters', type=int, default=12)
ap.add_argument('--repeats', type=int, default=5)
a = ap.parse_args()
dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(5)
V = torch.rand(a.rows, a.cols, device=dev, generator=g).half().float()
W = torch.rand(a.cols, a.rank, device=dev, generator=g) + 0.1
H = torch.rand(a.rows, a.rank, device=dev, generator=g) + 0.1
eng = DenseMU(V, W, H, 1.0, precision='f16')
del V
print(f'library {_capi.LIB_PATH}')
for name, st, step in (('W', eng.step_w, eng.w_step), ('H', eng.step_h, eng.h_step)):
    if st.struct.stage not in (_capi.STAGE_DMA_SP128, _capi.STAGE_DMA_SP128_RB0):
        print(f'{name} half-step: stage {st.struct.stage}, not the rank-128 software-pipelined kernel')
        continue
    nwg = (st.owner.rows_pad // st.block_rows) * st.nsplit
    for _ in range(a.iters):
        eng.w_step(), eng.h_step()
    for rep in range(a.repeats):
        buf = torch.zeros(64 + 5 * nwg, dtype=torch.int64, device=dev)
        st.struct.stamps = buf.data_ptr()
        try:
            step()
            torch.cuda.synchronize()
        finally:
            st.struct.stamps = None
        v = buf[:64].cpu().tolist()
        nt, loop = v[2], v[4] - v[0]          # slot 0 = loop start, slot 1 = loop end: word 4 slot + 0 is the shader clock
        if not v[18]:
            print(f'{name} half-step: this library records no phase sums (build it with -DNMFMU_SP128_PHASE_STAMPS)')
            break
        pa, pb = v[16] / max(1, nt - 1), v[17] / nt
        print(f'{name} half-step run {rep}: {nt} tiles, phase A {pa:7.1f} cycles, phase B {pb:7.1f} cycles, '
              f'A + B {pa + pb:7.1f}; loop {loop / nt:7.1f} cycles per tile')
