#!/usr/bin/env python3
"""Time one ARD-NMF iteration (``NMF.fit_ard``'s engine, ``ard.ArdMU``: two partial-sum launches, two ``nmfmu_ard_apply`` and one
``nmfmu_ard_relevance``) beside one iteration of the plain fit's engine (``engine.DenseMU`` as ``NMF._make_engine`` builds it:
the apply fused into the kernel's epilogue where the contraction is not split) on the same target in the same precision mode:

    python tools/bench_ard.py [--out profiles/ard.json]

4096 x 65536, ranks 64 and 128, beta in {1, 0.5}, precision 'auto' (what it resolves to is recorded; the ARD arm is given the
same mode by name).  Device events around blocks of ITERS iterations after a warm-up block, three repeats with the arms
alternating, median of the three.  The apply stage is timed where it runs: events around both half-steps' ``nmfmu_ard_apply``
calls (kernel + finalize) inside ITERS real iterations, summed per iteration, median of three such blocks;
``apply_hbm_fraction`` is the bytes it must move -- every slab once, the master in and out, the written image planes -- over
that time, against 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-nmf_amd'))

N, C = 4096, 65536
RANKS = (64, 128)
BETAS = (1.0, 0.5)
ITERS, REPEATS = 10, 3
HBM_PEAK = 8.0e12


def block_ms(step, iters=ITERS):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def apply_bytes(st, precision, kl, writes_p2):
    plane = st.owner.rows_pad * st.r_pad
    slabs = st.nsplit * plane * 4 * (1 if kl else 2)
    master = 2 * st.owner.rows * st.owner.rank * 4
    planes = (2 if precision == 'bf16x3' else 1) * (2 if writes_p2 else 1)
    return slabs + master + planes * plane * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ard.json'))
    a = ap.parse_args()
    import torch
    from torchnmf_amd import _capi
    from torchnmf_amd.ard import ArdMU, default_b
    from torchnmf_amd.engine import DenseMU
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(3)
    V = torch.rand(N, C, generator=g, device=dev) + 0.1
    v_mean = float(V.mean())
    res = dict(tool='tools/bench_ard.py', device=torch.cuda.get_device_name(0), shape=[N, C], iters_per_block=ITERS, repeats=REPEATS,
               hbm_peak=HBM_PEAK, rows=[])
    for R in RANKS:
        for beta in BETAS:
            gf = torch.Generator(device=dev).manual_seed(1)
            W0, H0 = torch.rand(C, R, generator=gf, device=dev) + 0.05, torch.rand(N, R, generator=gf, device=dev) + 0.05
            plain = DenseMU(V, W0.clone(), H0.clone(), beta, precision='auto', allow_f16=True, allow_gram=True)
            mode = plain.precision_name
            ard = ArdMU(V, W0.clone(), H0.clone(), beta, 'l1', 1.0, 5.0, default_b(v_mean, R, 5.0, 'l1'), mode)

            def plain_step():
                plain.w_step()
                plain.h_step()

            def ard_step():
                ard.w_step()
                ard.h_step()
                ard.relevance_step()

            def apply_pair_ms():
                """The two apply launches (each with its finalize) of ITERS real iterations, bracketed where they run: behind
                their partial-sum kernels, on the factors of a fit in progress."""
                e, evs = ard.eng, []
                for _ in range(ITERS):
                    for st, other, norm, tag in ((e.step_w, e.fH, ard.norm_w, 'w'), (e.step_h, e.fW, ard.norm_h, 'h')):
                        e._partial(st, tag)
                        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a0.record()
                        ard.be.ard_apply(st, other.colsum if e.kl else None, ard.pen, 'l1', None, norm)
                        a1.record()
                        evs.append((a0, a1))
                    ard.relevance_step()
                torch.cuda.synchronize()
                return sum(a0.elapsed_time(a1) for a0, a1 in evs) / ITERS
            block_ms(plain_step), block_ms(ard_step)          # warm-up
            t = {'plain': [], 'ard': []}
            for _ in range(REPEATS):                          # arms alternating
                t['plain'].append(block_ms(plain_step))
                t['ard'].append(block_ms(ard_step))
            t_apply = statistics.median(apply_pair_ms() for _ in range(REPEATS))
            e = ard.eng
            one_image = e.step_w.struct.stage in (_capi.STAGE_DMA_LDSTR, _capi.STAGE_DMA_SP128, _capi.STAGE_DMA_SP128_RB0)
            nbytes = sum(apply_bytes(st, mode, e.kl, not one_image) for st in (e.step_w, e.step_h))
            row = dict(rank=R, beta=beta, precision=mode, stage=int(e.step_w.struct.stage), nsplit=[e.step_w.nsplit, e.step_h.nsplit],
                       block_rows=[e.step_w.block_rows, e.step_h.block_rows],
                       plain_ms=statistics.median(t['plain']), ard_ms=statistics.median(t['ard']), plain_all=t['plain'], ard_all=t['ard'],
                       apply_pair_ms=t_apply, apply_bytes=nbytes, apply_hbm_fraction=nbytes / (t_apply * 1e-3) / HBM_PEAK)
            row['ratio'] = row['ard_ms'] / row['plain_ms']
            res['rows'].append(row)
            print(json.dumps(row), flush=True)
            del plain, ard
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
