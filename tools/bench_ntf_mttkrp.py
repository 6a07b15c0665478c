"""nmfmu_ntf_mttkrp per mode in both precisions (fp32, and bf16x3: nmfmu_ntf_mttkrp_x3) against nmfmu_ntf_terms at beta = 2 (same
shape, same tile), the three routes alternating, device events."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-nmf_amd')]
import torch  # noqa: E402
from torchnmf_amd import _capi, ntf  # noqa: E402

HBM = 8.0e12      # bytes / s, the MI355X's nominal HBM3E bandwidth
MFMA = {'fp32': 157.3e12, 'bf16x3': 2516.6e12 / 3}      # flop / s of the matrix pipes: 32x32x2f32, and 32x32x16 bf16 three times per product
REPS, WINDOWS = 50, 7


def smi():
    try:
        return subprocess.run(['rocm-smi', '--showclocks', '--showpower'], capture_output=True, text=True, timeout=30).stdout[-1500:]
    except Exception as e:      # noqa: BLE001
        return repr(e)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    lib = _capi.load()
    out = {'hbm_bytes_per_s': HBM, 'reps_per_window': REPS, 'windows': WINDOWS, 'smi_before': smi(), 'cases': []}
    for shape, R in (((512, 512, 512), 64), ((8, 1025, 8192), 32), ((24, 4096, 4096), 64), ((512, 512, 512), 256)):
        g = torch.Generator(device='cuda').manual_seed(1)
        V = torch.rand(shape, device='cuda', generator=g) + 0.1
        T = ntf._Dense(V)
        T.M = None
        fs = [torch.randn(d, R, device='cuda', generator=g).abs().contiguous() for d in shape]
        r_pad = lib.nmfmu_pad_rank(R)
        floor_ms = 4.0 * V.numel() / HBM * 1e3
        for mode in range(3):
            rows = shape[mode]
            c = V.numel() // rows
            auto = 'short' if lib.nmfmu_ntf_tile(rows, c, r_pad) == 1 else 'wide'
            for tile in ('wide', 'short'):
                if tile == 'short' and rows > 32 and shape != (512, 512, 512):
                    continue
                ws_m = torch.empty(max(1, lib.nmfmu_ntf_mttkrp_ws(rows, c, r_pad, 0, int(tile == 'short'))), device='cuda')
                ws_t = torch.empty(max(1, ntf._tile_entries(lib, tile, rows, c, r_pad)[0](rows, c, r_pad, 0)), device='cuda')
                num = torch.empty(rows, r_pad, device='cuda')
                new = lambda: ntf._mttkrp_call(T, fs, mode, tile=tile, _ws=ws_m, out=num)      # noqa: E731
                x3 = lambda: ntf._mttkrp_call(T, fs, mode, tile=tile, _ws=ws_m, out=num, precision='bf16x3')      # noqa: E731
                old = lambda: ntf._ntf_call(T, fs, mode, 2.0, _ws=ws_t, tile=tile)             # noqa: E731
                ref = old()[0]
                err = float(((new() - ref).abs() / ref.abs().clamp_min(1e-30)).max())
                err3 = float(((x3() - ref).abs() / ref.abs().clamp_min(1e-30)).max())
                for _ in range(3):
                    new(), x3(), old()
                torch.cuda.synchronize()
                tn, t3, to = [], [], []
                for _ in range(WINDOWS):
                    tn.append(window(new))
                    t3.append(window(x3))
                    to.append(window(old))
                tn.sort(), t3.sort(), to.sort()
                pad = -(-rows // (32 if tile == 'short' else 128)) * (32 if tile == 'short' else 128)
                mfma_ms = {k: 2.0 * pad * c * r_pad / v * 1e3 for k, v in MFMA.items()}      # padded rows and rank are multiplied too
                case = dict(shape=shape, rank=R, mode=mode, tile=tile, auto_tile=auto, mttkrp_ms=dict(median=tn[WINDOWS // 2], min=tn[0], max=tn[-1]),
                            mttkrp_x3_ms=dict(median=t3[WINDOWS // 2], min=t3[0], max=t3[-1]),
                            fused_terms_ms=dict(median=to[WINDOWS // 2], min=to[0], max=to[-1]), hbm_floor_ms=floor_ms,
                            mfma_floor_ms=mfma_ms, max_rel_diff_vs_terms_num=err, x3_max_rel_diff_vs_terms_num=err3)
                out['cases'].append(case)
                print(json.dumps(case), flush=True)
        del V, T
    out['smi_after'] = smi()
    if len(sys.argv) > 1:      # python tools/bench_ntf_mttkrp.py [OUT.json]: the whole result, clock readings included
        json.dump(out, open(sys.argv[1], 'w'), indent=1)


main()
