"""Host-side orchestration of NMFD (1-D convolutive NMF) on one MI355X.

Reference: ``NMFD.reconstruct`` = ``F.conv1d(H, W.flip(2), padding=T-1)`` (nmf.py:776-779) driven by the same
``fit`` loop (nmf.py:297-409).  With ``Wm = W.view(C, R*T)`` and the Toeplitz unfold
``Hu[(b,l)][(r,t)] = H[b][r][l-t]`` the reconstruction is ``Wm @ Hu.T`` and both conv-backward passes are GEMMs,
so one MU iteration is four NT GEMMs (C ABI ``nmfmu_gemm``) with fused epilogues plus small unfold / fold /
apply kernels:

    W half-step   Gn[c][(b,l)]   = ratio( Wm Hu^T , V )              GEMM + EPI_RATIO
                  num[c][(r,t)]  = Gn  HuT^T                         GEMM + EPI_F32   -> nmfmu_conv_apply_w
    H half-step   GnT[(b,l)][c]  = ratio( Hu Wm^T , V^T )            GEMM + EPI_RATIO (transposed problem)
                  Y[(r,t)][(b,l)] = WmT GnT^T                        GEMM + EPI_F32   -> nmfmu_conv_fold_apply_h

NMFD is not sharded across GPUs ("replicas only").
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from dataclasses import dataclass, fields
from typing import Optional

import torch

from . import _capi
from .engine import AsyncLossMixin, _ptr, mu_gamma


def _pad128(n: int) -> int:
    return (n + 127) // 128 * 128


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _i32(vals):
    return (C.c_int32 * len(vals))(*vals)


class _Planes:
    """bf16 (hi[, lo]) planes of a zero-padded row-major matrix."""

    def __init__(self, rows_pad, cols_pad, x3, dev, zero=False):
        self.rows_pad, self.cols_pad = rows_pad, cols_pad
        alloc = torch.zeros if zero else torch.empty     # zero: a writer that does not cover the padding every time
        self.hi = alloc(rows_pad * cols_pad, dtype=torch.int16, device=dev)
        self.lo = alloc(rows_pad * cols_pad, dtype=torch.int16, device=dev) if x3 else None


class _Table:
    """Window table of H standing in for an (implicit) Toeplitz operand: same interface as _Planes."""

    def __init__(self, rows_pad, cols_pad, nbytes, x3, dev):
        self.rows_pad, self.cols_pad = rows_pad, cols_pad
        self.hi = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.lo = torch.empty(nbytes, dtype=torch.uint8, device=dev) if x3 else None


def tail_round_split(mt: int, nt: int, slots: int, k_tiles: int, want: str = '1'):
    """Tail-round split of an EPI_FOLD GEMM with mt x nt tiles on `slots` workgroup slots (two per CU) and k_tiles k-tiles:
    (tail_rows, k_split), (0, 1) = none.  Automatic ('1'): when the tiles make at least one full round plus at most a
    quarter round that is whole tile rows, those rows are contraction-split as far as the free slots, half the k-tiles
    and 8 allow.  'rows,split' forces a choice (tests).  Either way the split is normalised so that every part holds
    ceil(k_tiles / split) k-tiles and none is empty (the kernel's parts are [z * per, (z + 1) * per))."""
    rows, split = 0, 1
    rem = (mt * nt) % slots
    if ',' in want:
        rows, split = (int(v) for v in want.split(','))
        assert 0 < rows <= mt and 2 <= split <= k_tiles
    elif mt * nt > slots and 0 < rem <= slots // 4 and rem % nt == 0 and k_tiles >= 8:
        rows = rem // nt
        split = max(2, min(slots // rem, k_tiles // 2, 8))
    if rows:
        per = -(-k_tiles // split)
        split = -(-k_tiles // per)
        if split < 2:
            rows, split = 0, 1
    return rows, split


def w_contraction_split(tiles: int, k_tiles: int, slots: int) -> int:
    """Split of the W-numerator GEMM's contraction (round 4, the general form): few output tiles and a very long contraction
    (NMF2D: 8 tiles x 2 048 k-tiles) -- as many parts as fill the workgroup slots, at most 64, each at least eight k-tiles,
    dividing the k-tiles evenly (nmfmu_gemm wants k_tiles % k_split == 0)."""
    want = min(64, slots // max(tiles, 1), k_tiles // 8)
    return max([s for s in range(1, max(want, 1) + 1) if k_tiles % s == 0])


def h_tap_fold(rank: int, taps_last: int) -> int:
    """Taps of the last axis folded into the 32-wide N tile of the window-operand GEMM (nmfmu_gemm_desc.win_fold): the
    largest F in {4, 2} with rank * F <= 32 that divides the taps of the last axis, else 1."""
    return max([f for f in (4, 2) if rank * f <= 32 and taps_last % f == 0] + [1])



F16_MIN_DIM = 1024       # 'auto' -> 'f16' from this size on (every contraction at least this long)
F16_MAX_ABS = 3.0e4      # ... and only when V, W, H fit fp16's range with headroom
F16_MIN_MEAN = 2.0 ** -10

# The switches of the convolutive engine: environment variable (after TORCHNMF_AMD_) -> default.  plan_conv reads them, once per
# engine; nothing else in this module looks at the environment.  All but EXPLICIT ('1': explicit Toeplitz planes everywhere) are
# on unless '0'; TAIL_SPLIT also takes 'rows,split' (forced, for tests).  What each one does: DESIGN.md section 3.
SWITCHES = {'NMFD_' + k: '1' for k in ('WINSTAGE', 'FOLD_PARTS', 'FUSED_SUMS', 'FUSED_TABLES', 'H_ROWS', 'H_FOLD', 'KSPLIT',
                                       'ROWS_FUSED', 'TAIL_SPLIT', 'RAGGED', 'RAGGED_IN_GRID', 'NARROW')}
SWITCHES.update(NMFD_EXPLICIT='0', AUTO_F16='1')


@dataclass(frozen=True)
class ConvPlan:
    """What ConvMU decides before it allocates (plan_conv).  None: the field belongs to a path that is not taken."""
    nd: int                  # shift axes: NMFD one, NMF2D / NMF3D two / three (nmf.py:700-942); flattened, the same problem
    L: int                   # flattened extents of V, W, H along the shift axes
    T: int
    Lh: int
    c_pad: int               # C, B L, R T rounded up to the 128 x 128 GEMM tile
    bl_pad: int
    rp_pad: int
    # Hu [(b,l)][(r,t)] = H[b][r][l-t] and its transpose are never materialised when taps and frames (of the last axis) are
    # multiples of 8: the GEMMs fetch them chunk-wise from two window tables of H that are 8x H (nmfmu_conv_tables; several axes:
    # those of every last-axis line of the zero-padded H, nmfmu_convnd_tables) instead of T x H.  The GEMM lanes address a table
    # with 32-bit byte offsets: from 2 GiB on, as on unaligned shapes, explicit planes rebuilt every iteration (nmfmu_conv_unfold)
    implicit: bool
    table_bytes: int         # of one window table (0: explicit planes)
    # H numerator.  fold_parts (one shift axis, >= 128 taps): the GEMM hands over per-tile diagonal sums (NMFMU_EPI_FOLD, 4 KiB a
    # tile) instead of storing Y[(r,t)][(b,l)] (4 R T B L bytes, 105 MB at configs[3]).  h_rows (NMFMU_OPS_A_WIN): no Y at all,
    # out[(b,j)][r] = sum_{t,c} GnT[(b, j + t)][c] W[c][r][t] on shifted rows of the ratio planes; any number of shift axes, no
    # alignment rules.  Neither: store Y, then fold.
    fold_parts: bool
    h_rows: bool
    y_elems: int             # fp32 elements of Y or of the diagonal sums (0 with h_rows)
    h_tail_rows: int         # tail-round split of the fold GEMM (tail_round_split; configs[3]: 1600 tiles on 512 slots = 3 rounds
    h_tail_split: int        # + the last tile row of 64): the parts of those rows add up in the gather, in fixed order
    # C = 128 k + (1..8) channels (1025 bins at configs[3]): the reconstruction GEMMs run over the first 128 k and the rest is
    # summed directly (nmfmu_conv_ragged_rows) -- a whole tile row, a second scheduling round, for one channel otherwise -- or
    # rides in the GEMMs' grids as one extra 16 x 16 MFMA block per workgroup (nmfmu_gemm_desc.rag_c0 / rag_channels)
    ragged: bool
    ragged_in_grid: bool
    c_main: int
    c_rows: Optional[int]    # 64: the GEMMs' channel side runs 64-row tiles (several axes, <= 64 channels); the planes keep their pitch
    loss_main: int           # loss partials of the GEMM part; those of the ragged channels follow
    loss_parts: int
    # beta == 1 launch diets.  fused_sums (fold-parts path): the rank sums ride in the kernels that produce / consume them;
    # fused_tables: the H update also writes the window tables of the new H (nmfmu_conv_fold_parts_apply_h_tables).  rows_fused
    # (window-operand path, >= 64 taps in total, rank <= 256): rank sums in the two apply kernels, Wk planes out of the W update.
    fused_sums: bool
    fused_tables: bool
    rows_fused: bool
    n_hparts: Optional[int]  # partial sums per rank that a fused H update leaves
    wk_rows: Optional[int]   # window-operand GEMM: padded rank,
    wk_fold: Optional[int]   # taps of the last axis folded into the 32-wide N tile (nmfmu_gemm_desc.win_fold: 1 / F of the MFMA work),
    wk_klen: Optional[int]   # length of the (t, c) contraction,
    hj_pad: Optional[int]    # padded positions,
    h_ksplit: Optional[int]  # split of the contraction over idle workgroup slots (few positions, many bins; nmfmu_slab_sum adds up)
    # W numerator GEMM [C x B L] . [B L x R T], few tiles and a long contraction (configs[3]: 225 tiles x 128 k-steps, one
    # workgroup per CU): split in two on the fused-sums path (the apply kernel adds the partials), w_contraction_split otherwise
    w_ksplit: int
    stage_mode: int          # nmfmu_gemm_desc.stage_mode: 0 stages implicit operands as windows where the library admits it
    # 'f16' (fp16 operand planes, window tables and ratio planes: 11 significant bits at the bf16 MFMA rate) exists for beta == 1
    # on window tables (implicit) whose H numerator takes the fold-parts or the window-operand path; 'auto' asks the data (f16_auto) where
    # every contraction is long enough for the rounding errors to average down, and tells the user
    # (f16_warn) when unaligned taps / frames alone cost the fast mode
    f16_ok: bool
    f16_auto: bool
    f16_warn: bool


def plan_conv(lib, B, C, ls, R, ts, beta, own_loop=True, ncu=256, env=None) -> ConvPlan:
    """The plan of ConvMU for V (B, C, *ls), W (C, R, *ts) on ``ncu`` CUs: sizes in, decisions out; no tensor, no device.
    ``lib`` answers the library's static predicates (host code), ``env`` holds the SWITCHES (default: the process environment).
    own_loop=False: a caller that drives the GEMMs itself (plca._ConvPlcaEM, the BetaMu trainer) -- none of the paths that fuse
    this engine's own update into a GEMM's neighbours."""
    env = os.environ if env is None else env
    sw = {k.replace('NMFD_', ''): env.get('TORCHNMF_AMD_' + k, default) for k, default in SWITCHES.items()}
    on = (lambda k: sw[k] != '0')
    ls, ts = tuple(ls), tuple(ts)
    nd, lhs = len(ts), tuple(l - t + 1 for l, t in zip(ls, ts))
    L, T, Lh = math.prod(ls), math.prod(ts), math.prod(lhs)
    kl = float(beta) == 1.0
    cp, blp, rpp = _pad128(C), _pad128(B * L), _pad128(R * T)
    slots = 2 * ncu                                     # workgroup slots of a GEMM: two per CU
    # operands of H
    aligned = ts[-1] % 8 == 0 and ls[-1] % 8 == 0 and sw['EXPLICIT'] != '1'
    table_bytes = 0
    if aligned:
        table_bytes = (lib.nmfmu_convnd_table_bytes(B, R, nd, _i32(lhs), _i32(ts)) if nd > 1 else
                       lib.nmfmu_conv_table_bytes(B, R, Lh, T))
    implicit = 0 < table_bytes < 2 ** 31
    if not implicit:
        table_bytes = 0
    # H numerator
    fold_parts = own_loop and nd == 1 and bool(lib.nmfmu_fold_parts_supported(B, R, Lh, T)) and on('FOLD_PARTS')
    h_rows = T > 1 and not fold_parts and 2 * blp * cp < 2 ** 31 and on('H_ROWS')
    h_tail = (0, 1)
    if fold_parts and sw['TAIL_SPLIT'] != '0':
        h_tail = tail_round_split(rpp // 128, blp // 128, slots, -(-C // 64), sw['TAIL_SPLIT'])
    y_elems = 0 if h_rows else (lib.nmfmu_fold_part_bytes(rpp, blp) // 4) * h_tail[1] if fold_parts else rpp * blp
    wk_rows = wk_fold = wk_klen = hj_pad = h_ksplit = None
    if h_rows:
        wk_rows = 32 if R <= 32 else 64 if R <= 64 else _pad128(R)
        wk_fold = h_tap_fold(R, ts[-1]) if on('H_FOLD') else 1
        wk_klen = (T // wk_fold) * (-(-C // 64)) * 64
        hj_pad = _pad128(B * (Lh // lhs[-1]) * (lhs[-1] + wk_fold - 1))
        h_ksplit = w_contraction_split((hj_pad // 128) * -(-wk_rows // 128), wk_klen // 64, slots) if on('KSPLIT') else 1
    # channels
    c_main = (C // 128) * 128
    ragged = (own_loop and nd == 1 and c_main >= 128 and 0 < C - c_main <= 8 and
              bool(lib.nmfmu_conv_ragged_supported(R, T)) and on('RAGGED'))
    ragged_in_grid = (ragged and implicit and on('RAGGED_IN_GRID') and      # (needs >= 1024 whole channels and frames)
                      bool(lib.nmfmu_gemm_ragged_supported(_capi.OPS_B_HU, c_main, blp, C - c_main)) and
                      bool(lib.nmfmu_gemm_ragged_supported(_capi.OPS_A_HU, blp, c_main, C - c_main)))
    c_rows = 64 if (nd > 1 and implicit and C <= 64 and on('NARROW')) else None
    nrag = lib.nmfmu_conv_ragged_blocks(B, Lh, T) * (C - c_main) if ragged else 0
    # rank sums
    fused_sums = kl and fold_parts and on('FUSED_SUMS')
    fused_tables = fused_sums and implicit and on('FUSED_TABLES')
    rows_fused = own_loop and kl and h_rows and not fused_sums and T >= 64 and R <= 256 and on('ROWS_FUSED')
    n_hparts = None
    if fused_sums:
        n_hparts = lib.nmfmu_fold_hsum_parts_tables(B, Lh) if fused_tables else lib.nmfmu_fold_hsum_parts(B, Lh)
    elif rows_fused:
        n_hparts = lib.nmfmu_conv_h_rows_parts(B, R, Lh // lhs[-1], lhs[-1])
    # W numerator (k-tiles of its contraction as _gemm runs it: the logical B L rounded up to 64 on implicit operands)
    tiles, kt_w = (cp // 128) * (rpp // 128), (-(-(B * L) // 64)) if (implicit and nd == 1) else blp // 64
    w_ksplit = 1
    if on('KSPLIT') and fused_sums:
        w_ksplit = 2 if (tiles <= 256 and kt_w % 2 == 0 and blp >= 2048) else 1
    elif on('KSPLIT'):
        w_ksplit = w_contraction_split(tiles, kt_w, slots)
    # 'f16' in two forms: the fold-parts path with fused sums (Y elements contract over the channels alone) and the
    # window-operand path (over channels x taps).  Only on window tables (`implicit`): explicit planes are written as bf16
    # (nmfmu_conv_unfold), also where aligned taps and frames lose their tables to the 2 GiB limit.
    f16_fold = nd == 1 and T >= 128 and on('FOLD_PARTS') and on('FUSED_SUMS')
    f16_rows = (nd > 1 or 1 < T < 128) and on('H_ROWS')
    f16_ok = own_loop and kl and implicit and (f16_fold or f16_rows) and (fold_parts or h_rows)
    long_fold = min(C, B * L) >= F16_MIN_DIM and R * T >= F16_MIN_DIM
    long_enough = long_fold if f16_fold else min(C * T, B * L, R * T) >= F16_MIN_DIM
    return ConvPlan(
        nd=nd, L=L, T=T, Lh=Lh, c_pad=cp, bl_pad=blp, rp_pad=rpp, implicit=implicit, table_bytes=table_bytes,
        fold_parts=fold_parts, h_rows=h_rows, y_elems=y_elems, h_tail_rows=h_tail[0], h_tail_split=h_tail[1], ragged=ragged,
        ragged_in_grid=ragged_in_grid, c_main=c_main, c_rows=c_rows, loss_main=(c_main // 128) * (blp // 128),
        loss_parts=(cp // 128) * (blp // 128) + nrag, fused_sums=fused_sums, fused_tables=fused_tables, rows_fused=rows_fused,
        n_hparts=n_hparts, wk_rows=wk_rows, wk_fold=wk_fold, wk_klen=wk_klen, hj_pad=hj_pad, h_ksplit=h_ksplit,
        w_ksplit=w_ksplit, stage_mode=1 if sw['WINSTAGE'] == '0' else 0, f16_ok=f16_ok,
        f16_auto=f16_ok and on('AUTO_F16') and long_enough,
        f16_warn=own_loop and nd == 1 and kl and T >= 128 and bool(T % 8 or L % 8) and long_fold)


def resolve_precision(plan: ConvPlan, precision, V, W, H) -> str:
    """The precision the engine runs in.  Only 'auto' on a shape the plan admits to 'f16' looks at data (one host sync)."""
    if precision in (None, 'auto'):
        precision = 'bf16x3'
        if plan.f16_warn:
            warnings.warn(f"torchnmf_amd: NMFD with {plan.T} taps over {plan.L} frames: the single-plane fp16 mode needs taps and "
                          "frames that are multiples of 8 (implicit Toeplitz operands); precision='auto' falls back to "
                          "split bf16 at three times the matrix work.  Trim or pad the frame axis to a multiple of 8 "
                          "for the fast mode.", stacklevel=4)
        if plan.f16_auto:
            stats = torch.stack([V.abs().max(), W.abs().max(), H.abs().max(), V.abs().mean(), W.abs().mean(),
                                 H.abs().mean()]).tolist()
            if max(stats[:3]) <= F16_MAX_ABS and min(stats[3:]) >= F16_MIN_MEAN:
                precision = 'f16'
    if precision not in _capi.PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_capi.PRECISIONS)} or 'auto', got {precision!r}")
    if precision in ('f16r', 'f16x'):
        raise ValueError(f"precision {precision!r} belongs to the dense rank <= 256 kernels; the convolutive engine (NMFD, "
                         "NMF2D, NMF3D, ranks above 256) is built for 'bf16', 'bf16x3' and 'f16'")
    if precision == 'f16' and not plan.f16_ok:
        raise ValueError("precision 'f16' is built for the convolutive models with beta == 1 and taps / frames (of the "
                         "last shift axis) that are multiples of 8 (implicit Toeplitz operands), on shapes whose H "
                         "numerator takes the fold-parts or the window-operand path (ratio planes below 2 GiB); use "
                         "'bf16x3' or 'bf16'")
    return precision


class ConvMU(AsyncLossMixin):
    """Engine for ``NMFD.fit``: V (B, C, L), W (C, R, T), H (B, R, L-T+1); W / H updated in place."""

    def __init__(self, V, W, H, beta, l1=0.0, l2=0.0, precision='auto', update_W=True, update_H=True, own_loop=True):
        self.lib = _capi.load()
        self.staged = {}          # tag of a GEMM launch -> nmfmu_gemm_window_staged() of its descriptor (None: the query failed)
        if not torch.cuda.is_available():
            raise _capi.NmfmuError('torchnmf_amd needs a ROCm device (MI355X); there is no CPU fallback')
        nd = V.dim() - 2
        assert nd in (1, 2, 3) and W.dim() == V.dim() and H.dim() == V.dim()
        B, Cc = V.shape[:2]
        C_, R = W.shape[:2]
        self.ls, self.ts, self.lhs = tuple(V.shape[2:]), tuple(W.shape[2:]), tuple(H.shape[2:])
        assert (C_, tuple(H.shape[:2])) == (Cc, (B, R)) and all(lh == l - t + 1 for lh, l, t in zip(self.lhs, self.ls, self.ts)), \
            'V, W, H shapes are inconsistent'
        for t_ in (W, H):
            assert t_.dtype == torch.float32 and t_.is_contiguous()
        ncu = torch.cuda.get_device_properties(V.device).multi_processor_count
        self.plan = plan_conv(self.lib, B, Cc, self.ls, R, self.ts, beta, own_loop, ncu)
        for fld in fields(self.plan):       # every decision as a plain attribute: what plca.py, trainer.py, tests and tools read
            setattr(self, fld.name, getattr(self.plan, fld.name))
        self.precision_name = resolve_precision(self.plan, precision, V, W, H)
        self.precision = _capi.PRECISIONS[self.precision_name]
        assert not (self.precision == _capi.PREC_F16 and not (self.fold_parts or self.h_rows))   # (f16_ok covers it)
        self.beta = float(beta)
        self.kl = self.beta == 1.0
        self.gamma, self.l1, self.l2 = mu_gamma(self.beta), float(l1), float(l2)
        self.W, self.H = W, H
        self.B, self.C, self.R = B, Cc, R
        self._lh_arr, self._t_arr = _i32(self.lhs), _i32(self.ts)
        self._allocate(V.contiguous(), V.device, self.precision == _capi.PREC_BF16X3)
        self.refresh_images()
        if self.rows_fused:                          # second pass: now through the fused kernel (tile sums of W for the first H update)
            self._pack_w()

    def _allocate(self, V, dev, x3):
        B, Cc, R, L, cp, blp, rpp = self.B, self.C, self.R, self.L, self.c_pad, self.bl_pad, self.rp_pad
        f32 = dict(dtype=torch.float32, device=dev)
        # targets: X_w[c][(b,l)] and X_h[(b,l)][c], fp32, zero padded; validation fused into the first gather
        self.flags = torch.tensor([0, 0x7f800000], dtype=torch.int32, device=dev)
        self.x_w = torch.empty(cp * blp, **f32)
        self.x_h = torch.empty(blp * cp, **f32)
        self._pack2d(V, Cc, B * L, 1, L, 0, L, Cc * L, 1, cp, blp, self.x_w, None, self.flags)
        self._pack2d(V, B * L, Cc, L, Cc * L, 1, 1, L, 0, blp, cp, self.x_h, None, None)
        # operand planes of W, and of H: window tables or explicit planes
        self.wm = _Planes(cp, rpp, x3, dev)     # [c][(r,t)]
        self.wmt = _Planes(rpp, cp, x3, dev)    # [(r,t)][c]
        self.koff = {}
        if self.implicit:
            self.hu = _Table(blp, rpp, self.table_bytes, x3, dev)     # reversed windows: rows (b,l), k = (r,t)
            self.hut = _Table(rpp, blp, self.table_bytes, x3, dev)    # forward windows:  rows (r,t), k = (b,l)
        else:
            self.hu = _Planes(blp, rpp, x3, dev)    # [(b,l)][(r,t)]
            self.hut = _Planes(rpp, blp, x3, dev)   # [(r,t)][(b,l)]
        if self.implicit and self.nd > 1:
            # the k-chunk's share of the chunk index comes from a small precomputed array
            for ops, kp in ((_capi.OPS_B_HU, rpp), (_capi.OPS_B_HUT, blp)):
                host = torch.empty(kp // 8 + 8, dtype=torch.int32)
                _capi.check(self.lib.nmfmu_convnd_koff(ops, B, R, self.nd, self._lh_arr, self._t_arr, kp, host.data_ptr()),
                            'nmfmu_convnd_koff')
                self.koff[ops] = host.to(dev)
            self.koff[_capi.OPS_A_HU] = self.koff[_capi.OPS_B_HU]
        # ratio planes: zero-initialised where the GEMM leaves their padding rows / columns alone
        rz = self.ragged or bool(self.c_rows)
        self.gn = _Planes(cp, blp, x3, dev, rz)     # W half-step ratio, [c][(b,l)]
        self.gnt = _Planes(blp, cp, x3, dev, rz)    # H half-step ratio, [(b,l)][c]
        self.gp = None if self.kl else _Planes(cp, blp, x3, dev, rz)
        self.gpt = None if self.kl else _Planes(blp, cp, x3, dev, rz)
        # numerators / denominators of the H half-step
        self.y = self.y_den = None
        if self.h_rows:
            self.wk = _Planes(self.wk_rows, _pad128(self.wk_klen), x3, dev)         # W as [(r, d)][(to, q, c)]
            self.hnum = torch.empty(self.h_ksplit * self.hj_pad * self.wk_rows, **f32)
            self.hden = None if self.kl else torch.empty_like(self.hnum)
        else:
            self.y = torch.empty(self.y_elems, **f32)
            self.y_den = None if self.kl else torch.empty(self.y_elems, **f32)
        # ... and of the W half-step, one slab per contraction part
        self.num_w = torch.empty(self.w_ksplit * cp * rpp, **f32)
        self.den_w = None if self.kl else torch.empty(self.w_ksplit * cp * rpp, **f32)
        self.sum_h = torch.zeros(R, **f32)   # sum_{b,j} H[b][r][j]
        self.sum_w = torch.zeros(R, **f32)   # sum_{c,t} W[c][r][t]
        self.sum_part = torch.empty(R * 128, **f32)
        if self.fused_sums or self.rows_fused:
            self.hpart = torch.zeros(R * self.n_hparts, **f32)
            self.wcol = torch.zeros((cp // 64) * (rpp // 64) * 2, **f32)
        # fused_tables: the blocks of the H update recompute a halo of their neighbours' elements, so two shadow copies of H
        # alternate as "old, read-only" and "new"; _pack_h -- the path every outside change of H takes -- refreshes them
        self._h_shadow = [torch.empty_like(self.H), torch.empty_like(self.H)] if self.fused_tables else None
        self.loss_part = torch.zeros(self.loss_parts, **f32)  # not all written
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=dev)
        # run-time state: which of the by-products of the fused kernels are current
        self._hs, self._hs_valid = 0, False           # the shadow copy that holds the current H; valid after _pack_h
        self._h_parts_valid = False                   # hpart holds the partial sums of the current H (else sum_h does)
        self._wk_ready, self._wcol_valid = False, False   # wk has been written whole once; wcol holds the tile sums of W

    # ------------------------------------------------------------------ helpers
    def _pack2d(self, src, rows, cols, rin, ros, ris, cin, cos, cis, rows_pad, cols_pad, dst_f32, planes, flags):
        _capi.check(self.lib.nmfmu_pack2d(src.data_ptr(), rows, cols, rin, ros, ris, cin, cos, cis, rows_pad, cols_pad,
                                          _ptr(dst_f32), _ptr(planes.hi) if planes else None,
                                          _ptr(planes.lo) if planes else None, _ptr(flags), _stream()), 'nmfmu_pack2d')

    def _gemm(self, a: _Planes, b: _Planes, epi, x=None, gn=None, gp=None, out=None, m_valid=0, n_valid=0, m_rows=None,
              n_rows=None, k_len=0, k_split=0, tail_rows=0, ragged=False, tag=None):
        """D = A B^T with the given epilogue.  m_rows / n_rows: only the first rows of A / of B (ragged channels); the
        output planes keep their leading dimension.  tag: name of the launch for an attached KernelTimer (bench.py)."""
        assert a.cols_pad == b.cols_pad
        m_pad, n_pad = m_rows or a.rows_pad, n_rows or b.rows_pad
        n_ld = b.rows_pad if n_rows else 0
        ops = _capi.OPS_PLANES
        if self.implicit:
            ops = (_capi.OPS_A_HU if a is self.hu else _capi.OPS_B_HU if b is self.hu else
                   _capi.OPS_B_HUT if b is self.hut else _capi.OPS_PLANES)
        if not k_len and ops != _capi.OPS_PLANES and self.nd == 1:
            # the contraction of an implicit operand runs over its logical extent rounded up to whole k-tiles, not over the
            # 128-padded pitch of the explicit planes (whose tail is zero): one k-tile less for half of all shapes, and the form
            # the library's window staging asks for (nmfmu_gemm_window_staged: k_len == the logical extent)
            k_len = -(-(self.B * self.L if ops == _capi.OPS_B_HUT else self.R * self.T) // 64) * 64
        d = _capi.GemmDesc(_ptr(a.hi), _ptr(a.lo), _ptr(b.hi), _ptr(b.lo), m_pad, n_pad, a.cols_pad,
                           self.precision, self.beta, _ptr(x), _ptr(gn.hi) if gn else None,
                           _ptr(gn.lo) if gn else None, _ptr(gp.hi) if gp else None, _ptr(gp.lo) if gp else None,
                           _ptr(out), m_valid, n_valid, ops, self.B, self.R, self.T, self.Lh, 128, n_ld, k_len, k_split,
                           tail_rows, self.c_main if ragged else 0, self.C if ragged else 0)
        if ops != _capi.OPS_PLANES and self.nd > 1:
            d.win_nd, d.win_lh, d.win_taps = self.nd, (C.c_int32 * 3)(*self.lhs), (C.c_int32 * 3)(*self.ts)
            d.t_koff = self.koff[ops].data_ptr()
        d.stage_mode = self.stage_mode
        if tag and tag not in self.staged:       # which launches stage their implicit operand as a window (host-side query, once)
            q = int(self.lib.nmfmu_gemm_window_staged(C.byref(d), epi))
            self.staged[tag] = q if q >= 0 else None        # (a negative answer is an error code, not a flag)
        self._launch_gemm(d, epi, tag)

    def _launch_gemm(self, d, epi, tag):
        timer = getattr(self, 'timer', None) if tag else None
        if timer is not None:
            timer.mark(tag + '<')
        _capi.check(self.lib.nmfmu_gemm(C.byref(d), epi, _stream()), 'nmfmu_gemm')
        if timer is not None:
            timer.mark(tag + '>')

    def _gemm_win(self, planes: _Planes, out, tag=None):
        """H numerator (or denominator) as the window-operand GEMM: out[(b,j)][r] from the ratio planes [(b,l)][c]."""
        d = _capi.GemmDesc(_ptr(planes.hi), _ptr(planes.lo), _ptr(self.wk.hi), _ptr(self.wk.lo), self.hj_pad, self.wk_rows,
                           self.wk.cols_pad, self.precision, self.beta, None, None, None, None, None, _ptr(out), 0, 0,
                           _capi.OPS_A_WIN, self.B, self.R, self.T, self.Lh, 128, 0, self.wk_klen, self.h_ksplit, 0, 0, 0,
                           self.nd, (C.c_int32 * 3)(*self.lhs), (C.c_int32 * 3)(*self.ts), self.C, planes.cols_pad,
                           self.wk_fold)
        self._launch_gemm(d, _capi.EPI_F32, tag)
        if self.h_ksplit > 1:
            _capi.check(self.lib.nmfmu_slab_sum(out.data_ptr(), self.hj_pad * self.wk_rows, self.h_ksplit, _stream()),
                        'nmfmu_slab_sum')

    def _ragged(self, mode, x, gn=None, gp=None):
        """The channels the reconstruction GEMM left out (mode 0: W half-step planes, 1: H half-step planes, 2: loss)."""
        ld = self.bl_pad if mode != 1 else self.c_pad
        loss = self.loss_part.data_ptr() + 4 * self.loss_main if mode == 2 else None
        _capi.check(self.lib.nmfmu_conv_ragged_rows(
            self.W.data_ptr(), self.C, self.R, self.T, self.H.data_ptr(), self.B, self.Lh, self.c_main, self.precision,
            self.beta, mode, x.data_ptr(), ld, _ptr(gn.hi) if gn else None, _ptr(gn.lo) if gn else None,
            _ptr(gp.hi) if gp else None, _ptr(gp.lo) if gp else None, loss, _stream()), 'nmfmu_conv_ragged_rows')

    def _rank_sums(self, src, outer, inner, out):
        """beta == 1 denominators (nmf.py:122-131): sum over everything but the rank axis.  (Running these two small
        kernels on a side stream beside the next GEMM was measured: no gain -- the event fork / join costs what the
        overlap saves; the same holds for the ragged-channel kernel beside its reconstruction GEMM.)"""
        if self.kl:
            _capi.check(self.lib.nmfmu_rank_sums(src.data_ptr(), outer, self.R, inner, self.sum_part.data_ptr(),
                                                 out.data_ptr(), _stream()), 'nmfmu_rank_sums')

    def _sum_h_args(self, use: bool):
        """(sum_h, hpart) of a fused W update: the finished vector after an outside change of H, else the partial sums the
        fused H update left; both null when the launch does not update."""
        if not use:
            return None, None
        return (None, self.hpart.data_ptr()) if self._h_parts_valid else (self.sum_h.data_ptr(), None)

    def _pack_w(self, update: bool = False):
        """W -> Wm / WmT planes (one kernel); with ``update`` the MU apply of nmf.py:78-92 runs in the same pass."""
        if self.fused_sums:
            return self._pack_w_sums(update)
        slabs = self.w_ksplit
        if update and (slabs > 2 or (slabs > 1 and self.c_rows)):
            # many split-K partials: a wide reduction first (the apply kernel has few blocks).  A slab holds the rows the GEMM
            # ran over (c_rows of them when the channel side uses the 64-row tile)
            for buf in (self.num_w, self.den_w):
                if buf is not None:
                    _capi.check(self.lib.nmfmu_slab_sum(buf.data_ptr(), (self.c_rows or self.c_pad) * self.rp_pad, slabs,
                                                        _stream()), 'nmfmu_slab_sum')
            slabs = 1
        if self.rows_fused and self._wk_ready:
            self._pack_w_wk(update, slabs)
        else:
            self._pack_w_plain(update, slabs)

    def _pack_w_sums(self, update):
        """fused_sums: sum_h arrives finished or as partials, the column sums of the new W leave as per-64-channel-tile
        partials for the H half-step (no rank_sums launches)."""
        sum_h, hpart = self._sum_h_args(update and self.kl)
        _capi.check(self.lib.nmfmu_conv_apply_pack_w_sums(
            self.W.data_ptr(), self.C, self.R, self.T, _ptr(self.num_w) if update else None, None, sum_h, hpart,
            self.n_hparts, self.wcol.data_ptr(), self.w_ksplit, self.c_pad, self.rp_pad, self.l1, self.l2, self.gamma,
            int(update), self.precision, _ptr(self.wm.hi), _ptr(self.wm.lo), _ptr(self.wmt.hi), _ptr(self.wmt.lo), _stream()),
            'nmfmu_conv_apply_pack_w_sums')

    def _pack_w_wk(self, update, slabs):
        """rows_fused, one launch: the update, Wm / WmT / Wk planes, tile sums of the new W for the H update."""
        sum_h, hpart = self._sum_h_args(update)
        _capi.check(self.lib.nmfmu_conv_apply_pack_w_wk(
            self.W.data_ptr(), self.C, self.R, self.T, _ptr(self.num_w) if update else None, None, sum_h, hpart,
            self.n_hparts, self.wcol.data_ptr(), slabs, self.c_pad, self.rp_pad, self.l1, self.l2, self.gamma, int(update),
            self.precision, _ptr(self.wm.hi), _ptr(self.wm.lo), _ptr(self.wmt.hi), _ptr(self.wmt.lo), self.ts[-1],
            self.wk_fold, self.wk.rows_pad, self.wk.cols_pad, _ptr(self.wk.hi), _ptr(self.wk.lo), _stream()),
            'nmfmu_conv_apply_pack_w_wk')
        self._wcol_valid = True

    def _pack_w_plain(self, update, slabs):
        """The _sums entry without its partial-sum operands (it adds the split-K slabs of num / den); rank sums of the new W
        and, on the window-operand path, the Wk planes by launches of their own."""
        _capi.check(self.lib.nmfmu_conv_apply_pack_w_sums(
            self.W.data_ptr(), self.C, self.R, self.T, _ptr(self.num_w) if update else None,
            _ptr(self.den_w) if update else None, self.sum_h.data_ptr() if (update and self.kl) else None, None, 0, None,
            slabs, self.c_pad, self.rp_pad, self.l1, self.l2, self.gamma, int(update), self.precision,
            _ptr(self.wm.hi), _ptr(self.wm.lo), _ptr(self.wmt.hi), _ptr(self.wmt.lo), _stream()),
            'nmfmu_conv_apply_pack_w_sums')
        self._rank_sums(self.W, self.C, self.T, self.sum_w)
        if self.h_rows:
            self._wk_ready = True                    # (the standalone kernel also writes the planes' zero padding: once)
            _capi.check(self.lib.nmfmu_conv_pack_wk(self.W.data_ptr(), self.C, self.R, self.T, self.ts[-1], self.wk_fold,
                                                    self.wk.rows_pad, self.wk.cols_pad, self.precision, _ptr(self.wk.hi),
                                                    _ptr(self.wk.lo), _stream()), 'nmfmu_conv_pack_wk')

    def _pack_h(self, sums: bool = True):
        if self.implicit and self.nd > 1:
            _capi.check(self.lib.nmfmu_convnd_tables(self.H.data_ptr(), self.B, self.R, self.nd, self._lh_arr, self._t_arr,
                                                     self.precision, _ptr(self.hu.hi), _ptr(self.hu.lo), _ptr(self.hut.hi),
                                                     _ptr(self.hut.lo), _stream()), 'nmfmu_convnd_tables')
        elif self.implicit:
            if self.precision == _capi.PREC_F16:
                _capi.check(self.lib.nmfmu_conv_tables_f16(self.H.data_ptr(), self.B, self.R, self.Lh, self.T,
                                                           _ptr(self.hu.hi), _ptr(self.hut.hi), _stream()),
                            'nmfmu_conv_tables_f16')
            else:
                _capi.check(self.lib.nmfmu_conv_tables(self.H.data_ptr(), self.B, self.R, self.Lh, self.T,
                                                       _ptr(self.hu.hi), _ptr(self.hu.lo), _ptr(self.hut.hi),
                                                       _ptr(self.hut.lo), _stream()), 'nmfmu_conv_tables')
        else:
            self._unfold()
        if self.fused_tables:
            self._h_shadow[self._hs].copy_(self.H)
            self._hs_valid = True
        if sums:
            self._rank_sums(self.H, self.B, self.Lh, self.sum_h)
            self._h_parts_valid = False

    def _unfold(self):
        if self.nd == 1:
            _capi.check(self.lib.nmfmu_conv_unfold(self.H.data_ptr(), self.B, self.R, self.Lh, self.T, _ptr(self.hu.hi),
                                                   _ptr(self.hu.lo), _ptr(self.hut.hi), _ptr(self.hut.lo), self.bl_pad,
                                                   self.rp_pad, _stream()), 'nmfmu_conv_unfold')
        else:
            _capi.check(self.lib.nmfmu_convnd_unfold(self.H.data_ptr(), self.B, self.R, self.nd, self._lh_arr,
                                                     self._t_arr, _ptr(self.hu.hi), _ptr(self.hu.lo), _ptr(self.hut.hi),
                                                     _ptr(self.hut.lo), self.bl_pad, self.rp_pad, _stream()),
                        'nmfmu_convnd_unfold')

    def refresh_images(self):
        self._pack_w()
        self._pack_h()

    # ------------------------------------------------------------------ the fit-loop interface (see nmf.BaseComponent.fit)
    def target_flags(self):
        bad, mn = (int(x) for x in self.flags.tolist())
        return bool(bad), mn == 0

    def _gemm_channels(self):
        """Channel rows the reconstruction GEMMs run over (None: all of the padded ones)."""
        return self.c_main if self.ragged else self.c_rows

    def recon_ratio_w(self):
        """Reconstruction + ratio planes of the W half-step (nmf.py:61-74 on Wm Hu^T): the GEMM over the channels that
        fill whole tiles, the ragged ones by direct summation."""
        self._gemm(self.wm, self.hu, _capi.EPI_RATIO, x=self.x_w, gn=self.gn, gp=self.gp, m_rows=self._gemm_channels(),
                   ragged=self.ragged_in_grid, tag='recon_w')
        if self.ragged and not self.ragged_in_grid:
            self._ragged(0, self.x_w, self.gn, self.gp)

    def w_step(self):
        """nmf.py:367-378 for the conv1d model."""
        self.recon_ratio_w()
        self._gemm(self.gn, self.hut, _capi.EPI_F32, out=self.num_w, k_split=self.w_ksplit, m_rows=self.c_rows, tag='num_w')
        if not self.kl:
            self._gemm(self.gp, self.hut, _capi.EPI_F32, out=self.den_w, k_split=self.w_ksplit, m_rows=self.c_rows)
        self._pack_w(update=True)

    def recon_ratio_h(self):
        """Reconstruction + ratio planes of the H half-step (the transposed problem Hu Wm^T against V^T), split like
        ``recon_ratio_w``."""
        self._gemm(self.hu, self.wm, _capi.EPI_RATIO, x=self.x_h, gn=self.gnt, gp=self.gpt, n_rows=self._gemm_channels(),
                   ragged=self.ragged_in_grid, tag='recon_h')
        if self.ragged and not self.ragged_in_grid:
            self._ragged(1, self.x_h, self.gnt, self.gpt)

    def h_step(self):
        """nmf.py:380-391 for the conv1d model (uses the freshly updated W), on the H-numerator path the plan chose."""
        self.recon_ratio_h()
        if self.h_rows:
            self._h_step_window()
        elif self.fold_parts:
            self._h_step_fold_parts()
        else:
            self._h_step_store_fold()

    def _h_step_window(self):
        """Window-operand GEMM; with rows_fused the update takes the tile sums of W and leaves partial sums of the new H."""
        self._gemm_win(self.gnt, self.hnum, tag='num_h')
        if not self.kl:
            self._gemm_win(self.gpt, self.hden)
        rows = (self.H.data_ptr(), self.B, self.R, self.Lh // self.lhs[-1], self.lhs[-1], self.wk_fold, self.hnum.data_ptr())
        if self.rows_fused and self._wcol_valid:
            _capi.check(self.lib.nmfmu_conv_apply_h_rows_sums(
                *rows, self.wcol.data_ptr(), self.c_pad // 64, self.rp_pad, self.T, self.wk_rows, self.l1, self.l2, self.gamma,
                self.hpart.data_ptr(), _stream()), 'nmfmu_conv_apply_h_rows_sums')
            self._pack_h(sums=False)
            self._h_parts_valid = True
            return
        # with rows_fused the rank sums ride in the fused kernels and self.sum_w is only as fresh as the last unfused pass:
        # the unfused update must not be reached once the fused form has run
        assert not (self.rows_fused and self._h_parts_valid), 'stale sum_w: the unfused H update after a fused one'
        _capi.check(self.lib.nmfmu_conv_apply_h_rows(
            *rows, _ptr(self.hden), self.sum_w.data_ptr() if self.kl else None, self.wk_rows, self.l1, self.l2, self.gamma,
            _stream()), 'nmfmu_conv_apply_h_rows')
        self._pack_h()

    def _num_h_gemm(self, epi):
        kc = -(-self.C // 64) * 64             # the contraction runs over the channels: skip the zero tail of the padding
        tail = dict(k_split=self.h_tail_split, tail_rows=self.h_tail_rows) if self.h_tail_rows else {}
        self._gemm(self.wmt, self.gnt, epi, out=self.y, k_len=kc, tag='num_h', **tail)
        if not self.kl:
            self._gemm(self.wmt, self.gpt, epi, out=self.y_den, k_len=kc, **tail)

    def _h_step_fold_parts(self):
        """Per-tile diagonal sums, gathered by the update; fused_sums: it takes the tile sums of W and leaves partial sums of
        the new H; fused_tables: it writes the window tables of the new H as well."""
        self._num_h_gemm(_capi.EPI_FOLD)
        fold = (self.B, self.R, self.Lh, self.T, self.y.data_ptr())
        tail = (self.bl_pad, self.l1, self.l2, self.gamma, self.rp_pad, self.h_tail_rows, self.h_tail_split)
        if not self.fused_sums:
            _capi.check(self.lib.nmfmu_conv_fold_parts_apply_h_tail(
                self.H.data_ptr(), *fold, _ptr(self.y_den), self.sum_w.data_ptr() if self.kl else None, None, 0, 0, None,
                *tail, _stream()), 'nmfmu_conv_fold_parts_apply_h_tail')
            return self._pack_h()
        sums = (None, None, self.wcol.data_ptr(), self.c_pad // 64, self.rp_pad, self.hpart.data_ptr())
        if self.fused_tables and self._hs_valid:
            old, new = self._h_shadow[self._hs], self._h_shadow[self._hs ^ 1]
            _capi.check(self.lib.nmfmu_conv_fold_parts_apply_h_tables(
                self.H.data_ptr(), old.data_ptr(), new.data_ptr(), *fold, *sums, *tail, self.precision, _ptr(self.hu.hi),
                _ptr(self.hu.lo), _ptr(self.hut.hi), _ptr(self.hut.lo), _stream()), 'nmfmu_conv_fold_parts_apply_h_tables')
            self._hs ^= 1
        else:
            _capi.check(self.lib.nmfmu_conv_fold_parts_apply_h_tail(self.H.data_ptr(), *fold, *sums, *tail, _stream()),
                        'nmfmu_conv_fold_parts_apply_h_tail')
            self._pack_h(sums=False)
        self._h_parts_valid = True

    def _h_step_store_fold(self):
        """Numerator Y[(r,t)][(b,l)] stored whole, then the col2im sum and the update in one kernel."""
        self._num_h_gemm(_capi.EPI_F32)
        kl_den = self.sum_w.data_ptr() if self.kl else None
        if self.nd == 1:
            _capi.check(self.lib.nmfmu_conv_fold_apply_h(self.H.data_ptr(), self.B, self.R, self.Lh, self.T,
                                                         self.y.data_ptr(), _ptr(self.y_den), kl_den, self.bl_pad,
                                                         self.l1, self.l2, self.gamma, _stream()),
                        'nmfmu_conv_fold_apply_h')
        else:
            _capi.check(self.lib.nmfmu_convnd_fold_apply_h(self.H.data_ptr(), self.B, self.R, self.nd, self._lh_arr,
                                                           self._t_arr, self.y.data_ptr(), _ptr(self.y_den), kl_den,
                                                           self.bl_pad, self.l1, self.l2, self.gamma, _stream()),
                        'nmfmu_convnd_fold_apply_h')
        self._pack_h()

    def left_f16_range(self) -> bool:
        """'f16' only: the range gate of 'auto' / the constructor looks at the initial data.  A factor value
        that grows beyond fp16's largest finite number during the fit is clamped to 65504 in the operand planes / window
        tables, and the updates stop following the reference.  fit() asks at its loss checkpoints (one more host sync
        there, two small reductions) and warns."""
        if self.precision != _capi.PREC_F16:
            return False
        return bool(torch.maximum(self.W.max(), self.H.max()).item() > 65504.0)

    def _loss_device(self):
        """Enqueue beta_div(conv1d reconstruction, V) (nmf.py:360-361 / 400-401); the value as a float64[1] device tensor."""
        self._gemm(self.wm, self.hu, _capi.EPI_LOSS, x=self.x_w, out=self.loss_part, m_valid=self.C,
                   n_valid=self.B * self.L, m_rows=self._gemm_channels())
        if self.ragged:
            self._ragged(2, self.x_w)
        return self.loss_part.double().sum().reshape(1)

    def _range_flag_device(self):
        if self.precision != _capi.PREC_F16:
            return None
        return (torch.maximum(self.W.max(), self.H.max()) > 65504.0).double().reshape(1)

    def _ckpt_tensors(self):
        return [self.W, self.H]

    def divergence(self) -> float:
        """One host sync."""
        return float(self._loss_device().item())


class WideRankMU:
    """``NMF.fit`` for ranks above 256.  The fused kernel keeps a rank-wide accumulator tile in registers, which
    stops at a padded rank of 256; a wider NMF is the T = 1 member of the NMFD family -- V^T as (1, C, N), W as
    (C, R, 1), H^T as (1, R, N) -- and runs on the GEMM engine, whose effective rank R*T is unbounded.  W shares
    storage with the parameter; H is kept transposed and copied back after every H half-step (N x R floats)."""

    def __init__(self, V, W, H, beta, l1=0.0, l2=0.0, precision='auto', update_W=True, update_H=True):
        assert V.dim() == 2 and W.dim() == 2 and H.dim() == 2
        self.H_user = H
        self.Ht = H.t().contiguous().unsqueeze(0)
        self.eng = ConvMU(V.t().contiguous().unsqueeze(0), W.unsqueeze(2), self.Ht, beta, l1, l2, precision=precision,
                          update_W=update_W, update_H=update_H)
        self.precision_name = self.eng.precision_name

    def target_flags(self):
        return self.eng.target_flags()

    def refresh_images(self):
        """After external edits of W / H (sparse_fit): the transposed working copy of H, then the engine's images."""
        self.Ht[0].copy_(self.H_user.t())
        self.eng.refresh_images()

    def w_step(self):
        self.eng.w_step()

    def h_step(self):
        self.eng.h_step()
        self.H_user.copy_(self.Ht[0].t())

    def divergence(self) -> float:
        return self.eng.divergence()


def reconstruct(H: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """``NMFD / NMF2D / NMF3D.reconstruct`` (nmf.py:776-779, 857-860, 937-940) on the device: Wm @ Hu^T through the
    split-bf16 GEMM, fp32 out."""
    if H.device.type != 'cuda' or W.device.type != 'cuda':
        raise _capi.NmfmuError('reconstruct: tensors must live on the ROCm device (no CPU fallback)')
    lib = _capi.load()
    Hc, Wc = H.detach().float().contiguous(), W.detach().float().contiguous()
    nd = Hc.dim() - 2
    assert nd in (1, 2, 3) and Wc.dim() == Hc.dim()
    B, R = Hc.shape[:2]
    Cc, R2 = Wc.shape[:2]
    assert R == R2
    lhs, ts = tuple(Hc.shape[2:]), tuple(Wc.shape[2:])
    ls = tuple(lh + t - 1 for lh, t in zip(lhs, ts))
    L, T = int(torch.tensor(ls).prod()), int(torch.tensor(ts).prod())
    dev = H.device
    cp, blp, rpp = _pad128(Cc), _pad128(B * L), _pad128(R * T)
    wm, hu, hut = _Planes(cp, rpp, True, dev), _Planes(blp, rpp, True, dev), _Planes(rpp, blp, True, dev)
    RT = R * T
    _capi.check(lib.nmfmu_pack2d(Wc.data_ptr(), Cc, RT, 1, RT, 0, 1, 1, 0, cp, rpp, None, _ptr(wm.hi), _ptr(wm.lo), None,
                                 _stream()), 'nmfmu_pack2d')
    if nd == 1:
        _capi.check(lib.nmfmu_conv_unfold(Hc.data_ptr(), B, R, lhs[0], T, _ptr(hu.hi), _ptr(hu.lo), _ptr(hut.hi),
                                          _ptr(hut.lo), blp, rpp, _stream()), 'nmfmu_conv_unfold')
    else:
        _capi.check(lib.nmfmu_convnd_unfold(Hc.data_ptr(), B, R, nd, (C.c_int32 * nd)(*lhs), (C.c_int32 * nd)(*ts),
                                            _ptr(hu.hi), _ptr(hu.lo), _ptr(hut.hi), _ptr(hut.lo), blp, rpp, _stream()),
                    'nmfmu_convnd_unfold')
    out = torch.empty(cp, blp, dtype=torch.float32, device=dev)
    d = _capi.GemmDesc(_ptr(wm.hi), _ptr(wm.lo), _ptr(hu.hi), _ptr(hu.lo), cp, blp, rpp, _capi.PREC_BF16X3, 2.0, None,
                       None, None, None, None, out.data_ptr(), 0, 0, _capi.OPS_PLANES, 0, 0, 0, 0)
    _capi.check(lib.nmfmu_gemm(C.byref(d), _capi.EPI_F32, _stream()), 'nmfmu_gemm')
    return out[:Cc, :B * L].reshape(Cc, B, *ls).transpose(0, 1).contiguous()
