"""The ping-pong MU kernel's "transpose in LDS" instance (NMFMU_STAGE_DMA_LDSTR, csrc/nmfmu_pp.h: PPCfg::TRL).

The instance fetches ONE panel image per tile (P1, row-major) and builds the transposed tile of the second GEMM (P2) in LDS:
per wave and tile four ds_read_b64_tr_b16 from the landed P1 ring slot and four ds_write_b64 into the P2 ring slot, at the
addresses the matrix segment reads.  Operand values and MFMA order are those of the two-image instance, so everything it
computes must be BIT-identical to it, and nothing may depend on the transposed images in HBM any more.

CPU: the lane map of the transposing read (as probed by tools/ubench/tr_probe.hip) plus the kernel's source / destination
address formulas, replayed on an integer-tagged tile.  GPU: torch.equal against the two-image instance, NaN-poisoned P2
buffers, and one case against the oracle.
"""
import numpy as np
import pytest
import torch

from test_layout_emulation import _tr_read, p1_offset, p2_offset

R_PAD = 128
ROWB = 2 * R_PAD            # bytes per P1 row
IMG = 64 * ROWB             # bytes of one image tile
NSLOT = 3
P1_BASE, P2_BASE = 0, NSLOT * IMG


# ---- CPU: lane map + addresses -------------------------------------------------------------------------------------------
def _wave_addresses(wave, slot):
    """nmfmu_pp.h (PPCfg::TRL): per-lane byte addresses of wave `wave`'s four read / write pairs, ring slot `slot`."""
    rt, tt = wave & 3, wave >> 2
    src, dst = [], []
    for p in range(4):
        s_, d_ = [], []
        for lane in range(64):
            j, hl = lane & 31, lane >> 5
            grp, s16 = lane >> 4, lane & 15
            i4 = s16 >> 2
            cslot = 2 * (grp & 1) + ((s16 & 3) >> 1)
            tr_src = P1_BASE + slot * IMG + (32 * (grp >> 1) + 16 * tt + i4) * ROWB + (((((rt ^ i4) << 2) | cslot) << 4) + 8 * (s16 & 1))
            tr_dst = P2_BASE + slot * IMG + (32 * rt + j) * 128 + (((4 * hl + 2 * tt) ^ ((j >> 1) & 7)) << 4)
            s_.append((tr_src ^ (16 * p)) + 4 * p * ROWB)
            d_.append((tr_dst ^ (16 * (p >> 1))) + 8 * (p & 1))
        src.append(s_)
        dst.append(d_)
    return src, dst


@pytest.mark.parametrize('slot', range(NSLOT))
def test_lds_transpose_builds_the_dma_image(slot):
    """Every (panel row, rank) pair at padded rank 128, every ring slot: the eight waves' 32 read / write pairs turn the P1
    tile that LDS-DMA placed (a linear copy of the HBM tile) into exactly the P2 tile LDS-DMA would have placed; every write
    is 8-byte aligned, no element is written twice, nothing outside the slot is touched; each 32-lane pass of a transposing
    read touches every bank once."""
    lds = np.full(2 * NSLOT * IMG // 2, 0xFFFF, dtype=np.uint16)        # the kernel's LDS, in 16-bit elements
    want = lds.copy()
    for row in range(64):
        for r in range(R_PAD):
            tag = row * R_PAD + r                                       # < 8192: unique, never the fill value
            lds[(P1_BASE + slot * IMG) // 2 + p1_offset(row, r, R_PAD)] = tag
            want[(P1_BASE + slot * IMG) // 2 + p1_offset(row, r, R_PAD)] = tag
            want[(P2_BASE + slot * IMG) // 2 + p2_offset(row, r, R_PAD)] = tag
    written = set()
    for wave in range(8):
        src, dst = _wave_addresses(wave, slot)
        for p in range(4):
            assert all(a % 8 == 0 for a in src[p]) and all(a % 8 == 0 for a in dst[p])
            got = _tr_read(lds, src[p])
            for half in range(2):
                banks = []
                for lane in range(32 * half, 32 * half + 32):
                    banks += [(src[p][lane] // 4) % 64, (src[p][lane] // 4 + 1) % 64]
                assert len(set(banks)) == 64, ('bank conflict', wave, p, half)
            for lane in range(64):
                assert P2_BASE + slot * IMG <= dst[p][lane] < P2_BASE + (slot + 1) * IMG
                for i in range(4):
                    e = dst[p][lane] // 2 + i
                    assert e not in written
                    written.add(e)
                    lds[e] = got[lane, i]
    assert len(written) == 64 * R_PAD
    np.testing.assert_array_equal(lds, want)


def test_lds_transpose_slot_schedule():
    """Ring-slot reuse of the schedule in nmfmu_pp.h, segment by segment (segment s = 2t: A runs M(t), B runs E(t-1);
    s = 2t+1: A runs E(t), B runs M(t); M(t) reads P1(t) and P2(t-1); the peeled last tile pre-reads P2(nt-1) in its E):
    every wave builds P2(t+1) from P1(t+1) in its E(t).  P1(t+1) must have landed and must not yet be overwritten, the
    destination slot's previous tenant must have been read for the last time in an EARLIER segment, and the first reader of
    P2(t+1) must come in a LATER segment than the last writer."""
    for nt in (2, 4, 6, 8):
        p1_ready = {u: (0 if u < 2 else 2 * u - 1) for u in range(nt)}        # first segment in which P1(u) may be read
        p1_gone = {u: 2 * u + 3 for u in range(nt)}                           # segment whose DMA overwrites P1(u)'s slot (P1(u+3))
        reads = {u: [2 * u + 2, 2 * u + 3] for u in range(nt)}                # segments that read P2(u): A's, B's M(u+1)
        reads[nt - 1] = [2 * (nt - 1) + 1, 2 * (nt - 1) + 2, 2 * nt, 2 * nt + 1]   # last tile: operand pre-reads in E(nt-1) as well
        writes = {0: [0, 0]}                                                  # prologue: behind the first barrier
        for t in range(nt - 1):
            writes[t + 1] = [2 * t + 1, 2 * t + 2]                            # A's E(t), B's E(t)
        for u in range(nt):
            assert min(writes[u]) >= p1_ready[u] and max(writes[u]) < p1_gone[u], (nt, u)
            assert max(writes[u]) < min(reads[u]), (nt, u)
            if u >= NSLOT:
                assert max(reads[u - NSLOT]) < min(writes[u]), (nt, u)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _engine(dev, V, W0, H0, prec, stage, l1=0.0, l2=0.0):
    from torchnmf_amd.engine import DenseMU
    W = W0.clone().to(dev).contiguous()
    H = H0.clone().to(dev).contiguous()
    eng = DenseMU(V.to(dev), W, H, 1.0, l1, l2, precision=prec, stage=stage)
    assert eng.step_w.block_rows == 256 and eng.step_h.block_rows == 256
    return eng, W, H


def _snapshot(eng, W, H):
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (W, H, eng.fW.colsum, eng.fH.colsum, eng.fW.p1_hi, eng.fH.p1_hi)]


def _run(dev, V, W0, H0, prec, stage, nsplit, iters=2, l1=0.0, l2=0.0, poison=False, riding=False):
    """`iters` iterations (W half-step, H half-step); a snapshot of W, H, both column sums and both P1 images after each."""
    eng, W, H = _engine(dev, V, W0, H0, prec, stage, l1, l2)
    if nsplit is not None:
        for st in (eng.step_w, eng.step_h):
            ktiles = st.panel.rows_pad // 64
            if nsplit > 1 and ktiles // nsplit < 2:
                pytest.fail('shape too short for the requested split')
            if st.nsplit != nsplit:
                st.nsplit = st.struct.nsplit = nsplit
                st.slab_num = torch.empty(nsplit * st.plane, dtype=torch.float32, device=dev)
                st.struct.slab_num = st.slab_num.data_ptr()
    if poison:   # NaN bit patterns (fp16 0x7e00 / bf16 0x7fc0 pairs) over both transposed images
        for f in (eng.fW, eng.fH):
            f.p2_hi.view(torch.int16).fill_(0x7e00 if prec != 'bf16' else 0x7fc0)
    out = []
    for it in range(iters):
        if riding and it == 0:
            eng.checkpoint_begin()
            assert eng._riding_pending
        eng.w_step()
        eng.h_step()
        if riding and it == 0:
            out.append(eng.checkpoint_result()[0])
        out.append(_snapshot(eng, W, H))
    return out


def _data(N, C, R, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, C, generator=g), torch.randn(C, R, generator=g).abs(), torch.randn(N, R, generator=g).abs()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


def _assert_same(a, b, what):
    names = ('W', 'H', 'colsum W', 'colsum H', 'P1 W', 'P1 H')
    for it, (sa, sb) in enumerate(zip(a, b)):
        if not isinstance(sa, list):
            assert sa == sb, (what, 'riding loss', sa, sb)
            continue
        for n, x, y in zip(names, sa, sb):
            assert torch.equal(x, y), (what, 'iteration', it + 1, n)
    # (the images hold the fp16 / bf16 roundings of W and H: a NaN anywhere would show in torch.equal as a mismatch)
    assert all(torch.isfinite(x[0]).all() and torch.isfinite(x[1]).all() for x in a if isinstance(x, list))


# The W half-step has C owner rows and contracts over N, the H half-step the other way round; both axes are padded to 256 rows,
# so a contraction of 128 / 256 columns is 4 tiles and one of 384 is 8.  Owner rows 256, 300 (ragged tile, general epilogue
# branch) and 512; contractions 128, 256, 384 and -- for a workgroup that really runs SIX tiles -- 700; rank 128 and 100 -> 128;
# both operand types; fused apply (nsplit 1: 4 or 8 tiles per workgroup) and slabs + apply kernel (nsplit 2: 2 tiles = prologue
# and straight-line tail only, 4, and 6 = the three-slot ring wraps inside the loop).
CASES = [
    # N,   C,   R,   prec,  nsplit
    (256, 128, 128, 'f16', 1),
    (300, 256, 100, 'f16', 1),
    (256, 300, 128, 'bf16', 1),
    (384, 512, 128, 'f16', 1),
    (512, 384, 100, 'bf16', 1),
    (256, 128, 128, 'bf16', 2),
    (128, 256, 100, 'f16', 2),
    (300, 384, 100, 'bf16', 2),
    (384, 512, 128, 'f16', 2),
    (300, 700, 100, 'f16', 2),
    (700, 300, 128, 'bf16', 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,R,prec,nsplit', CASES)
def test_lds_transpose_bit_identical(dev, N, C, R, prec, nsplit):
    """One and two iterations under NMFMU_STAGE_DMA_LDSTR against NMFMU_STAGE_DMA: W, H, both column-sum vectors and both P1
    images torch.equal.  The second iteration consumes factors whose P2 image was never refreshed."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(N, C, R, N + C + R)
    ref = _run(dev, V, W0, H0, prec, _capi.STAGE_DMA, nsplit)
    got = _run(dev, V, W0, H0, prec, _capi.STAGE_DMA_LDSTR, nsplit)
    _assert_same(got, ref, (N, C, R, prec, nsplit))


@pytest.mark.gpu
@pytest.mark.parametrize('nsplit', [1, 2])
def test_lds_transpose_bit_identical_regularised(dev, nsplit):
    from torchnmf_amd import _capi
    V, W0, H0 = _data(300, 384, 100, 5)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA, nsplit, l1=0.03, l2=0.05)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_LDSTR, nsplit, l1=0.03, l2=0.05)
    _assert_same(got, ref, ('regularised', nsplit))


@pytest.mark.gpu
def test_lds_transpose_bit_identical_f16r(dev):
    """The 3-byte-target instance (X loads inside the matrix segment)."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(300, 384, 100, 6)
    ref = _run(dev, V, W0, H0, 'f16r', _capi.STAGE_DMA, None)
    got = _run(dev, V, W0, H0, 'f16r', _capi.STAGE_DMA_LDSTR, None)
    _assert_same(got, ref, 'f16r')


@pytest.mark.gpu
def test_lds_transpose_bit_identical_riding_loss(dev):
    """The riding-loss instance: the W half-step of the first iteration carries a checkpoint's loss."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(300, 384, 100, 7)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA, None, riding=True)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_LDSTR, None, riding=True)
    _assert_same(got, ref, 'riding loss')


@pytest.mark.gpu
@pytest.mark.parametrize('prec,nsplit', [('f16', 1), ('bf16', 2)])
def test_lds_transpose_reads_no_p2_from_hbm(dev, prec, nsplit):
    """Both factors' transposed images filled with NaN bit patterns before stepping: same results as the clean run."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(300, 384, 100, 8)
    ref = _run(dev, V, W0, H0, prec, _capi.STAGE_DMA_LDSTR, nsplit)
    got = _run(dev, V, W0, H0, prec, _capi.STAGE_DMA_LDSTR, nsplit, poison=True)
    _assert_same(got, ref, ('poisoned', prec, nsplit))


@pytest.mark.gpu
def test_lds_transpose_is_the_default_and_is_refused_elsewhere(dev):
    """DenseMU picks the new stage where both half-steps run the ping-pong MU kernel at padded rank 128, and only there; the
    library refuses it for a step that has no such instance instead of falling back."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    V, W0, H0 = _data(300, 384, 100, 9)
    mk = lambda R, **kw: DenseMU(V.to(dev), W0[:, :R].clone().to(dev).contiguous(), H0[:, :R].clone().to(dev).contiguous(), **kw)
    assert mk(100, beta=1.0, precision='f16').step_w.struct.stage == _capi.STAGE_DMA_LDSTR
    assert mk(100, beta=1.0, precision='bf16').step_h.struct.stage == _capi.STAGE_DMA_LDSTR
    assert mk(64, beta=1.0, precision='f16').step_w.struct.stage == _capi.STAGE_DMA          # padded rank 64: no instance
    assert mk(100, beta=2.0, precision='f16').step_w.struct.stage == _capi.STAGE_DMA         # four-wave kernel
    assert mk(100, beta=1.0, precision='f16', block_rows=128).step_w.struct.stage == _capi.STAGE_DMA
    assert mk(100, beta=1.0, precision='f16', update_W=False).step_h.struct.stage == _capi.STAGE_DMA
    eng = mk(64, beta=1.0, precision='f16', stage=_capi.STAGE_DMA_LDSTR)
    with pytest.raises(NotImplementedError):
        eng.w_step()


@pytest.mark.gpu
@pytest.mark.parametrize('prec,tol', [('f16', 1e-4), ('bf16', 5e-3)])
def test_lds_transpose_parity(dev, prec, tol):
    """One iteration against the fp32 oracle, at the tolerance tests/test_gpu_parity.py::test_half_steps_f16 / _bf16 use."""
    from conftest import rel_err
    from oracle import mu_oracle as O
    from torchnmf_amd import _capi
    N, C, R = 300, 700, 128
    g = torch.Generator().manual_seed(N + R)
    V = torch.rand(N, C, generator=g)
    if prec == 'bf16':
        V = V.bfloat16().float()
    W0 = torch.randn(C, R, generator=g).abs()
    H0 = torch.randn(N, R, generator=g).abs()
    snap = _run(dev, V, W0, H0, prec, _capi.STAGE_DMA_LDSTR, None, iters=1)[0]
    Wr = O.nmf_w_step(V, W0, H0, 1, 1.0)
    Hr = O.nmf_h_step(V, Wr, H0, 1, 1.0)
    ew, eh = rel_err(snap[0], Wr), rel_err(snap[1], Hr)
    print(f'lds transpose parity {prec}: rel_err W={ew:.3e} H={eh:.3e}')
    assert ew < tol and eh < tol, (ew, eh)
