"""The software-pipelined four-wave MU kernel with 64 owner rows per wave (NMFMU_STAGE_DMA_SP128, csrc/nmfmu_sp128.h).

It keeps the ping-pong kernel's MFMA order per accumulator (rank steps ascending in GEMM1, (tt, m2) ascending within a tile
and tiles ascending in GEMM2), its ratio arithmetic and its epilogues, so at equal contraction splits everything it
computes must be BIT-identical to the ping-pong kernel's one-image instance (NMFMU_STAGE_DMA_LDSTR): fp32 masters, column
sums and row-major operand images after 1 and 3 iterations.  One case is held against the rounding-exact float64
emulation (tests/mu_emulation.py) per element, so that parity does not rest on the ping-pong kernel alone.

A workgroup's tiles come in groups of four (ring slot = tile & 3) with a straight-line last group: 4 tiles = the last group
alone, 8 = one looped group + the tail, 12 = several.  Both axes are padded to 256 rows, so a contraction of 256 columns
is 4 tiles, 512 is 8, 768 is 12; with nsplit 2 / 3 a contraction of 1024 / 1536 gives 8 tiles per workgroup.
"""
import numpy as np
import pytest
import torch

import mu_emulation as E
from test_gpu_emulated_parity import _check_images, _read_images
from test_pp_lds_transpose import _assert_same, _data, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


# W half-step: C owner rows, contraction over N; H half-step: N owner rows, contraction over C.
CASES = [
    # N,    C,    R,   nsplit   owner rows (W, H) / tiles per workgroup (W, H)
    (256, 256, 128, 1),      # 256, 256 / 4, 4: one workgroup, the last group alone
    (512, 768, 128, 1),      # 768, 512 / 8, 12
    (768, 512, 100, 1),      # 512, 768 / 12, 8; padding ranks masked in the fused apply
    (300, 512, 128, 1),      # 512, 300 (ragged block) / 8 (ragged contraction), 8
    (512, 300, 100, 1),      # 300 (ragged block, general epilogue), 512 / 8, 8 (ragged contraction)
    (1024, 1024, 128, 2),    # split: 1024, 1024 / 8, 8 -- slabs + apply kernel in both half-steps
    (1536, 1536, 100, 3),    # split in three: 8 tiles each
    (1024, 300, 100, 2),     # W: 300 owner rows, 8 tiles per split; H: 300 columns = 8 tiles over 2 splits of 4
]


@pytest.mark.parametrize('N,C,R,nsplit', CASES)
def test_sp128_bit_identical_to_the_ping_pong_kernel(dev, N, C, R, nsplit):
    from torchnmf_amd import _capi
    V, W0, H0 = _data(N, C, R, N + C + R)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_LDSTR, nsplit, iters=3)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128, nsplit, iters=3)
    _assert_same(got, ref, (N, C, R, nsplit))


@pytest.mark.parametrize('N,C,R,nsplit', [(300, 512, 100, 1), (512, 768, 128, 1), (1024, 1024, 128, 2)])
def test_sp128_bit_identical_regularised(dev, N, C, R, nsplit):
    """l1 + l2: the general form of the fused-apply epilogue (nsplit 1), the apply kernel behind the slabs (nsplit 2)."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(N, C, R, 11)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_LDSTR, nsplit, iters=3, l1=0.03, l2=0.05)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128, nsplit, iters=3, l1=0.03, l2=0.05)
    _assert_same(got, ref, ('regularised', N, C, R, nsplit))


def test_sp128_reads_no_p2_from_hbm(dev):
    """Both factors' transposed images filled with NaN bit patterns before stepping: same results as the clean run."""
    from torchnmf_amd import _capi
    V, W0, H0 = _data(300, 512, 100, 8)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128, 1)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128, 1, poison=True)
    _assert_same(got, ref, 'poisoned')


def test_sp128_is_refused_where_it_has_no_instance(dev):
    """bf16 operands, the 3-byte target and padded rank 64 have no instance: an error, not another kernel."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    V, W0, H0 = _data(300, 384, 100, 9)
    mk = lambda R, prec: DenseMU(V.to(dev), W0[:, :R].clone().to(dev).contiguous(), H0[:, :R].clone().to(dev).contiguous(), 1.0,
                                 precision=prec, stage=_capi.STAGE_DMA_SP128)
    for R, prec in ((100, 'bf16'), (100, 'f16r'), (64, 'f16')):
        eng = mk(R, prec)
        with pytest.raises(NotImplementedError):
            eng.w_step()


def test_sp128_is_the_default_where_both_launches_fill_the_chip(dev, monkeypatch):
    """DenseMU picks the stage for 'f16' at padded rank 128 when both half-steps launch at least one workgroup per CU and cut
    the contraction into whole groups of four tiles (4096 x 4096: 16 row blocks x 16 splits of 4 tiles), TORCHNMF_AMD_SP128=0
    keeps the ping-pong kernel, smaller problems and bf16 keep it anyway; the two choices give the same factors after two
    iterations."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    V, W0, H0 = _data(4096, 4096, 128, 3)

    def mk(prec='f16', n=4096):
        W, H = W0[:n].clone().to(dev), H0[:n].clone().to(dev)
        return DenseMU(V[:n, :n].contiguous().to(dev), W, H, 1.0, precision=prec), W, H
    eng, W, H = mk()
    fills = all((st.owner.rows_pad // 256) * st.nsplit >= ncu and (st.panel.rows_pad // 64) % (4 * st.nsplit) == 0
                for st in (eng.step_w, eng.step_h))
    want = _capi.STAGE_DMA_SP128 if fills else _capi.STAGE_DMA_LDSTR
    assert eng.step_w.struct.stage == want and eng.step_h.struct.stage == want
    if ncu <= 256:
        assert fills
    for _ in range(2):
        eng.w_step()
        eng.h_step()
    torch.cuda.synchronize()
    assert mk('bf16')[0].step_w.struct.stage == _capi.STAGE_DMA_LDSTR
    assert mk('f16', 512)[0].step_h.struct.stage == _capi.STAGE_DMA_LDSTR
    monkeypatch.setenv('TORCHNMF_AMD_SP128', '0')
    ref, Wr, Hr = mk()
    assert ref.step_w.struct.stage == _capi.STAGE_DMA_LDSTR and ref.step_h.struct.stage == _capi.STAGE_DMA_LDSTR
    for _ in range(2):
        ref.w_step()
        ref.h_step()
    torch.cuda.synchronize()
    assert torch.equal(W, Wr) and torch.equal(H, Hr) and torch.isfinite(W).all() and torch.isfinite(H).all()


def test_sp128_per_element_against_the_emulation(dev):
    """256 x 256, rank 128: numerator slabs (slab epilogue) and the new masters (fused-apply epilogue) of both half-steps per
    element within mu_emulation.TOL['f16'] of the float64 emulation that rounds where the kernels round; the row-major
    images bit-exact the rounding of the new masters."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    N = C = 256
    R = 128
    V, W0, H0 = _data(N, C, R, 21)
    W, H = W0.clone().to(dev), H0.clone().to(dev)
    eng = DenseMU(V.to(dev), W, H, 1.0, precision='f16', stage=_capi.STAGE_DMA_SP128)
    tol = E.TOL['f16']
    for which, st in (('w', eng.step_w), ('h', eng.step_h)):
        assert st.block_rows == 256 and st.nsplit == 1 and st.struct.stage == _capi.STAGE_DMA_SP128
        owner, panel = st.owner, st.panel
        X = (V.t() if which == 'w' else V).numpy()
        A_hi, _ = _read_images(owner, st.r_pad, 'f16')
        B_hi, _ = _read_images(panel, st.r_pad, 'f16')
        cs_o, cs_p = owner.colsum.cpu().numpy(), panel.colsum.cpu().numpy()
        theta = owner.f.cpu().numpy().astype(np.float64)
        em = E.half_step(X, None, None, 1.0, 'f16', M=owner.rows, K=panel.rows, cs_owner=cs_o, cs_panel=cs_p,
                         A_img=(A_hi[:owner.rows, :R], None), B_img=(B_hi[:panel.rows, :R], None))
        st.slab_num.fill_(float('nan'))
        eng._partial(st, which)
        torch.cuda.synchronize()
        num = st.slab_num.view(1, owner.rows_pad, st.r_pad).double().sum(0).cpu().numpy()[:owner.rows, :R]
        e_num = float(E.elem_err(num, em['num'], em['num_amb']).max())
        eng.status.zero_()
        (eng.w_step if which == 'w' else eng.h_step)()
        torch.cuda.synchronize()
        new = owner.f.cpu().numpy().astype(np.float64)
        ref = E.apply(theta, em['num'], em['den'], 1.0, st.struct.gamma, 0.0, 0.0, kl_den=cs_p)
        allow = E.apply_allowance(ref, em['num'], em['den'], em['num_amb'], em['den_amb'], 1.0, st.struct.gamma, l1=0.0, l2=0.0,
                                  theta=theta)
        e_new = float(E.elem_err(new, ref, allow).max())
        print(f'sp128 emulated parity {which}: num {e_num:.3e} master {e_new:.3e} (tol {tol:.1e})')
        assert e_num <= tol and e_new <= tol, (which, e_num, e_new)
        assert _check_images(owner, st.r_pad, 'f16', True) == {'p1_hi': 0}
        assert int(eng.status.item()) & 1 == 0
