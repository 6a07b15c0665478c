"""The rank-128 software-pipelined MU kernel with its ratio stage re-spaced across both phases (csrc/nmfmu_sp128.h, RB > 0).

NMFMU_STAGE_DMA_SP128 runs the shipped placement of the ratio stage, NMFMU_STAGE_DMA_SP128_RB0 the same kernel with the whole
stage in phase A.  Only VALU placement differs -- same MFMA order and operands, same three instructions per element -- so
the two stages and the ping-pong kernel's one-image instance (NMFMU_STAGE_DMA_LDSTR) must agree BIT for bit: masters, column
sums and row-major images after each of 3 iterations.  The shapes walk the pipeline's ends: 4 tiles per workgroup = the
last group alone (the prologue issues tile 0's moved reciprocals, the last tile's phase B none), 8 and 12 = phase B(3) of a
looped group serves tile 0 of the next; a ragged block on the general epilogue; slabs with two splits.
"""
import pytest
import torch

from test_pp_lds_transpose import _assert_same, _data, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torchnmf_amd import _capi
    _capi.load()
    return torch.device('cuda:0')


CASES = [
    # N,   C,   R,   nsplit
    (256, 256, 128, 1),      # 4 tiles in both half-steps: the last group alone
    (512, 768, 128, 1),      # 8 and 12 tiles
    (300, 512, 100, 1),      # ragged block, padding ranks: the general epilogue
    (1024, 1024, 128, 2),    # two splits of 8 tiles: slabs + apply kernel
]


@pytest.mark.parametrize('N,C,R,nsplit', CASES)
def test_respaced_schedule_is_bit_identical(dev, N, C, R, nsplit):
    from torchnmf_amd import _capi
    V, W0, H0 = _data(N, C, R, N + C + R)
    got = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128, nsplit, iters=3)
    rb0 = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_SP128_RB0, nsplit, iters=3)
    ref = _run(dev, V, W0, H0, 'f16', _capi.STAGE_DMA_LDSTR, nsplit, iters=3)
    _assert_same(got, rb0, ('against the RB = 0 schedule', N, C, R, nsplit))
    _assert_same(got, ref, ('against the ping-pong kernel', N, C, R, nsplit))
