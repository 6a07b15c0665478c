"""Host side of the autograd entries: the split rule of nmfmu_reconstruct_backward as include/nmfmu.h states it, the scratch
size, and argument checking (no device work: every call here returns before a launch)."""
import ctypes

import pytest

from torchnmf_amd import _capi


def rule(rows, contraction, rank):
    """include/nmfmu.h, nmfmu_reconstruct_backward: parts of one half's contraction."""
    tiles = -(-rows // 128) * -(-rank // 128)
    stages = -(-contraction // 32)
    n = max(1, min(-(-512 // tiles), stages // 4, 64))
    return -(-stages // -(-stages // n))


SHAPES = [(1, 1, 1), (33, 130, 7), (128, 128, 32), (300, 257, 33), (513, 1000, 128), (200, 90, 256), (1000, 1100, 7),
          (700, 650, 130), (4096, 65536, 128), (65536, 4096, 128), (5, 100000, 300), (100000, 5, 3)]


@pytest.mark.parametrize('shape', SHAPES)
def test_split_rule_and_scratch(shape):
    lib = _capi.load()
    m, k, rank = shape
    s = (ctypes.c_int * 2)()
    n = lib.nmfmu_reconstruct_backward_ws(m, k, rank, 1, 1, s)
    so, sp = rule(m, k, rank), rule(k, m, rank)
    assert (s[0], s[1]) == (so, sp)
    assert n == (so * m * rank if so > 1 else 0) + (sp * k * rank if sp > 1 else 0)
    for contraction, parts in ((k, so), (m, sp)):             # no empty part
        part_len = -(-(-(-contraction // 32)) // parts) * 32
        assert (parts - 1) * part_len < contraction <= parts * part_len
    assert lib.nmfmu_reconstruct_backward_ws(m, k, rank, 1, 0, s) == (so * m * rank if so > 1 else 0) and s[1] == 0
    assert lib.nmfmu_reconstruct_backward_ws(m, k, rank, 0, 1, s) == (sp * k * rank if sp > 1 else 0) and s[0] == 0
    assert lib.nmfmu_reconstruct_backward_ws(m, k, rank, 0, 0, None) == 0


def test_flagship_shape_fills_the_machine():
    from torchnmf_amd.nmf import reconstruct_backward_splits
    assert reconstruct_backward_splits(4096, 65536, 128) == (16, 1)      # 32 tiles x 16 parts / 512 tiles x 1


def test_bad_arguments():
    lib = _capi.load()
    assert lib.nmfmu_reconstruct_backward_ws(0, 5, 5, 1, 1, None) == _capi.ERR_ARG
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    bw = lib.nmfmu_reconstruct_backward
    assert bw(None, 5, 4, 5, p, p, 3, p, p, None, None) == _capi.ERR_ARG          # no gradient
    assert bw(p, 4, 4, 5, p, p, 3, p, p, None, None) == _capi.ERR_ARG             # ld < k
    assert bw(p, 5, 0, 5, p, p, 3, p, p, None, None) == _capi.ERR_ARG
    assert bw(p, 5, 4, 5, p, None, 3, p, None, None, None) == _capi.ERR_ARG       # grad_owner needs the panel
    assert bw(p, 5, 4, 5, None, p, 3, None, p, None, None) == _capi.ERR_ARG       # grad_panel needs the owner
    assert bw(p, 1100, 1000, 1100, p, p, 7, p, p, None, None) == _capi.ERR_ARG    # split halves need the scratch
    assert lib.nmfmu_beta_div_grad(None, p, 4, 1.0, p, p, None) == _capi.ERR_ARG
    assert lib.nmfmu_beta_div_grad(p, p, 4, 1.0, None, p, None) == _capi.ERR_ARG
    assert lib.nmfmu_beta_div_grad(p, p, -1, 1.0, p, p, None) == _capi.ERR_ARG
