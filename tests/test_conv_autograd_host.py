"""Host side of nmfmu_conv_backward: the split rule as include/nmfmu.h states it (the rule of nmfmu_reconstruct_backward with
rows / contraction = B prod(lh) / C prod(taps) for grad_h and the reverse for grad_w), the scratch size, and argument checking
(no device work: every call here returns before a launch)."""
import ctypes
import itertools

import pytest

from torchnmf_amd import _capi


def rule(rows, contraction, rank):
    """include/nmfmu.h, nmfmu_reconstruct_backward: parts of one half's contraction."""
    tiles = -(-rows // 128) * -(-rank // 128)
    stages = -(-contraction // 32)
    n = max(1, min(-(-512 // tiles), stages // 4, 64))
    return -(-stages // -(-stages // n))


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def _arr(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def _ws(shape, want_h=1, want_w=1, splits=True):
    B, C, R, lh, taps = shape
    s = (ctypes.c_int * 2)(-7, -7)
    n = _capi.load().nmfmu_conv_backward_ws(B, C, R, len(lh), _arr(lh), _arr(taps), want_h, want_w, s if splits else None)
    return n, s[0], s[1]


# (B, C, R, lh, taps): a grid over the sizes, the shift axes and both rank tiles, plus the benchmark shapes and the test shapes
GRID = [(B, C, R, lh, taps)
        for B, C, R in itertools.product((1, 3), (1, 33, 1025), (1, 8, 33, 130))
        for lh, taps in (((1,), (1,)), ((50,), (5,)), ((40,), (45,)), ((7793,), (400,)), ((9, 14), (3, 4)), ((300, 41), (16, 8)),
                         ((4, 5, 6), (2, 3, 2)), ((30, 9, 80), (3, 1, 4)))]
GRID += [(2, 55, 7, (500,), (20,)), (1, 13, 130, (20, 35), (5, 10)), (1, 257, 33, (129,), (4,)), (5, 2, 300, (100000,), (1,))]


@pytest.mark.parametrize('shape', GRID)
def test_split_rule_and_scratch(shape):
    B, C, R, lh, taps = shape
    bj, ct = B * _prod(lh), C * _prod(taps)
    sh, sw = rule(bj, ct, R), rule(ct, bj, R)
    n, s0, s1 = _ws(shape)
    assert (s0, s1) == (sh, sw)
    n_h, n_w = (sh * bj * R if sh > 1 else 0), (sw * ct * R if sw > 1 else 0)
    assert n == n_h + n_w
    for contraction, parts in ((ct, sh), (bj, sw)):          # no empty part, only the last one short
        part_len = -(-(-(-contraction // 32)) // parts) * 32
        assert part_len % 32 == 0 and (parts - 1) * part_len < contraction <= parts * part_len
    assert _ws(shape, 1, 0) == (n_h, sh, 0)
    assert _ws(shape, 0, 1) == (n_w, 0, sw)
    assert _ws(shape, 0, 0, splits=False)[0] == 0
    assert _ws(shape) == (n, s0, s1)                          # nothing but the shape goes in


def test_only_the_flattened_sizes_count():
    """The rule sees B prod(lh), C prod(taps) and the rank: how they factor over batch, channels and the shift axes does not
    matter, nor does the number of axes."""
    a = _ws((2, 55, 7, (500,), (20,)))
    assert a == _ws((1, 11, 7, (10, 100), (5, 20))) == _ws((4, 1100, 7, (5, 5, 10), (1, 1, 1))) == _ws((1, 1100, 7, (1000,), (1,)))
    assert a[1] >= 3 and a[2] >= 3


def test_benchmark_shape_splits():
    from torchnmf_amd.nmf import conv_backward_splits
    # NMFD (1, 1025, 8192), rank 8, T = 400: grad_H has 61 row tiles -> 9 parts; grad_W has 3204 row tiles -> 1 part
    assert conv_backward_splits((1, 8, 7793), (1025, 8, 400)) == (9, 1)


def test_bad_arguments():
    lib = _capi.load()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    ws_ = lib.nmfmu_conv_backward_ws
    bw = lib.nmfmu_conv_backward
    lh, taps = _arr((50,)), _arr((5,))
    E = _capi.ERR_ARG
    # the workspace query
    assert ws_(2, 33, 7, 0, lh, taps, 1, 1, None) == E and ws_(2, 33, 7, 4, _arr((2, 2, 2, 2)), _arr((1, 1, 1, 1)), 1, 1, None) == E
    assert ws_(0, 33, 7, 1, lh, taps, 1, 1, None) == E and ws_(2, 0, 7, 1, lh, taps, 1, 1, None) == E
    assert ws_(2, 33, 0, 1, lh, taps, 1, 1, None) == E and ws_(2, 33, -1, 1, lh, taps, 1, 1, None) == E
    assert ws_(2, 33, 7, 1, _arr((0,)), taps, 1, 1, None) == E and ws_(2, 33, 7, 1, lh, _arr((-5,)), 1, 1, None) == E
    assert ws_(2, 33, 7, 2, _arr((9, 0)), _arr((3, 4)), 1, 1, None) == E
    assert ws_(2, 33, 7, 1, None, taps, 1, 1, None) == E and ws_(2, 33, 7, 1, lh, None, 1, 1, None) == E
    assert ws_(2, 33, 7, 1, lh, taps, 1, 1, None) == 0                                       # (the good call)
    # the launch entry: each of these returns before any device work
    assert bw(p, p, p, 2, 33, 7, 0, lh, taps, p, p, None, None) == E                         # ndim outside 1..3
    assert bw(p, p, p, 2, 33, 7, 4, _arr((2, 2, 2, 2)), _arr((1, 1, 1, 1)), p, p, None, None) == E
    assert bw(p, p, p, 0, 33, 7, 1, lh, taps, p, p, None, None) == E                         # non-positive sizes
    assert bw(p, p, p, 2, -3, 7, 1, lh, taps, p, p, None, None) == E
    assert bw(p, p, p, 2, 33, 0, 1, lh, taps, p, p, None, None) == E
    assert bw(p, p, p, 2, 33, 7, 1, _arr((0,)), taps, p, p, None, None) == E
    assert bw(p, p, p, 2, 33, 7, 1, lh, _arr((0,)), p, p, None, None) == E
    assert bw(None, p, p, 2, 33, 7, 1, lh, taps, p, p, None, None) == E                      # no gradient
    assert bw(p, p, p, 2, 33, 7, 1, lh, taps, None, None, None, None) == E                   # no output
    assert bw(p, None, p, 2, 33, 7, 1, lh, taps, p, None, None, None) == E                   # grad_h needs w
    assert bw(p, p, None, 2, 33, 7, 1, lh, taps, None, p, None, None) == E                   # grad_w needs h
    split = (2, 55, 7, (500,), (20,))
    assert _ws(split)[0] > 0 and _ws(split, 1, 0)[0] > 0 and _ws(split, 0, 1)[0] > 0
    for gh, gw in ((p, p), (p, None), (None, p)):                                            # split halves need the scratch
        assert bw(p, p, p, 2, 55, 7, 1, _arr((500,)), _arr((20,)), gh, gw, None, None) == E
    # sizes the kernel's 32-bit flattened axes do not hold
    assert ws_(1, 1 << 20, 8, 1, _arr((8,)), _arr((1 << 11,)), 1, 1, None) == E
