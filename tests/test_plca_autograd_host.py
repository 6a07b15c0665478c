"""Host side of nmfmu_plca_backward / nmfmu_conv_plca_backward: the half-selection rule, the finishing kernel's workgroup rule
and the scratch layout as include/nmfmu.h states them, mirrored here in Python as pure functions of the shape, and argument
checking (no device work: every call here returns before a launch)."""
import ctypes
import itertools

import pytest

from torchnmf_amd import _capi

E = _capi.ERR_ARG
WANTS = list(itertools.product((0, 1), repeat=3))            # (want_h, want_w, want_z)


def split_rule(rows, contraction, rank):
    """include/nmfmu.h, nmfmu_reconstruct_backward: parts of one half's contraction."""
    tiles = -(-rows // 128) * -(-rank // 128)
    stages = -(-contraction // 32)
    n = max(1, min(-(-512 // tiles), stages // 4, 64))
    return -(-stages // -(-stages // n))


def finish_grid(outer, rank, inner):
    """include/nmfmu.h, nmfmu_plca_backward: (nbo, chunk, nseg, seg) of the finishing kernel over [outer][rank][inner]."""
    want = min(2048, -(-(outer * rank * inner) // 8192))
    chunk = -(-outer // min(want, outer))
    nbo = -(-outer // chunk)
    if inner == 1:
        return nbo, chunk, 1, 1
    ns = max(1, min(-(-want // nbo), inner // 1024))
    seg = -(-(-(-inner // ns)) // 4) * 4
    return nbo, chunk, -(-inner // seg), seg


def plan(want_h, want_w, want_z, parts_h, parts_w, h_view, w_view, rank):
    """(floats of ws, info[5]) by the rules of include/nmfmu.h; *_view = (outer, inner) of that half's output."""
    run_h = bool(want_h)
    z_h = bool(want_z and want_h and not want_w)
    run_w = bool(want_w or (want_z and not want_h))
    info, n = [0, 0, 0, 0, 0], 0
    for idx, run, parts, (outer, inner), wanted in ((0, run_h, parts_h, h_view, want_h), (1, run_w, parts_w, w_view, want_w)):
        if run:
            nbo, _, nseg, _ = finish_grid(outer, rank, inner)
            info[idx], info[2 + idx] = parts, nbo * nseg
            if parts > 1 or not wanted:
                n += -(-(parts * outer * rank * inner) // 4) * 4     # each slab region is rounded up to 4 floats
    if want_z:
        info[4] = 1 if z_h else 2
        n += info[2 if z_h else 3] * rank
    return n, info


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def _arr(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def _dense_ws(m, k, r, wants, with_info=True):
    info = (ctypes.c_int * 5)(*([-7] * 5))
    n = _capi.load().nmfmu_plca_backward_ws(m, k, r, *wants, info if with_info else None)
    return n, list(info)


def _conv_ws(shape, wants, with_info=True):
    B, C, R, lh, taps = shape
    info = (ctypes.c_int * 5)(*([-7] * 5))
    n = _capi.load().nmfmu_conv_plca_backward_ws(B, C, R, len(lh), _arr(lh), _arr(taps), *wants, info if with_info else None)
    return n, list(info)


DENSE = [(m, k, r) for m, k in ((1, 1), (33, 130), (300, 257), (200, 90), (1000, 1100), (700, 650), (4096, 65536), (5, 100000))
         for r in (1, 7, 33, 128, 130, 256, 1030)]
CONV = [(B, C, R, lh, taps)
        for B, C, R in itertools.product((1, 3), (1, 33, 1025), (1, 8, 33, 130))
        for lh, taps in (((1,), (1,)), ((50,), (5,)), ((40,), (45,)), ((7793,), (400,)), ((9, 14), (3, 4)), ((300, 41), (16, 8)),
                         ((30, 9, 80), (3, 1, 4)))]
CONV += [(2, 55, 7, (500,), (20,)), (1, 13, 130, (20, 35), (5, 10)), (2, 33, 2, (3, 9, 8), (3, 1, 4)), (5, 2, 300, (100000,), (1,))]


@pytest.mark.parametrize('shape', DENSE)
def test_dense_plan(shape):
    m, k, r = shape
    ph, pw = split_rule(m, k, r), split_rule(k, m, r)
    for wants in WANTS:
        got = _dense_ws(m, k, r, wants)
        assert got == plan(*wants, ph, pw, (m, 1), (k, 1), r), (shape, wants)
        assert _dense_ws(m, k, r, wants, with_info=False)[0] == got[0]
        assert _dense_ws(m, k, r, wants) == got                  # nothing but the shape and the wanted outputs goes in


@pytest.mark.parametrize('shape', CONV)
def test_conv_plan(shape):
    B, C, R, lh, taps = shape
    bj, ct = B * _prod(lh), C * _prod(taps)
    ph, pw = split_rule(bj, ct, R), split_rule(ct, bj, R)
    for wants in WANTS:
        got = _conv_ws(shape, wants)
        assert got == plan(*wants, ph, pw, (B, _prod(lh)), (C, _prod(taps)), R), (shape, wants)
        assert _conv_ws(shape, wants, with_info=False)[0] == got[0]


def test_half_selection():
    """grad_Z from the W half when that half runs anyway or no factor gradient is wanted; from the H half only with grad_h and
    without grad_w; a half runs only when its gradient is wanted or it feeds grad_Z."""
    expect = {(0, 0, 0): (0, 0, 0), (0, 0, 1): (0, 1, 2), (0, 1, 0): (0, 1, 0), (0, 1, 1): (0, 1, 2),
              (1, 0, 0): (1, 0, 0), (1, 0, 1): (1, 0, 1), (1, 1, 0): (1, 1, 0), (1, 1, 1): (1, 1, 2)}
    for wants, (run_h, run_w, z_half) in expect.items():
        for n, info in (_dense_ws(300, 257, 33, wants), _conv_ws((2, 33, 7, (50,), (5,)), wants)):
            assert (info[0] > 0, info[1] > 0, info[4]) == (bool(run_h), bool(run_w), z_half), wants
            assert (info[2] > 0, info[3] > 0) == (bool(run_h), bool(run_w))
    assert _dense_ws(300, 257, 33, (0, 0, 0))[0] == 0


@pytest.mark.parametrize('view', [(1, 1, 1), (33, 7, 1), (4096, 128, 1), (65536, 128, 1), (1 << 30, 1, 1), (7, 1 << 20, 1),
                                  (1, 8, 7793), (1, 8, 8192), (1025, 8, 400), (3, 130, 5), (2, 2, 216), (1, 1, 1 << 30),
                                  (13, 130, 50), (1, 3, 2049)])
def test_finish_grid_covers_the_output(view):
    outer, rank, inner = view
    nbo, chunk, nseg, seg = finish_grid(outer, rank, inner)
    assert 1 <= nbo <= 2048 and 1 <= nseg <= 2048
    assert (nbo - 1) * chunk < outer <= nbo * chunk               # no empty workgroup, only the last chunk short
    if inner > 1:
        assert seg % 4 == 0 and (nseg - 1) * seg < inner <= nseg * seg
        assert nseg == 1 or seg >= 1024
    assert nbo * nseg == 1 or (outer * rank * inner) / (nbo * nseg) >= 2048   # a workgroup is not starved


def test_benchmark_shapes():
    # PLCA 4096 x 65536, rank 128: grad_h in 16 parts, grad_w in one; 64 and 1024 finishing workgroups
    n, info = _dense_ws(4096, 65536, 128, (1, 1, 1))
    assert info == [16, 1, 64, 1024, 2]
    assert n == 16 * 4096 * 128 + 1024 * 128
    assert _dense_ws(33, 130, 7, (0, 0, 1))[0] == 912 + 1 * 7      # a raw product of 130 x 7 = 910 floats, rounded up
    # SIPLCA (1, 1025, 8192), rank 8, T = 400: the split of the NMFD backward; H's 7793-long lines are cut into segments
    n, info = _conv_ws((1, 1025, 8, (7793,), (400,)), (1, 1, 1))
    assert info[:2] == [9, 1] and info[4] == 2
    assert info[2] == finish_grid(1, 8, 7793)[2] > 1


def test_bad_arguments():
    lib = _capi.load()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    # dense: the workspace query
    ws_ = lib.nmfmu_plca_backward_ws
    for bad in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (-1, 5, 3), (5, -2, 3), (5, 5, -3)):
        assert ws_(*bad, 1, 1, 1, None) == E
    assert ws_(5, 5, 3, 1, 1, 1, None) == 1 * 3                   # (the good call: one workgroup's partial sums)
    # dense: the launch entry; each of these returns before any device work
    bw = lib.nmfmu_plca_backward
    assert bw(None, 5, 5, 5, p, p, p, 3, p, p, p, p, None) == E   # NULL inputs
    assert bw(p, 5, 5, 5, None, p, p, 3, p, p, p, p, None) == E
    assert bw(p, 5, 5, 5, p, None, p, 3, p, p, p, p, None) == E
    assert bw(p, 5, 5, 5, p, p, None, 3, p, p, p, p, None) == E
    assert bw(p, 5, 0, 5, p, p, p, 3, p, p, p, p, None) == E      # non-positive sizes
    assert bw(p, 5, 5, -1, p, p, p, 3, p, p, p, p, None) == E
    assert bw(p, 5, 5, 5, p, p, p, 0, p, p, p, p, None) == E
    assert bw(p, 4, 5, 5, p, p, p, 3, p, p, p, p, None) == E      # ld < k
    assert bw(p, 5, 5, 5, p, p, p, 3, None, None, None, p, None) == E      # no output
    for outs in ((p, p, p), (None, None, p), (p, None, p), (None, p, p)):  # grad_z always needs scratch
        assert bw(p, 5, 5, 5, p, p, p, 3, *outs, None, None) == E
    for outs in ((p, None, None), (None, p, None), (p, p, None)):          # split halves need the scratch
        assert _dense_ws(1000, 1100, 7, tuple(int(o is not None) for o in outs))[0] > 0
        assert bw(p, 1100, 1000, 1100, p, p, p, 7, *outs, None, None) == E
    # conv: the workspace query
    cws = lib.nmfmu_conv_plca_backward_ws
    lh, taps = _arr((50,)), _arr((5,))
    assert cws(2, 33, 7, 0, lh, taps, 1, 1, 1, None) == E and cws(2, 33, 7, 4, _arr((2, 2, 2, 2)), _arr((1, 1, 1, 1)), 1, 1, 1, None) == E
    assert cws(0, 33, 7, 1, lh, taps, 1, 1, 1, None) == E and cws(2, 0, 7, 1, lh, taps, 1, 1, 1, None) == E
    assert cws(2, 33, 0, 1, lh, taps, 1, 1, 1, None) == E and cws(2, 33, -1, 1, lh, taps, 1, 1, 1, None) == E
    assert cws(2, 33, 7, 1, _arr((0,)), taps, 1, 1, 1, None) == E and cws(2, 33, 7, 1, lh, _arr((-5,)), 1, 1, 1, None) == E
    assert cws(2, 33, 7, 1, None, taps, 1, 1, 1, None) == E and cws(2, 33, 7, 1, lh, None, 1, 1, 1, None) == E
    assert cws(1, 1 << 20, 8, 1, _arr((8,)), _arr((1 << 11,)), 1, 1, 1, None) == E           # flattened axis above 2^30
    assert cws((1 << 30) + 1, 2, 8, 1, _arr((1,)), _arr((1,)), 1, 1, 1, None) == E
    info = (ctypes.c_int * 5)(*([-7] * 5))
    assert cws(0, 33, 7, 1, lh, taps, 1, 1, 1, info) == E and list(info) == [-7] * 5         # a rejected call touches nothing
    assert cws(2, 33, 7, 1, lh, taps, 1, 1, 0, None) == 0                                     # (the good call)
    # conv: the launch entry
    cb = lib.nmfmu_conv_plca_backward
    good = (2, 33, 7, 1, lh, taps)
    assert cb(None, p, p, p, *good, p, p, p, p, None) == E
    assert cb(p, None, p, p, *good, p, p, p, p, None) == E
    assert cb(p, p, None, p, *good, p, p, p, p, None) == E
    assert cb(p, p, p, None, *good, p, p, p, p, None) == E
    assert cb(p, p, p, p, *good, None, None, None, p, None) == E                             # no output
    assert cb(p, p, p, p, 2, 33, 7, 0, lh, taps, p, p, p, p, None) == E                       # ndim outside 1..3
    assert cb(p, p, p, p, 2, 33, 7, 4, _arr((2, 2, 2, 2)), _arr((1, 1, 1, 1)), p, p, p, p, None) == E
    assert cb(p, p, p, p, 0, 33, 7, 1, lh, taps, p, p, p, p, None) == E
    assert cb(p, p, p, p, 2, -3, 7, 1, lh, taps, p, p, p, p, None) == E
    assert cb(p, p, p, p, 2, 33, 0, 1, lh, taps, p, p, p, p, None) == E
    assert cb(p, p, p, p, 2, 33, 7, 1, _arr((0,)), taps, p, p, p, p, None) == E
    assert cb(p, p, p, p, 2, 33, 7, 1, lh, _arr((0,)), p, p, p, p, None) == E
    assert cb(p, p, p, p, 2, 33, 7, 1, None, taps, p, p, p, p, None) == E
    assert cb(p, p, p, p, 1, 1 << 20, 8, 1, _arr((8,)), _arr((1 << 11,)), p, p, p, p, None) == E
    for outs in ((p, p, p), (None, None, p), (p, None, None), (None, p, None)):               # scratch needed and missing
        wants = tuple(int(o is not None) for o in outs)
        assert _conv_ws((2, 55, 7, (500,), (20,)), wants)[0] > 0
        assert cb(p, p, p, p, 2, 55, 7, 1, _arr((500,)), _arr((20,)), *outs, None, None) == E


@pytest.mark.parametrize('tag', ['plca', 'siplca', 'siplca2', 'siplca3'])
def test_float64_formulas_agree_with_the_golden_gradients(tag):
    """The float64 formulas the GPU tests compare against (plca_autograd_reference.py) reproduce the gradients the reference's
    own modules gave in float64 (tests/golden/g18_plca_autograd.npz) to 1e-12 relative -- from either half for grad_Z."""
    import torch
    from conftest import load_golden
    from plca_autograd_reference import reference
    d = load_golden('g18_plca_autograd')
    T = lambda k: torch.from_numpy(d[f'{tag}_{k}'])
    ref = reference(T('G'), T('H0'), T('W0'), T('Z0'))
    for mine, theirs in (('gH', 'gH'), ('gW', 'gW'), ('gZ', 'gZ'), ('gZ_from_H', 'gZ')):
        want = T(theirs)
        assert want.dtype == torch.float64 and ref[mine].shape == want.shape
        assert float((ref[mine] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (tag, mine)
    assert all(bool((ref[b] >= 0).all()) for b in ('bH', 'bW', 'bZ'))
