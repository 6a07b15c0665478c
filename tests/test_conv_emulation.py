"""tests/conv_emulation.py on the CPU: the unrounded emulation IS the oracle's algorithm, unfold and fold are adjoint, the
per-element checks of tests/test_gpu_conv_emulated_parity.py catch seeded faults that the whole-factor norm of the older GPU
tests lets through, the case list reaches the control flow it claims as far as the host functions can tell and holds a case
for every plan the default switches reach on a grid of small shapes, and 'f16' is admitted on window tables only."""
import numpy as np
import pytest
import torch

from conftest import rel_err
import conv_emulation as CE
import mu_emulation as E
from oracle import mu_oracle as O

OLD_BAR = {'bf16x3': 1e-4, 'f16': 6e-4, 'bf16': 2e-2}     # rel_err bars of the norm-based NMFD tests (test_gpu_parity.py)

SHAPES = [(2, 7, (20,), 3, (4,)), (1, 9, (17,), 2, (1,)), (2, 5, (6, 9), 2, (2, 3)), (2, 4, (4, 5, 6), 2, (2, 2, 3))]


def _problem(B, C, ls, R, ts, seed=1):
    g = torch.Generator().manual_seed(seed)
    lhs = tuple(l - t + 1 for l, t in zip(ls, ts))
    V = (torch.rand(B, C, *ls, generator=g) + 1e-3).double()
    W = torch.randn(C, R, *ts, generator=g).abs().double()
    H = torch.randn(B, R, *lhs, generator=g).abs().double()
    return V, W, H


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s[2]))
@pytest.mark.parametrize('regs', [(0.0, 0.0), (0.05, 0.05)], ids=['plain', 'reg'])
@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 1.5, 2, 3])
def test_unrounded_emulation_is_the_oracle(shape, regs, beta):
    V, W, H = _problem(*shape)
    l1, l2 = regs
    gam = O.gamma_of(beta)
    nd1 = len(shape[2]) == 1
    w = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3', l1, l2, rounding=False)['new']
    h = CE.h_half_step(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3', l1, l2, rounding=False)['new']
    refs = [(O.convnd_w_step(V, W, H, beta, gam, l1, l2), O.convnd_h_step(V, W, H, beta, gam, l1, l2))]
    if nd1:
        refs.append((O.nmfd_w_step(V, W, H, beta, gam, l1, l2), O.nmfd_h_step(V, W, H, beta, gam, l1, l2)))
    for wr, hr in refs:
        assert np.abs(w - wr.numpy()).max() <= 1e-12 * float(wr.abs().max())
        assert np.abs(h - hr.numpy()).max() <= 1e-12 * float(hr.abs().max())
    want = float(O.beta_div(O.convnd_reconstruct(H, W), V, beta))
    assert CE.loss(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3', rounding=False)[0] == pytest.approx(want, rel=1e-10)
    assert CE.gamma_of(beta) == gam


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s[2]))
def test_unfold_and_fold_are_adjoint_and_reconstruct(shape):
    B, C, ls, R, ts = shape
    V, W, H = _problem(*shape)
    Hu = CE.unfold(H.numpy(), ts)
    Y = np.random.default_rng(3).standard_normal(Hu.shape)
    lhs = tuple(H.shape[2:])
    assert float((Hu * Y).sum()) == pytest.approx(float((H.numpy() * CE.fold(Y, B, R, lhs, ts)).sum()), rel=1e-12)
    rec = CE.w_matrix(W.numpy()) @ Hu.T                              # [c][(b, l)]
    assert np.abs(rec - CE.target_w(O.convnd_reconstruct(H, W).numpy())).max() <= 1e-12 * np.abs(rec).max()
    if len(ls) == 1:
        assert np.abs(rec - CE.target_w(O.nmfd_reconstruct(H, W).numpy())).max() <= 1e-12 * np.abs(rec).max()
    assert ((Hu != 0).sum(axis=1) <= R * int(np.prod(ts))).all() and Hu.shape == (B * int(np.prod(ls)), R * int(np.prod(ts)))


@pytest.mark.parametrize('prec,beta', [('bf16x3', 1), ('bf16', 0.5), ('f16', 1), ('bf16x3', 0), ('bf16', 3)])
def test_conv_half_step_is_the_dense_one_on_the_unfolded_matrices(prec, beta):
    """... given the stored target: mu_emulation.half_step(x_stored=) with the fp32 target reproduces the conv W half-step
    (beta != 2: there the dense 16-bit modes use the stored word as the operand).  Its default is unchanged."""
    V, W, H = (x.float() for x in _problem(2, 7, (20,), 3, (4,)))
    em = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), beta, prec)
    ops = em['ops']
    Xw = CE.target_w(V.numpy())
    d = E.half_step(Xw, None, None, beta, prec, A_img=ops['Wm'], B_img=ops['Hu'], x_stored=Xw)
    assert np.array_equal(d['num'], em['num']) and (d['den'] is None or np.array_equal(d['den'], em['den']))
    assert np.array_equal(np.broadcast_to(d['num_amb'], d['num'].shape), np.broadcast_to(em['num_amb'], d['num'].shape))
    a = E.half_step(Xw, None, None, beta, prec, A_img=ops['Wm'], B_img=ops['Hu'])
    b = E.half_step(Xw, None, None, beta, prec, A_img=ops['Wm'], B_img=ops['Hu'], x_stored=E.stored_target(Xw, prec))
    assert np.array_equal(a['num'], b['num'])
    if prec != 'bf16x3':
        assert not np.array_equal(a['num'], d['num'])                # the dense modes round the target, this engine does not


# ---- seeded faults ----------------------------------------------------------------------------------------------------
def _fault_problem(B=1, C=70, L=136, R=3, T=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    V = torch.rand(B, C, L, generator=g) + 1e-3
    W = torch.randn(C, R, T, generator=g).abs()
    H = torch.randn(B, R, L - T + 1, generator=g).abs()
    return V, W, H


def _judge(which, prec, beta, V, W, H, faulty, good, pad=None):
    """(per-element check passes, rel_err of the faulty factor against the unrounded oracle)."""
    C, BL = W.shape[0], V.shape[0] * V.shape[2]
    p128 = lambda n: -(-n // 128) * 128
    rp, cp = (p128(C), p128(BL)) if which == 'w' else (p128(BL), p128(C))
    got = CE.as_kernel_result(faulty, prec, which, rp, cp)
    if pad is not None:
        pad(got)
    ok, fig = CE.check_half_step(got, good, prec, beta, which)
    ok0, _ = CE.check_half_step(CE.as_kernel_result(good, prec, which, rp, cp), good, prec, beta, which)
    assert ok0                                                      # the unfaulted emulation passes its own check
    step = O.nmfd_w_step if which == 'w' else O.nmfd_h_step
    ref = step(V.double(), W.double(), H.double(), beta, O.gamma_of(beta))
    return ok, rel_err(faulty['new'], ref), fig


def _trunc(prec):
    def rr(G, split):
        t = torch.from_numpy(np.asarray(G, dtype=np.float64).astype(np.float32).ravel().copy())
        bits = t.view(torch.int32)
        if prec == 'f16':       # drop the 13 fraction bits fp16 does not keep (normal range; the test's ratios are)
            hi = (bits & ~0x1fff).view(torch.float32).clamp(max=E.F16_MAX).double().numpy()
        else:
            hi = (bits & ~0xffff).view(torch.float32).double().numpy()
        return [hi.reshape(np.shape(G))]
    return rr


def test_fault_hu_shifted_one_frame_in_one_k_chunk():
    V, W, H = _fault_problem()
    good = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3')
    hu = [p.copy() for p in good['ops']['Hu']]
    for p in hu:
        p[:, 8:16] = np.roll(p[:, 8:16], 1, axis=0)                 # the chunk (r = 0, t = 8..15) one frame late
    bad = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3', Hu_num=tuple(hu))
    ok, old, fig = _judge('w', 'bf16x3', 1, V, W, H, bad, good)
    assert not ok and fig['num'] > 1e-3 and fig['master'] > 1e-3


@pytest.mark.parametrize('prec', ['bf16', 'f16'])
def test_fault_ratio_plane_truncated_passes_the_old_bar(prec):
    V, W, H = _fault_problem()
    for which, fn in (('w', CE.w_half_step), ('h', CE.h_half_step)):
        good = fn(V.numpy(), W.numpy(), H.numpy(), 1, prec)
        bad = fn(V.numpy(), W.numpy(), H.numpy(), 1, prec, ratio_round=_trunc(prec))
        ok, old, fig = _judge(which, prec, 1, V, W, H, bad, good)
        assert not ok and fig['ratio']['gn']['bad'] > 0.3 * good['ratio']['gn'].size and fig['master'] > E.TOL[prec]
        assert old < OLD_BAR[prec], old


def test_fault_fold_drops_the_last_tap_of_one_rank_passes_the_old_bar():
    V, W, H = _fault_problem(L=264, T=136)
    taps = lambda r: [(t,) for t in range(136 if r != 1 else 135)]
    good = CE.h_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16')
    bad = CE.h_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16', taps=taps)
    ok, old, fig = _judge('h', 'bf16', 1, V, W, H, bad, good)
    assert not ok and fig['master'] > 1e-3 and fig['num'] > 1e-3
    assert old < OLD_BAR['bf16'], old


def test_fault_ragged_channel_from_rounded_operands_passes_the_old_bar():
    """The direct-summation kernel rounding W and H to bf16 in the split mode (its single-plane behaviour)."""
    V, W, H = _fault_problem(C=129)
    for which, fn in (('w', CE.w_half_step), ('h', CE.h_half_step)):
        good = fn(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3', exact_channels=(128,))
        ops = good['ops']
        rt = CE.ratio(CE.target_w(V.numpy()), dict(ops, Wx=ops['Wm'][0], Hux=ops['Hu'][0]), 1, 'bf16x3', (128,))
        nm = CE.numerators_w(rt, ops) if which == 'w' else CE.numerators_h(rt, ops, 1)
        new, _ = CE.update(W.numpy() if which == 'w' else H.numpy(), nm, H.numpy() if which == 'w' else W.numpy(), 1, 1.0)
        bad = dict(nm, ratio=rt, new=new)
        ok, old, fig = _judge(which, 'bf16x3', 1, V, W, H, bad, good)
        # (136 elements of one channel: the hi word moves where the 2^-9 error crosses a rounding point, the lo word nearly always)
        assert not ok and fig['ratio']['gn']['bad'] > 0 and fig['ratio']['gn_lo']['bad'] > 50, fig['ratio']
        assert old < OLD_BAR['bf16x3'], old


def test_fault_kl_denominator_from_the_previous_h():
    V, W, H = _fault_problem()
    Hn = CE.h_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3')['new'].astype(np.float32)
    good = CE.w_half_step(V.numpy(), W.numpy(), Hn, 1, 'bf16x3')
    bad = CE.w_half_step(V.numpy(), W.numpy(), Hn, 1, 'bf16x3', kl_den=H.double().numpy().sum(axis=(0, 2)))
    ok, old, fig = _judge('w', 'bf16x3', 1, V, W, torch.from_numpy(Hn), bad, good)
    assert not ok and fig['num'] == 0.0 and fig['master'] > 1e-3     # only the update is wrong


@pytest.mark.parametrize('beta', [1, 0.5])
def test_fault_nonzero_padding_column_of_a_ratio_plane_passes_the_old_bar(beta):
    V, W, H = _fault_problem()
    good = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16')

    def pad(got):
        hi = got['planes']['gn'][0]
        hi[5, V.shape[2] + 3] = CE.nan_word('bf16') if beta != 1 else CE.encode(np.array([1.0]), 'bf16')[0]
    ok, old, fig = _judge('w', 'bf16', beta, V, W, H, good, good, pad=pad)
    assert not ok and fig['ratio']['gn']['pad_bad'] == 1 and fig['master'] == 0.0
    assert old < OLD_BAR['bf16'], old
    # a plane the engine zero-initialises and the GEMM leaves alone: any word there is a fault, finite or not
    got = CE.as_kernel_result(good, 'bf16', 'w', 128, 256)
    got['planes']['gn'][0][100, 7] = CE.encode(np.array([1.0]), 'bf16')[0]
    assert not CE.check_half_step(got, good, 'bf16', beta, 'w', gemm_rows=64)[0]


def test_fault_one_tile_of_w_not_updated():
    V, W, H = _fault_problem(C=200)
    good = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3')
    new = good['new'].reshape(200, -1).copy()
    new[64:128, 0:48][:, :] = W.numpy().reshape(200, -1)[64:128, 0:48]
    bad = dict(good, new=new.reshape(good['new'].shape))
    ok, old, fig = _judge('w', 'bf16x3', 1, V, W, H, bad, good)
    assert not ok and fig['num'] == 0.0 and fig['master'] > 1e-2


def test_fault_a_zero_that_does_not_stay_zero():
    V, W, H = _fault_problem()
    W[3] = 0.0
    good = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3')
    new = good['new'].copy()
    new[3, 1, 2] = 1e-30
    assert not _judge('w', 'bf16x3', 1, V, W, H, dict(good, new=new), good)[0]


def test_fp32_order_error_is_small_and_sees_the_order():
    V, W, H = _fault_problem()
    em = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16')
    e = CE.fp32_order_error(em['ratio']['gn_ops'], em['ops']['Hu'], em['num'])
    assert 0 < e < E.TOL['bf16']


# ---- the case list -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncu', [256, 304])
def test_case_list_reaches_what_it_claims(ncu):
    cases = CE.conv_cases()
    assert len({c['id'] for c in cases}) == len(cases)
    for c in cases:
        p = CE.plan(c, ncu)
        for cl in c['claims']:
            assert CE.claim_holds(cl, p, c), (c['id'], cl, p)
        if c['precision'] == 'f16':
            assert c['beta'] == 1.0 and p['implicit'] and (p['fold_parts'] and p['fused_sums'] or p['h_rows'])
        assert c['tol_x'] == 1.0 or c.get('tol_ref')                 # a raised tolerance names its reference-side figure
    claimed = {cl for c in cases for cl in c['claims']}
    for need in ('!implicit', 'implicit', 'fold_parts', 'fused_tables', '!fused_tables', '!fused_sums', 'tail_split', 'w_ksplit=2',
                 'wk_fold=1', 'wk_fold=2', 'wk_fold=4', 'h_ksplit>1', 'rows_fused', '!rows_fused', 'c_rows', 'ragged',
                 'ragged_in_grid', '!ragged_in_grid', 'rank_in_ktile', 'batch_in_tile', '!h_rows'):
        assert need in claimed, need
    assert {len(c['ts']) for c in cases} == {1, 2, 3} and any(c['wide'] and c['R'] > 256 for c in cases)
    assert {c['C'] % 128 for c in cases if 'ragged' in c['claims']} >= {1, 2, 8}
    for prec, betas in (('bf16x3', {1, 2, 0.5, 0, -1}), ('bf16', {1, 2, 0.5, 0, 1.5, -1}), ('f16', {1})):
        assert {c['beta'] for c in cases if c['precision'] == prec} >= betas


# The plans a user gets with every switch at its default, over small shapes on both sides of every rule of plan_conv: taps
# and frames aligned or not, T below / at / above 64 and 128, channels around the 64-row tile, the 128-row tile and the
# ragged rule, ranks at each tap fold.  (T, L) / (ts, ls) per number of shift axes.
GRID_AXES = ([((t,), (l,)) for t, l in ((5, 61), (6, 50), (8, 96), (16, 128), (16, 203), (24, 200), (64, 128), (72, 256),
                                        (128, 256), (136, 264))] +
             [((3, 4), (14, 19)), ((3, 8), (18, 24)), ((8, 8), (30, 40)), ((2, 5), (12, 31)), ((4, 16), (20, 48)),
              ((8, 16), (24, 64))] +
             [((2, 3, 8), (6, 9, 16)), ((2, 3, 2), (5, 7, 9)), ((2, 1, 4), (4, 5, 11)), ((2, 2, 16), (5, 6, 32))])
GRID_B, GRID_C, GRID_R, GRID_BETA = (1, 2), (20, 64, 70, 129, 200), (2, 5, 11, 40), (1.0, 2.0, 0.5)


def test_every_default_plan_on_the_grid_has_a_case():
    """Every signature (conv_emulation.signature) that plan_conv reaches on the grid at 256 CUs with the switches at their
    defaults is the signature of at least one case of the per-element GPU test: a plan path added later fails here until it
    has a case."""
    import dataclasses
    import itertools
    from torchnmf_amd import _capi, nmfd_engine as N
    lib = _capi.load()
    covered = {CE.signature(CE.plan(c, 256)) for c in CE.conv_cases()}
    reached = {}
    for (ts, ls), B, C, R, beta in itertools.product(GRID_AXES, GRID_B, GRID_C, GRID_R, GRID_BETA):
        p = dataclasses.asdict(N.plan_conv(lib, B, C, ls, R, ts, beta, True, 256, env={}))
        reached.setdefault(CE.signature(p), (B, C, ls, R, ts, beta))
    missing = {s: ex for s, ex in reached.items() if s not in covered}
    for s, ex in sorted(missing.items(), key=repr):
        print('no case for', s, 'e.g. (B, C, ls, R, ts, beta) =', ex)
    assert len(reached) >= 52                                        # (the grid still reaches what it was built to reach)
    assert not missing, f'{len(missing)} of {len(reached)} signatures of the default-switch grid have no per-element case'


class _TablesOf2GiB:
    """The library with window tables of 2 GiB whatever the shape (the two table-size queries; everything else passes)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ('nmfmu_conv_table_bytes', 'nmfmu_convnd_table_bytes'):
            return lambda *a: 2 ** 31
        return getattr(self._lib, name)


@pytest.mark.parametrize('shape', [(2, 70, (200,), 5, (24,)), (2, 70, (256,), 2, (128,)), (2, 20, (30, 40), 3, (8, 8))],
                         ids=['rows-1d', 'fold-parts', 'rows-2d'])
def test_f16_is_refused_where_the_window_tables_reach_2_gib(shape):
    """Aligned taps and frames whose window tables reach 2 GiB get explicit planes, which are bf16: the plan is the
    NMFD_EXPLICIT=1 plan in every field, 'f16' raises and 'auto' stays split bf16 without looking at data."""
    import dataclasses
    from torchnmf_amd import _capi, nmfd_engine as N
    lib = _capi.load()
    B, C, ls, R, ts = shape
    small = N.plan_conv(lib, B, C, ls, R, ts, 1.0, True, 256, env={})
    assert small.implicit and small.f16_ok                           # (the shapes are admitted while the tables are small)
    big = N.plan_conv(_TablesOf2GiB(lib), B, C, ls, R, ts, 1.0, True, 256, env={})
    explicit = N.plan_conv(lib, B, C, ls, R, ts, 1.0, True, 256, env={'TORCHNMF_AMD_NMFD_EXPLICIT': '1'})
    assert not big.implicit and big.table_bytes == 0
    for k, v in dataclasses.asdict(explicit).items():
        assert getattr(big, k) == v, (k, getattr(big, k), v)
    assert big.f16_ok is False and big.f16_auto is False
    with pytest.raises(ValueError, match="precision 'f16' is built for"):
        N.resolve_precision(big, 'f16', None, None, None)
    assert N.resolve_precision(big, 'auto', None, None, None) == 'bf16x3'      # (no tensor to read: it did not ask)


def test_device_planes_feed_the_numerators_and_a_silent_channel_does_not_hide_the_rest():
    V, W, H = _fault_problem()
    W[3] = 0.0
    for which, fn, beta in (('w', CE.w_half_step, 1), ('h', CE.h_half_step, 0.5)):
        good = fn(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3')
        C, BL = 70, 136
        rp, cp = (128, 256) if which == 'w' else (256, 128)
        got = CE.as_kernel_result(good, 'bf16x3', which, rp, cp)
        same = fn(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3', planes=got['planes'])
        assert np.array_equal(same['num'], good['num']) and np.array_equal(same['new'], good['new'])
        # the other neighbour in one lo word: the numerators follow the device's words, the plane check still judges them
        lo = got['planes']['gn'][1]
        lo[10, 20] += 1
        moved = fn(V.numpy(), W.numpy(), H.numpy(), beta, 'bf16x3', planes=got['planes'])
        assert not np.array_equal(moved['num'], good['num'])
    # num_w of a live row off by 1e-4 next to a silent channel whose numerators are 1e7 times larger
    good = CE.w_half_step(V.numpy(), W.numpy(), H.numpy(), 1, 'bf16x3')
    num = good['num'].copy()
    assert num[3].min() > 1e5 * num[10].max()
    num[10, 7] *= 1 + 1e-4
    ok, _, fig = _judge('w', 'bf16x3', 1, V, W, H, dict(good, num=num), good)
    assert not ok and fig['num'] > 5e-5 and fig['master'] == 0.0
