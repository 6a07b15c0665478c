"""The dense loss kernels per partial against the float64 model of tests/mu_emulation.py.

``DenseMU.divergence()`` -- the value fit()'s stop rule differences -- is one float per (row block, contraction split) from
the loss instance of the ping-pong kernel (256-row blocks) or of the four-wave kernel (everything else: also where the MU
step is the sp, sp2 or Gram-path kernel), summed in float64 in a fixed order.  For every case of ``mu_emulation.loss_cases``:

* the plan is the engine's: loss kernel family, tile height, nsplit, number of partials;
* every partial (the buffer poisoned with NaN first) against its float64 reference under its own derived bound
  (``loss_partials``: loss_elem's roundings, the lane's addition chain, the reduction tree, the fp32 reconstruction); a partial
  without a valid element -- an empty split, a split or a row block of padding only -- must be exactly 0.0;
* the double total is the fixed-order float64 sum of the partials read back, bit for bit.

The riding loss (the W half-step after a checkpoint carries the loss): every (sum x log2 s, sum s) pair per wave against
``riding_partials``, the finished value against the float64 KL divergence under ``riding_total``'s bound.  The fused checkpoint's
range flag.  ``metrics.beta_div`` on plain arrays around its launch boundaries, and ``target_stats`` on targets smaller than a
workgroup.  Each reference is computed from the images read back from the GPU.
"""
import numpy as np
import pytest
import torch

from conftest import record
import mu_emulation as E
from oracle import mu_oracle as O
from test_gpu_emulated_parity import _read_images

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _fixed_order_sum(part) -> float:
    """sum_finalize_kernel (nmfmu_aux.hip:403-414) in float64: thread i adds part[i], part[i + 256], ...; then the halving tree."""
    red = np.zeros(256, dtype=np.float64)
    part = np.asarray(part, dtype=np.float64)
    for i in range(min(256, len(part))):
        s = 0.0
        for v in part[i::256]:
            s += float(v)
        red[i] = s
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return float(red[0])


def _engine(dev, monkeypatch, case, V, W0, H0):
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DenseMU
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    stage = _capi.STAGE_DMA_NOP2 if case.get('stage') == 'nop2' else None
    W, H = W0.clone().to(dev), H0.clone().to(dev)
    return DenseMU(V.to(dev), W, H, case['beta'], precision=case['precision'], stage=stage, block_rows=case.get('block_rows'),
                   allow_gram=case.get('gram', False))


@pytest.mark.parametrize('case', E.loss_cases(_ncu()), ids=lambda c: c['id'])
def test_loss_partials(dev, monkeypatch, case):
    from torchnmf_amd import _capi
    ncu = _ncu()
    N, C, R, prec, beta = case['N'], case['C'], case['R'], case['precision'], case['beta']
    plan = E.loss_plan(N, C, R, prec, beta, ncu, case['nsplit'], case['block_rows'], case['gram'])
    V, W0, H0 = E.loss_problem(case)
    eng = _engine(dev, monkeypatch, case, V, W0, H0)
    # the plan is the engine's
    st = eng.step_h
    assert (st.block_rows, st.nsplit, eng.loss_part.numel()) == (plan['block_rows'], plan['nsplit'], plan['nparts']), plan
    assert plan['family'] == ('pp' if st.block_rows == 256 else 'fused')
    assert eng.gram_path == (plan['mu_family'] == 'xb')
    if case['block_rows'] is None and not case['gram']:
        fam = {'pp': _capi.KERNEL_PP, 'sp': _capi.KERNEL_SP, 'sp2': _capi.KERNEL_SP, 'fused': _capi.KERNEL_FUSED}[plan['mu_family']]
        assert eng.be.kernel_family(eng.r_pad, eng.precision, beta) == fam
    if case['group'] in ('pp', 'sp', 'sp2', 'xb'):
        assert plan['mu_family'] == case['group']
    # the loss tile list against the MU step's of the same struct
    if case['group'] in ('sp', 'sp2') and case['nsplit'] == 4:
        assert plan['tiles'] == [5, 5, 5, 5] and plan['mu_tiles'] == [8, 8, 4, 0]
    else:
        assert plan['tiles'] == plan['mu_tiles']
    torch.cuda.synchronize()
    A = _read_images(eng.fH, eng.r_pad, prec)
    B = _read_images(eng.fW, eng.r_pad, prec)
    lp = E.loss_partials(V.numpy(), A, B, beta, prec, plan)
    eng.loss_part.fill_(float('nan'))
    total = eng.divergence()
    part32 = eng.loss_part.cpu().numpy()
    got = part32.astype(np.float64)
    ex = E.partial_excess(got, lp['ref'], lp['bound'])
    nsp = plan['nsplit']
    empty = [i for i in range(plan['nparts']) if plan['tiles'][i % nsp] == 0]
    blank = [i for i in range(plan['nparts']) if lp['bound'][i] == 0]
    live = lp['abs_terms'] > 0
    worst = int(np.argmax(ex))
    print(f"{case['id']}: worst fraction of the bound {ex.max():.3f} at partial {worst} (got {got[worst]!r}, ref {lp['ref'][worst]!r}, "
          f"bound {lp['bound'][worst]:.3e}); bound / terms <= {float((lp['bound'][live] / lp['abs_terms'][live]).max()):.2e}; "
          f"total {total!r} vs model {lp['ref'].sum()!r}")
    record('loss_emulated_parity', case=case['id'], family=plan['family'], precision=prec, beta=beta, tiles=plan['tiles'],
           mu_tiles=plan['mu_tiles'], worst_fraction=float(ex.max()), worst_partial=worst, empty=empty, blank=blank,
           total=total, model_total=float(lp['ref'].sum()), bound_total=float(lp['bound'].sum()))
    assert np.isfinite(got).all(), 'poison read back: a workgroup did not write its slot'
    assert all(part32[i] == 0.0 for i in empty + blank), (empty, blank, part32)
    assert ex.max() <= 1.0, (worst, float(ex.max()), got[worst], lp['ref'][worst], lp['bound'][worst])
    assert total == _fixed_order_sum(part32)
    if case['fitted']:
        # total cancellation: no relative tolerance on the loss means anything here; it may not be negative beyond the bound
        assert total >= -float(lp['bound'].sum()), (total, float(lp['bound'].sum()))


@pytest.mark.parametrize('case', E.RIDING_CASES, ids=lambda c: c['id'])
def test_riding_loss_pairs_and_total(dev, monkeypatch, case):
    ncu = _ncu()
    N, C, R, prec = case['N'], case['C'], case['R'], case['precision']
    plan = E.riding_plan(N, C, R, prec, ncu, case['nsplit'])
    V, W0, H0 = E.riding_problem(case)
    eng = _engine(dev, monkeypatch, case, V, W0, H0)
    assert eng._riding is not None
    sw = eng.step_w
    assert (sw.block_rows, sw.nsplit) == (256, plan['nsplit'])
    torch.cuda.synchronize()
    A = _read_images(eng.fW, eng.r_pad, prec)        # the images BEFORE the update: what the checkpoint's loss is about
    B = _read_images(eng.fH, eng.r_pad, prec)
    eng.checkpoint_begin()
    assert eng._riding_pending
    buf = eng._riding['bufs'][0]
    assert buf.numel() == 16 * plan['nwg']
    buf.fill_(float('nan'))
    eng.w_step()
    div, left = eng.checkpoint_result()
    pairs = buf.cpu().double().numpy().reshape(plan['nwg'], 8, 2)
    rp = E.riding_partials(V.numpy().T, A, B, prec, plan)
    ex = E.partial_excess(pairs.reshape(-1), rp['ref'].reshape(-1), rp['bound'].reshape(-1)).reshape(pairs.shape)
    rt = E.riding_total(V.numpy(), A, B, prec, plan)
    frac_total = abs(div - rt['ref']) / rt['bound']
    print(f"{case['id']}: pairs worst fraction x log2 s {ex[..., 0].max():.3f}, s {ex[..., 1].max():.3f}; total {div!r} vs {rt['ref']!r}, "
          f"bound {rt['bound']:.3e} (fraction {frac_total:.3f})")
    record('riding_emulated_parity', case=case['id'], precision=prec, tiles=plan['tiles'], worst_xlogs=float(ex[..., 0].max()),
           worst_s=float(ex[..., 1].max()), total=div, ref=rt['ref'], bound=rt['bound'], total_fraction=float(frac_total))
    assert np.isfinite(pairs).all(), 'poison read back: a wave did not write its pair'
    assert not left
    assert ex.max() <= 1.0, (np.unravel_index(int(np.argmax(ex)), ex.shape), float(ex.max()))
    assert frac_total <= 1.0, (div, rt)


def test_loss_checkpoint_range_flag(dev):
    """nmfmu_loss_checkpoint: out2[1] is bit 0 of the step's status word, out2[0] the loss pass's value bit for bit, and the two
    snapshots are the factors."""
    from torchnmf_amd.engine import DenseMU
    g = torch.Generator().manual_seed(17)
    N, C, R = 300, 520, 12
    V = (torch.rand(N, C, generator=g) + 0.01).half().float().to(dev)
    W, H = (torch.rand(C, R, generator=g) + 0.1).to(dev), (torch.rand(N, R, generator=g) + 0.1).to(dev)
    eng = DenseMU(V, W, H, 1.0, precision='f16')
    want = eng.divergence()
    for flag in (1, 0, 3, 2):
        eng.status.fill_(flag)
        out2 = torch.full((2,), float('nan'), dtype=torch.float64, device=dev)
        snaps = [torch.full_like(eng.fW.f, float('nan')), torch.full_like(eng.fH.f, float('nan'))]
        eng.loss_part.fill_(float('nan'))
        eng.be.loss_checkpoint(eng.step_h, eng.loss_part, out2, eng.fW.f, snaps[0], eng.fH.f, snaps[1])
        torch.cuda.synchronize()
        assert float(out2[1]) == float(flag & 1), (flag, out2)
        assert float(out2[0]) == want
        assert torch.equal(snaps[0], eng.fW.f) and torch.equal(snaps[1], eng.fH.f)
    eng.status.zero_()


# n on both sides of one workgroup (256 threads) and of the grid cap (1024 workgroups x 256: beyond it a thread strides);
# the kernel loads scalars, so there is no vector-width remainder to straddle
BETA_DIV_N = (1, 255, 256, 257, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1, 300001)


@pytest.mark.parametrize('beta', [-1, 0, 0.5, 1, 1.5, 2, 3])
def test_metrics_beta_div_on_plain_arrays(dev, beta):
    """metrics.beta_div (nmfmu_beta_div, 1024 doubles of scratch) against oracle.mu_oracle.beta_div in float64, with 30 % exact
    zeros in the reconstruction, in the target and in both, under ``beta_div_bound``."""
    from torchnmf_amd.metrics import beta_div
    b32 = float(np.float32(beta))
    worst = 0.0
    for n in BETA_DIV_N:
        g = torch.Generator().manual_seed(n % 1000 + 1)
        x0, y0 = torch.rand(n, generator=g), torch.rand(n, generator=g)
        zx, zy = torch.rand(n, generator=g) < 0.3, torch.rand(n, generator=g) < 0.3
        for pat in ('none', 'x', 'y', 'both'):
            x = torch.where(zx, torch.zeros(()), x0) if pat in ('x', 'both') else x0
            y = torch.where(zy, torch.zeros(()), y0) if pat in ('y', 'both') else y0
            got = float(beta_div(x.to(dev), y.to(dev), beta))
            ref, bound = E.beta_div_bound(x.numpy(), y.numpy(), b32)
            want = float(O.beta_div(x.double(), y.double(), b32))
            at = float(E.loss_abs_terms(x.double().numpy() + (0.0 if beta == 2 else E.EPS), y.double().numpy(), b32).sum())
            assert abs(want - ref) <= 1e-12 * at, (n, pat, want, ref)
            assert np.isfinite(got), (n, pat)
            frac = abs(got - want) / (bound + 1e-12 * at)
            worst = max(worst, frac)
            assert frac <= 1.0, (n, pat, got, want, bound)
    record('beta_div_plain', beta=beta, worst_fraction=worst)


def test_target_stats_on_targets_smaller_than_a_workgroup(dev):
    """nmfmu_target_sums launches 1024 workgroups whatever the size: 1 x 1, 3 x 5 and a one-row strided view leave nearly all of
    them empty.  The assertions of test_target_stats_one_pass_matches_the_torch_passes."""
    from torchnmf_amd.engine import DenseMU, DEFAULT_BACKEND_FACTORY, target_stats
    be = DEFAULT_BACKEND_FACTORY()
    g = torch.Generator().manual_seed(3)
    W, H = (torch.rand(500, 8, generator=g) + 0.1).to(dev), (torch.rand(300, 8, generator=g) + 0.1).to(dev)
    big = torch.rand(4, 700, generator=g)
    cases = {'1x1': torch.rand(1, 1, generator=g), '1x1-exact': torch.full((1, 1), 0.5), '1x1-zero': torch.zeros(1, 1),
             '3x5': torch.rand(3, 5, generator=g), '3x5-exact': torch.rand(3, 5, generator=g).half().float(),
             'row': big[1:2, :500], 'row-exact': big.half().float()[1:2, :500]}
    for name, v in cases.items():
        if name.startswith('row'):
            src = (big if name == 'row' else big.half().float()).to(dev)
            vd = src[1:2, :500]
            assert vd.stride(0) == 700 and vd.shape == (1, 500)
        else:
            vd = v.to(dev)
        got = DenseMU.f16_stats(vd, W, H, be)
        want = DenseMU.f16_stats(vd, W, H)
        assert got == want, (name, got, want)
        assert got[1] == name.endswith(('exact', 'zero'))
        out4 = target_stats(vd, be).cpu()
        assert bool(torch.isfinite(out4).all())
        v64 = v.double()
        assert float(out4[1]) == pytest.approx(float(v64.sum()), rel=1e-9)
        ref_a = float((v64 * (v.float() + torch.finfo(torch.float32).eps).double().log()).sum())
        assert float(out4[0]) == pytest.approx(ref_a, rel=2e-6, abs=1e-3), (name, float(out4[0]), ref_a)
        assert float(out4[2]) == float(v.max())
