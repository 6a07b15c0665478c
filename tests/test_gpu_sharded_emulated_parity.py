"""The column-sharded H half-step on the HIP kernels with more than one shard, per element (tests/shard_sim.py).

``DenseMU(group=...)`` had only ever run on the GPU at world size 1, where the all-reduce is the identity: an apply that took
its beta == 1 denominators from the local column sums, read the slabs instead of the reduced buffer, added slab planes beyond
``nslab = 1`` or read the tail of the row-halves form at the wrong offset would have passed, and so would a slab contribution
that is only right when it is the whole sum (the per-launch fp16 scale exponent ki differs between shards and between the two
row halves of one shard, and must be taken out again before the slabs are written).

Here G = 2 and 3 engines live on ``cuda:0``, each on its own column shard with its own clones of ``W[C_g]`` and ``H``, and
``torch.distributed.all_reduce`` is ``shard_sim.ShardWorld``: record, restore, replay, exact by the bit-for-bit assertion of
the replay.  For every case of ``shard_sim.shard_cases`` -- every kernel family the sharded H half-step can run on, in the
single-collective form and the row-halves form (TORCHNMF_AMD_AR_OVERLAP=1), equal and unequal shards, split and unsplit
contractions -- two iterations of W half-steps and one H half-step of the whole world, each H half-step emulated from the
masters, images and column sums read back before it:

1. the case is what it says: kernel family, tile height, nsplit as ``mu_emulation.half_step_plan`` gives them for the shard's
   shape; the row halves present exactly where expected; never the Gram path;
2. each rank's recorded packed buffer: numerator (and denominator) plane per element against ``mu_emulation.half_step`` on
   the shard, each launch of the row-halves form with its own M; at beta == 1 the tail is ``fW.colsum`` bit for bit;
3. the reduced buffer is bit for bit the rank-order fp32 sum of the contributions;
4. the apply sees only the reduced buffer (its padding is NaN): every element of the new H against ``mu_emulation.apply`` of
   the float64 sums; images bit-exact the rounding of the new master with zero padding; column sums; status clear;
5. H, its images and column sums bit-equal on all ranks;
6. wrong references (local column sums, a numerator without one rank) are farther than the tolerance on most elements;
7. the loss: each rank's value against ``mu_emulation.loss_partials`` on its shard, the total the rank-order double sum;
8. flags: a zero, a negative entry, a NaN in one shard's target reach every rank.

The bound is ``mu_emulation.TOL[precision]`` throughout; the one rounding the sharded path adds, the rank-order fp32 sum, is
allowed for as (G - 1) 2^-24 sum_g |c_g| per element (``shard_sim.summed``).

``allreduce='direct'`` (``nmfmu_mu_step_allreduce``) performs the collective inside the library over RCCL and cannot be
simulated; it issues the same four calls in the same order (nmfmu_capi.hip) and keeps its world-1 test
(``test_sharded_path_world1_rccl``).
"""
import pytest
import torch

from conftest import record
import mu_emulation as E
import shard_sim as S
from test_gpu_emulated_parity import _check_images, _read_images
from test_gpu_loss_emulated_parity import _fixed_order_sum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _check_plan(case, engines):
    from torchnmf_amd import _capi
    fam = {'pp': _capi.KERNEL_PP, 'sp': _capi.KERNEL_SP, 'sp2': _capi.KERNEL_SP, 'fused': _capi.KERNEL_FUSED}[case['family']]
    for eng, plan in zip(engines, case['plans']):
        st = eng.step_h
        assert not eng.gram_path and eng._comm is None
        assert eng.be.kernel_family(eng.r_pad, eng.precision, case['beta']) == fam
        assert (st.block_rows, st.nsplit) == (plan['block_rows'], plan['nsplit']), plan
        if plan['rows'] is None:
            assert eng._h_rows is None
        else:
            assert [(v.r0, v.owner.rows, v.owner.rows_pad, v.nsplit) for v in eng._h_rows] == plan['rows']


def _check_owner(case, eng):
    """Check 4 beyond the masters: images, column sums, status of one rank's H."""
    from torchnmf_amd import _capi
    st, R = eng.step_h, case['R']
    nop2 = st.struct.stage == _capi.STAGE_DMA_NOP2 and case['family'] == 'sp'
    bad = _check_images(st.owner, st.r_pad, case['precision'], nop2)
    assert not any(bad.values()), bad
    full = st.owner.f.cpu().double()
    cs = st.owner.colsum.cpu().double()
    assert float(((cs[:R] - full.sum(0)).abs() / full.sum(0).abs().clamp_min(1e-30)).max()) <= 1e-6
    assert R == st.r_pad or float(cs[R:].abs().max()) == 0.0
    assert int(eng.status.item()) & 1 == 0


def _check_loss(case, world, engines, V, bounds, ncu):
    """Check 7.  Returns the worst |local - ref| / bound over the ranks."""
    N, R, prec, beta = case['N'], case['R'], case['precision'], case['beta']
    refs = []
    for eng, (s, e) in zip(engines, bounds):
        plan = E.loss_plan(N, e - s, R, prec, beta, ncu, case['nsplit'], None)
        assert (eng.step_h.block_rows, eng.step_h.nsplit, eng.loss_part.numel()) == (plan['block_rows'], plan['nsplit'],
                                                                                   plan['nparts'])
        lp = E.loss_partials(V[:, s:e].numpy(), _read_images(eng.fH, eng.r_pad, prec), _read_images(eng.fW, eng.r_pad, prec),
                             beta, prec, plan)
        refs.append((_fixed_order_sum(lp['ref']), float(lp['bound'].sum())))
    totals = world.divergence(engines)
    worst, want = 0.0, 0.0
    for g, (ref, bound) in enumerate(refs):
        local = float(world.sent[(g, 0)].item())
        frac = abs(local - ref) / bound
        print(f"  loss rank {g}: {local!r} vs {ref!r}, bound {bound:.3e} (fraction {frac:.3f})")
        assert frac <= 1.0, (g, local, ref, bound)
        worst = max(worst, frac)
        want += local
    assert totals == [want] * len(engines), (totals, want)
    return worst


def _check_flags(case, world, engines, V, bounds, dev):
    """Check 8: the flags of ONE shard's target reach every rank (``repack_target`` re-runs the validation)."""
    G = case['G']
    assert world.target_flags(engines) == [(False, False)] * G
    g = G - 1
    s, e = bounds[g]
    for val in (0.0, -1.0, float('nan')):
        Vg = V[:, s:e].clone()
        Vg[min(3, case['N'] - 1), (e - s) // 2] = val
        engines[g].repack_target(Vg.to(dev))
        got = world.target_flags(engines)
        assert len(set(got)) == 1, got
        assert (got[0] == (False, True)) if val == 0.0 else (got[0][0] is True), (val, got)
    engines[g].repack_target(V[:, s:e].contiguous().to(dev))
    assert world.target_flags(engines) == [(False, False)] * G


@pytest.mark.parametrize('case', S.shard_cases(_ncu()), ids=lambda c: c['id'])
def test_sharded_h_half_steps_per_element(dev, monkeypatch, case):
    import torch.distributed as dist
    ncu = _ncu()
    prec, G = case['precision'], case['G']
    tol = E.TOL[prec]
    if case['nsplit'] is not None:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    monkeypatch.setenv('TORCHNMF_AMD_AR_OVERLAP', '1' if case['form'] == 'rows' else '0')
    monkeypatch.delenv('TORCHNMF_AMD_AR_SPLIT', raising=False)
    monkeypatch.delenv('TORCHNMF_AMD_COMM', raising=False)
    world = S.ShardWorld(G)
    monkeypatch.setattr(dist, 'all_reduce', world.all_reduce)
    V, W0, H0 = S.shard_problem(case)
    bounds = S.case_bounds(case)
    engines = S.build_engines(case, V, W0, H0, dev)
    _check_plan(case, engines)
    torch.cuda.synchronize()
    for it in range(2):
        for eng in engines:
            eng.w_step()
        out, states, ems = S.checked_h_step(world, engines, case, V, _read_images, True, tol)
        print(f"{case['id']} it {it}: num {out['num']:.3e} den {out['den']:.3e} master {out['master']:.3e} (raw {out['num_raw']:.3e} {out['den_raw']:.3e} {out['master_raw']:.3e}; tol {tol:.1e}); "
              f"wrong references far on >= {out['wrong_refs_far']:.2f}; ki {out['ki']}")
        for eng in engines:
            _check_owner(case, eng)
        if case['ki_rank'] is not None:
            kis = S.check_ki_condition(case, states[0]['cs_o'], [st['cs_p'] for st in states])
            assert [[k for _, k in r] for r in kis] == out['ki']
        loss = _check_loss(case, world, engines, V, bounds, ncu)
        record('sharded_parity', case=case['id'], family=case['family'], precision=prec, beta=case['beta'], form=case['form'],
               G=G, it=it, tol=tol, nsplit=[e.step_h.nsplit for e in engines], loss_fraction=loss, **out)
    _check_flags(case, world, engines, V, bounds, dev)
