"""The simulated world of tests/shard_sim.py on the CPU, over the oracle-backed stand-in backend (tests/cpu_backend.py).

What runs here is torchnmf_amd's host logic of the column-sharded H half-step -- both forms -- with the G shards one after
the other in this process, ``torch.distributed.all_reduce`` replaced by ``ShardWorld``.  The checks are the ones the GPU test
(tests/test_gpu_sharded_emulated_parity.py) applies to the HIP kernels, here against the plain float64 algorithm (the stand-in
computes from the fp32 masters; its partial sums are taken in float64 so that ``mu_emulation.TOL`` means something).  Seeded
faults show which check catches what.
"""
import pytest
import torch

from conftest import rel_err
import mu_emulation as E
import shard_sim as S
from cpu_backend import OracleBackend
from oracle import mu_oracle as O

CPU = torch.device('cpu')
CASES = S.shard_cases(256)


class Oracle64(OracleBackend):
    """The stand-in with its contractions in float64 (slabs, masters and column sums stay fp32)."""

    def _terms(self, st):
        A, B, X = st.owner.f.double(), st.panel.f.double(), st.xp.double()
        return O.mu_terms(X, A @ B.t(), float(st.struct.beta)), B


# ---- seeded faults: each is a stand-in backend (or world) that is wrong in one way ------------------------------------
class LocalColumnSums(Oracle64):
    """The apply takes its beta == 1 denominators from the local fW.colsum, not from the reduced tail."""

    def mu_apply(self, st, num, den, nslab, kl_den):
        super().mu_apply(st, num, den, nslab, st.panel.colsum if kl_den is not None else None)


class ApplyReadsSlabs(Oracle64):
    """The apply ignores ``num`` / ``den`` and sums st.slab_num / st.slab_den: the local partial sums."""

    def mu_apply(self, st, num, den, nslab, kl_den):
        super().mu_apply(st, None, None, 0, kl_den)


class DropsLastSlab(Oracle64):
    def slab_reduce(self, st, num_out, den_out):
        num_out.copy_(st.slab_num.view(st.nsplit, -1)[:-1].sum(0))
        if den_out is not None:
            den_out.copy_(st.slab_den.view(st.nsplit, -1).sum(0))


class TailAtOffsetZero(Oracle64):
    """Row-halves form: the apply takes the tail from offset 0 of the SECOND collective's buffer, not from behind the
    numerator plane."""

    def mu_apply(self, st, num, den, nslab, kl_den):
        eng = self.eng
        if eng._h_rows is not None and st is eng.step_h:
            off = eng._h_rows[0].plane
            if kl_den is not None:
                kl_den = eng.xbuf[off:off + kl_den.numel()]
            else:
                den = eng.xbuf[off:off + den.numel()]
        super().mu_apply(st, num, den, nslab, kl_den)


class LeavesLastRankOut(S.ShardWorld):
    def reduce(self, idx, op):
        full, self.G = self.G, self.G - 1
        try:
            return super().reduce(idx, op)
        finally:
            self.G = full


def _world(monkeypatch, case, world_cls=S.ShardWorld):
    import torch.distributed as dist
    world = world_cls(case['G'])
    monkeypatch.setattr(dist, 'all_reduce', world.all_reduce)
    monkeypatch.setenv('TORCHNMF_AMD_AR_OVERLAP', '1' if case['form'] == 'rows' else '0')
    monkeypatch.delenv('TORCHNMF_AMD_AR_SPLIT', raising=False)
    monkeypatch.delenv('TORCHNMF_AMD_COMM', raising=False)
    return world


def _run(monkeypatch, case, backend=Oracle64, world_cls=S.ShardWorld, iters=1):
    world = _world(monkeypatch, case, world_cls)
    V, W0, H0 = S.shard_problem(case)
    engines = S.build_engines(case, V, W0, H0, CPU, backend_factory=backend)
    for eng in engines:
        assert (eng._h_rows is not None) == (case['form'] == 'rows')
        if eng._h_rows is not None:
            assert [(v.r0, v.owner.rows, v.owner.rows_pad) for v in eng._h_rows] == S.row_parts(case['N'])
    out = None
    for _ in range(iters):
        for eng in engines:
            eng.w_step()
        out, _, _ = S.checked_h_step(world, engines, case, V, S.master_reader, False, E.TOL[case['precision']], images=False)
    return out


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['id'])
def test_checks_pass_on_the_stand_in(monkeypatch, case):
    """Every case of the GPU test, unfaulted: checks 2 to 6 hold for the stand-in at the GPU test's tolerance."""
    out = _run(monkeypatch, case, iters=2)
    assert out['master'] <= E.TOL[case['precision']] and out['wrong_refs_far'] > 0.5


def _pick(form, kl, n=2):
    """The first ``n`` cases of a form with beta == 1 (kl) or beta != 1, unequal bounds first."""
    sel = [c for c in CASES if c['form'] == form and (E.beta_kind(c['beta']) == 'kl') == kl]
    sel.sort(key=lambda c: c['bounds'] is None)
    return sel[:n]


FAULTS = [(LocalColumnSums, S.ShardWorld, 'apply', _pick('single', True) + _pick('rows', True)),
          (ApplyReadsSlabs, S.ShardWorld, 'apply', _pick('single', True, 1) + _pick('single', False, 1) + _pick('rows', True, 1)
           + _pick('rows', False, 1)),
          (DropsLastSlab, S.ShardWorld, 'contribution', _pick('single', True, 1) + _pick('single', False, 1)
           + _pick('rows', True, 1) + _pick('rows', False, 1)),
          (TailAtOffsetZero, S.ShardWorld, 'apply', _pick('rows', True) + _pick('rows', False)),
          (Oracle64, LeavesLastRankOut, 'reduced', _pick('single', True, 1) + _pick('single', False, 1) + _pick('rows', True, 1)
           + _pick('rows', False, 1))]


@pytest.mark.parametrize('backend,world_cls,check,case',
                         [(b, w, ch, c) for b, w, ch, cs in FAULTS for c in cs],
                         ids=lambda v: v['id'] if isinstance(v, dict) else getattr(v, '__name__', str(v)))
def test_seeded_fault_is_caught_by_its_check(monkeypatch, backend, world_cls, check, case):
    with pytest.raises(S.ShardCheckError) as ei:
        _run(monkeypatch, case, backend, world_cls)
    assert ei.value.check == check, str(ei.value)


def test_replay_refuses_a_contribution_that_changed(monkeypatch):
    """One slab element perturbed between the passes: the replay must refuse it, not reduce it."""
    case = next(c for c in CASES if c['form'] == 'single' and c['family'] == 'pp')
    world = _world(monkeypatch, case)
    V, W0, H0 = S.shard_problem(case)
    engines = S.build_engines(case, V, W0, H0, CPU, backend_factory=Oracle64)

    class Nudged(Oracle64):
        def mu_partial(self, st):
            super().mu_partial(st)
            st.slab_num[5] *= 1.001

    def nudge():
        engines[1].be = Nudged()
    with pytest.raises(S.ShardCheckError) as ei:
        world.h_step(engines, after_restore=nudge)
    assert ei.value.check == 'replay' and 'rank 1 call 0: 1 words differ' in str(ei.value)
    assert world.mode is None and world.rank is None


def _small_problem(beta):
    g = torch.Generator().manual_seed(77)
    N, Cc, R = 300, 90, 5          # 300 rows pad to 512: row halves [0, 256) and [256, 512) with 44 valid rows
    V = torch.rand(N, Cc, generator=g) + (1e-3 if beta <= 0 else 0.0)
    return V, torch.randn(Cc, R, generator=g).abs() + 1e-3, torch.randn(N, R, generator=g).abs() + 1e-3


@pytest.mark.parametrize('beta', [1, 2, 0.5])
@pytest.mark.parametrize('form', ['single', 'rows'])
@pytest.mark.parametrize('G', [2, 3])
def test_two_iterations_reproduce_the_unsharded_oracle(monkeypatch, G, form, beta):
    """The stand-in world against oracle.mu_oracle on the unsharded problem, at the tolerance of the gloo tests."""
    V, W0, H0 = _small_problem(beta)
    case = dict(N=300, C=90, R=5, G=G, bounds=None, form=form, beta=float(beta), precision='bf16x3', regs=(0.025, 0.025))
    world = _world(monkeypatch, case)
    engines = S.build_engines(case, V, W0, H0, CPU, backend_factory=OracleBackend)
    assert all((e._h_rows is not None) == (form == 'rows') for e in engines)
    gamma = O.gamma_of(beta)
    Wr, Hr = W0.clone(), H0.clone()
    for _ in range(2):
        for e in engines:
            e.w_step()
        world.h_step(engines)
        Wr = O.nmf_w_step(V, Wr, Hr, beta, gamma, 0.025, 0.025)
        Hr = O.nmf_h_step(V, Wr, Hr, beta, gamma, 0.025, 0.025)
    S.check_replication(engines, images=False)
    assert rel_err(torch.cat([e.fW.f for e in engines]), Wr) < 1e-5
    assert all(rel_err(e.fH.f, Hr) < 1e-5 for e in engines)
    # the loss and the flags through the same record / replay
    totals = world.divergence(engines)
    assert len(set(totals)) == 1
    want = 0.0
    for g in range(G):
        want += float(world.sent[(g, 0)].item())
    assert totals[0] == want
    assert totals[0] == pytest.approx(float(O.beta_div(Hr @ Wr.t(), V, beta)), rel=1e-4)
    assert world.target_flags(engines) == [(False, False)] * G


@pytest.mark.parametrize('kind,want', [('zero', (False, True)), ('negative', (True, None)), ('nan', (True, None))])
def test_flags_of_one_shard_reach_every_rank(monkeypatch, kind, want):
    V, W0, H0 = _small_problem(1)
    V = V.clone()
    V[7, 80] = {'zero': 0.0, 'negative': -1.0, 'nan': float('nan')}[kind]     # a column of the last shard only
    case = dict(N=300, C=90, R=5, G=3, bounds=None, form='single', beta=1.0, precision='bf16x3', regs=(0.0, 0.0))
    world = _world(monkeypatch, case)
    engines = S.build_engines(case, V, W0, H0, CPU, backend_factory=OracleBackend)
    got = world.target_flags(engines)
    assert len(set(got)) == 1 and got[0][0] == want[0]
    assert want[1] is None or got[0][1] == want[1]


@pytest.mark.parametrize('case', [c for c in CASES if c['ki_rank'] is not None], ids=lambda c: c['id'])
def test_ki_cases_have_different_scale_exponents(case):
    """The condition the ki cases are named for, from column sums computed on the host: it is checked here, not discovered on
    the GPU.  (The GPU test asserts it again from the column sums it reads back before every H half-step.)"""
    V, W0, H0 = S.shard_problem(case)
    assert case['precision'] == 'f16' and E.beta_kind(case['beta']) in ('is', 'sqrt')
    cs_H = H0.sum(0).numpy()
    cs_W = [W0[s:e].sum(0).numpy() for s, e in S.case_bounds(case)]
    kis = S.check_ki_condition(case, cs_H, cs_W)
    assert len(kis) == case['G']


def test_case_matrix_names_every_family_in_both_forms():
    for form in ('single', 'rows'):
        have = {(c['family'], c['precision'], c['beta']) for c in CASES if c['form'] == form}
        assert have >= set(S.FAMILY_TABLE), set(S.FAMILY_TABLE) - have
        assert any(c['bounds'] is not None for c in CASES if c['form'] == form)
        assert {c['G'] for c in CASES if c['form'] == form} == {2, 3}
        for fam in ('pp', 'fused', 'sp', 'sp2'):
            ns = [p['nsplit'] for c in CASES if c['form'] == form and c['family'] == fam for p in c['plans']]
            assert 1 in ns and max(ns) > 1, (form, fam, ns)
    for c in CASES:
        assert [p['family'] for p in c['plans']] == [c['family']] * c['G']
        if c['form'] == 'rows':
            N = c['N']
            want = {300: [(0, 256, 256), (256, 44, 256)], 700: [(0, 256, 256), (256, 444, 512)]}[N]
            assert all([r[:3] for r in p['rows']] == want for p in c['plans'])
        else:
            assert all(p['rows'] is None for p in c['plans'])
        V, _, _ = S.shard_problem(c)
        assert float(V.min()) > 0                      # the clean target sets neither flag
    uneq = [c for c in CASES if c['bounds'] == S.UNEQ3]
    assert uneq and all(p['k_pad'] for p in uneq[0]['plans']) and [p['k_pad'] for p in uneq[0]['plans']] == [256, 512, 768]
