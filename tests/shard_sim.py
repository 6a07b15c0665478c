"""A simulated world of column shards on one device, and the checks of the sharded H half-step (test-only).

``DenseMU(group=...)``: rank g holds ``V[:, C_g]`` and ``W[C_g]``, ``H`` is replicated.  The H half-step
is partial sums -> ``slab_reduce`` into the packed buffer ``[numerator | sum_c W or denominator]`` -> all-reduce ->
``mu_apply(nslab = 1)`` on the reduced buffer.  The engine asks one thing of ``torch.distributed``: ``all_reduce``.
``ShardWorld`` stands in for it, so that the G shards run one after the other in ONE process on one device:

* record: every engine runs its half-step; each tensor handed to ``all_reduce`` is cloned under (rank, index of the call) and
  left as it is (that pass's apply sees a local buffer; its result is thrown away);
* the masters are restored and the images rebuilt, so the second pass starts from the same bits;
* replay: every engine runs the half-step again.  The tensor handed in must equal the recorded one BIT FOR BIT -- the
  kernels are deterministic run to run, and this assertion is what makes the replay a legitimate collective -- and is then
  overwritten with the reduction over ranks of the recorded tensors: SUM in rank order 0 .. G-1 in the tensor's own dtype,
  MIN / MAX elementwise.

No thread, no barrier, no second process, nothing that waits on a peer.  What this does not cover: RCCL itself, and
``allreduce='direct'`` (``nmfmu_mu_step_allreduce`` performs the collective inside the library).

The checks of one H half-step of the whole world (``checked_h_step``) are shared by the GPU test
(tests/test_gpu_sharded_emulated_parity.py: HIP kernels against ``mu_emulation``'s rounding-exact emulation) and the CPU test
(tests/test_shard_sim.py: the oracle-backed stand-in backend against the plain float64 algorithm, with seeded faults).  A
failed check raises ``ShardCheckError`` whose ``check`` names it: 'replay', 'contribution', 'reduced', 'apply',
'replication', 'sensitivity'.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import mu_emulation as E
from oracle import mu_oracle as O

GROUP = object()          # any non-None sentinel: with an explicit precision and ar_direct=False DenseMU only passes it on
U32 = 2.0 ** -24          # unit roundoff of fp32


class ShardCheckError(AssertionError):
    def __init__(self, check: str, msg: str):
        super().__init__(f'[{check}] {msg}')
        self.check = check


def _fail(check, msg):
    raise ShardCheckError(check, msg)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


class _Done:
    """What ``all_reduce(async_op=True)`` returns here: the work is complete when the call returns."""

    def wait(self):
        return True


class ShardWorld:
    """Stand-in for ``torch.distributed.all_reduce`` over G simulated ranks (module docstring)."""

    def __init__(self, G: int):
        self.G = G
        self.mode = None
        self.rank = None
        self.hook = None
        self._idx = 0
        self.sent = {}        # (rank, call index) -> the contribution, cloned
        self.reduced = {}     # call index -> the reduction over ranks (before the hook)
        self.ops = {}

    @contextlib.contextmanager
    def as_rank(self, g: int):
        assert self.rank is None and 0 <= g < self.G
        self.rank, self._idx = g, 0
        try:
            yield self
        finally:
            self.rank = None

    def begin(self, mode: str, hook=None):
        assert mode in ('record', 'replay')
        if mode == 'record':
            self.sent, self.reduced, self.ops = {}, {}, {}
        self.mode, self.hook = mode, hook

    def end(self):
        self.mode, self.hook = None, None

    def reduce(self, idx: int, op):
        """The reduction of call ``idx`` over the ranks, from the recorded contributions, in rank order."""
        import torch.distributed as dist
        out = self.sent[(0, idx)].clone()
        for g in range(1, self.G):
            p = self.sent[(g, idx)]
            if op == dist.ReduceOp.SUM:
                out += p                      # one rounding per rank, in the tensor's own dtype
            elif op == dist.ReduceOp.MIN:
                out = torch.minimum(out, p)
            elif op == dist.ReduceOp.MAX:
                out = torch.maximum(out, p)
            else:
                raise NotImplementedError(op)
        return out

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        import torch.distributed as dist
        op = dist.ReduceOp.SUM if op is None else op
        assert self.rank is not None and self.mode is not None, 'all_reduce outside ShardWorld.as_rank / begin'
        idx = self._idx
        key = (self.rank, idx)
        self._idx += 1
        if self.mode == 'record':
            assert key not in self.sent
            self.sent[key] = tensor.detach().clone()
            assert self.ops.setdefault(idx, op) == op, 'the ranks disagree about the collective'
        else:
            if key not in self.sent or self.ops[idx] != op:
                _fail('replay', f'rank {self.rank} call {idx}: no such collective was recorded')
            want = self.sent[key]
            if not bits_equal(tensor, want):
                n = int((_bits(tensor) != _bits(want)).sum()) if tensor.shape == want.shape else -1
                _fail('replay', f'rank {self.rank} call {idx}: {n} words differ from the recorded contribution')
            if idx not in self.reduced:
                self.reduced[idx] = self.reduce(idx, op)
            out = self.reduced[idx].clone()
            if self.hook is not None:
                self.hook(self.rank, idx, out)
            tensor.copy_(out)
        return _Done() if async_op else None

    # -- a call of every engine, through record and replay
    def both(self, engines, fn, hook=None, between=None):
        """``fn(engine)`` on every rank in record mode, ``between()``, then in replay mode; the replay's results."""
        assert len(engines) == self.G
        try:
            self.begin('record')
            for g, e in enumerate(engines):
                with self.as_rank(g):
                    fn(e)
            if between is not None:
                between()
            self.begin('replay', hook)
            res = []
            for g, e in enumerate(engines):
                with self.as_rank(g):
                    res.append(fn(e))
            return res
        finally:
            self.end()

    def h_step(self, engines, on_ready=None, hook=None, after_restore=None):
        """One H half-step of the whole world: snapshot H, rebuild the images; record; restore; replay."""
        snaps = [e.fH.f.clone() for e in engines]
        for e in engines:
            e.refresh_images()
        if on_ready is not None:
            on_ready()

        def restore():
            for e, s_ in zip(engines, snaps):
                e.fH.f.copy_(s_)
                e.refresh_images()
                e.status.zero_()
            if after_restore is not None:
                after_restore()
        self.both(engines, lambda e: e.h_step(), hook, between=restore)

    def divergence(self, engines):
        return self.both(engines, lambda e: e.divergence())

    def target_flags(self, engines):
        return self.both(engines, lambda e: e.target_flags())


# ---- shards, cases, problems ----------------------------------------------------------------------------------------
def shard_bounds(C: int, G: int, bounds=None):
    """``oracle.mu_oracle.shard_bounds``, or explicit (unequal) bounds checked to tile [0, C) in G pieces."""
    if bounds is None:
        return O.shard_bounds(C, G)
    bounds = [tuple(int(x) for x in b) for b in bounds]
    assert len(bounds) == G and bounds[0][0] == 0 and bounds[-1][1] == C
    assert all(s < e for s, e in bounds) and all(bounds[i][1] == bounds[i + 1][0] for i in range(G - 1))
    return bounds


def case_bounds(case):
    return shard_bounds(case['C'], case['G'], case['bounds'])


UNEQ3 = [(0, 40), (40, 340), (340, 1000)]     # one shard narrower than a 64-column tile; k_pad 256 / 512 / 768
UNEQ2 = [(0, 300), (300, 1000)]
REG = (0.05, 0.05)
KI_FACTOR = 64.0


def row_parts(N: int):
    """The two launches of the row-halves form (engine.DenseMU.__init__ with the default split fraction), or None where the
    engine keeps the single launch: [(r0, valid rows, padded rows)]."""
    m_pad = E.pad_rows(N)
    nblk = m_pad // 256
    r0 = min(max(int(0.5 * nblk + 1e-9), 1), max(nblk - 1, 1)) * 256
    if nblk < 2 or N <= r0:
        return None
    return [(0, r0, r0), (r0, N - r0, m_pad - r0)]


def expected_plan(case, cols: int, ncu: int):
    """What the H half-step of a shard of ``cols`` columns runs with: ``mu_emulation.half_step_plan`` on the shard's shape,
    plus the launches [(r0, rows, rows_pad, nsplit)] (``StepRows.nsplit_for``: at least the whole step's split)."""
    p = E.half_step_plan(case['N'], cols, case['R'], case['precision'], case['beta'], ncu, case['nsplit'], None)['h']
    parts = row_parts(case['N']) if case['form'] == 'rows' else None
    rows = None
    if parts is not None:
        rows = [(r0, n, n_pad, max(p['nsplit'], E.choose_nsplit(n_pad, p['k_pad'], p['r_pad'], case['precision'], case['beta'],
                                                              p['block_rows'], ncu, case['nsplit'])))
                for r0, n, n_pad in parts]
    return dict(family=p['family'], block_rows=p['block_rows'], nsplit=p['nsplit'], rows=rows, k_pad=p['k_pad'])


def shard_cases(ncu: int):
    """The case matrix: every kernel family the sharded H half-step can run on, each in the single-collective form and in the
    row-halves form.  300 rows pad to 512: halves [0, 256) and [256, 512) with 44 valid rows; 700 pad to 768: 256 + 512 with
    444 valid rows.  ``nsplit``: the TORCHNMF_AMD_NSPLIT hook (clipped per shard to k_pad / 256, so the 40-column shard of
    UNEQ3 always runs unsplit); 1 matters because the sharded path must not take the fused-apply epilogue.  ``ki_rank``: the
    shard whose columns (target and W rows) are multiplied by 64, so that the fp16 scale exponent differs between ranks; the
    ki cases have 300 rows, where the two launches of the row-halves form see M = 256 and M = 44: log2(256 / 44) = 2.5 moves
    ki by 2 or 3 at beta = 0 and by 1 or 2 at beta = 0.5, so the halves of one rank always differ too."""
    cases = []

    def add(family, prec, beta, N, R, G, bounds=None, nsplit=None, regs=(0.0, 0.0), sample=None, ki_rank=None, C=1000):
        r_pad = E.pad_rank(R)
        assert E.kernel_family(r_pad, prec, beta, E.default_block_rows(r_pad, prec, beta)) == family
        for form in ('single', 'rows'):
            tag = (f"{family}-{prec}-b{beta:g}-{N}x{C}r{R}-G{G}{'u' if bounds else 'e'}-ns{nsplit}-{form}"
                   + ('-reg' if regs != (0.0, 0.0) else '') + ('-ki' if ki_rank is not None else ''))
            c = dict(id=tag, family=family, precision=prec, beta=float(beta), N=N, C=C, R=R, G=G, bounds=bounds, nsplit=nsplit,
                     form=form, regs=regs, sample=sample, ki_rank=ki_rank, target='rand')
            assert (row_parts(N) is not None)
            c['plans'] = [expected_plan(c, e - s, ncu) for s, e in case_bounds(c)]
            cases.append(c)

    # ping-pong kernel (beta == 1, one operand plane, padded rank <= 128)
    add('pp', 'bf16', 1, 300, 100, 2, None, 2)
    add('pp', 'f16', 1, 300, 33, 3, UNEQ3, 1, REG)           # rank 33: the float4 group 32 .. 35 straddles the rank
    add('pp', 'f16r', 1, 700, 128, 2, UNEQ2, None, sample=96)
    # four-wave kernel, split bf16, every beta branch
    rot = [(24, 2, None, 2, (0.0, 0.0)), (64, 3, UNEQ3, 1, REG), (100, 3, None, 3, (0.0, 0.0)), (100, 2, UNEQ2, 1, REG)]
    for i, beta in enumerate((1, 2, 0, 0.5, 1.5, 3, -1)):
        R, G, bounds, ns, regs = rot[i % len(rot)]
        add('fused', 'bf16x3', beta, 300, R, G, bounds, ns, regs)
    # four-wave kernel, fp16 operands with the per-launch scale exponent
    add('fused', 'f16', 0, 300, 50, 2, None, 2, ki_rank=1)
    add('fused', 'f16', 0.5, 300, 64, 3, UNEQ3, 1, REG, ki_rank=2)
    # beta == 2 on a sharded engine: the reconstruction kernels with denominator slabs (never the Gram path)
    add('fused', 'f16x', 2, 300, 100, 2, None, 1, REG)
    add('fused', 'bf16', 2, 700, 64, 3, None, 2, sample=96)
    # software-pipelined rank-256 kernel
    add('sp', 'f16', 1, 300, 200, 2, None, 2)
    add('sp', 'f16', 1, 300, 200, 3, UNEQ3, 1, REG)
    # two-accumulator kernel (padded rank 128, fp16, beta not in {1, 2})
    add('sp2', 'f16', 0, 300, 100, 2, None, 2, ki_rank=0)
    add('sp2', 'f16', 0.5, 300, 100, 3, UNEQ3, 1, REG, ki_rank=1)
    return cases


# the families of the issue's table: (family, precision, beta)
FAMILY_TABLE = ([('pp', p, 1.0) for p in ('bf16', 'f16', 'f16r')]
                + [('fused', 'bf16x3', b) for b in (1.0, 2.0, 0.0, 0.5, 1.5, 3.0, -1.0)]
                + [('fused', 'f16', 0.0), ('fused', 'f16', 0.5), ('fused', 'f16x', 2.0), ('fused', 'bf16', 2.0),
                   ('sp', 'f16', 1.0), ('sp2', 'f16', 0.0), ('sp2', 'f16', 0.5)])


def shard_problem(case):
    """(V, W0, H0) of a case on the CPU (``mu_emulation.make_problem``), the ``ki_rank`` shard scaled by 64."""
    V, W0, H0 = E.make_problem(case)
    if case['ki_rank'] is not None:
        s, e = case_bounds(case)[case['ki_rank']]
        V[:, s:e] *= KI_FACTOR
        W0[s:e] *= KI_FACTOR
    return V, W0, H0


def sample_rows(case):
    N = case['N']
    if not case['sample']:
        return np.arange(N)
    g = np.random.default_rng(11)
    # always with the first and last row of either launch of the row-halves form
    edge = {0, N - 1, 255, 256} & set(range(N))
    pick = set(g.choice(N, size=case['sample'], replace=False).tolist()) | edge
    return np.array(sorted(pick))


def launch_ki(case, cs_owner, cs_panel, cols: int):
    """ki of every launch of one rank's H half-step: [(M of the launch, ki)]."""
    parts = row_parts(case['N']) if case['form'] == 'rows' else None
    ms = [case['N']] if parts is None else [n for _, n, _ in parts]
    return [(m, E.scale_exponent(cs_owner, cs_panel, m, cols, case['beta'], case['precision'])) for m in ms]


def check_ki_condition(case, cs_H, cs_W):
    """The ki cases are what they say: the exponent differs between ranks, and between the launches of one rank."""
    bounds = case_bounds(case)
    kis = [launch_ki(case, cs_H, cs_W[g], e - s) for g, (s, e) in enumerate(bounds)]
    firsts = {k[0][1] for k in kis}
    assert len(firsts) > 1, ('ki equal on every rank', kis)
    if case['form'] == 'rows':
        assert all(k[0][1] != k[1][1] for k in kis), ('the two halves of a rank share ki', kis)
    return kis


# ---- reading an engine --------------------------------------------------------------------------------------------
def master_reader(fac, r_pad, prec):
    """The stand-in backend keeps no images: its operand IS the fp32 master (padded with zeros)."""
    out = np.zeros((fac.rows_pad, r_pad))
    out[:fac.rows, :fac.rank] = fac.f.detach().cpu().double().numpy()
    return out, None


def read_state(engines, reader, prec):
    """What the H half-step of every rank is about to read: master, operand images, column sums."""
    out = []
    for e in engines:
        st = e.step_h
        out.append(dict(theta=st.owner.f.detach().cpu().double().numpy(), A=reader(st.owner, st.r_pad, prec),
                        B=reader(st.panel, st.r_pad, prec), cs_o=st.owner.colsum.detach().cpu().numpy().copy(),
                        cs_p=st.panel.colsum.detach().cpu().numpy().copy()))
    return out


def launches(eng):
    st = eng.step_h
    if eng._h_rows is None:
        return [(0, st.owner.rows, st.owner.rows_pad)]
    return [(v.r0, v.owner.rows, v.owner.rows_pad) for v in eng._h_rows]


def poison_mask(eng) -> torch.Tensor:
    """Over the packed buffer: padded rows and padded rank columns of the numerator and denominator planes.  The kernel
    reads whole float4 groups, so the group that straddles ``rank`` stays as it is; so does the beta == 1 tail."""
    st = eng.step_h
    rows_pad, r_pad, N, R = st.owner.rows_pad, st.r_pad, st.owner.rows, eng.rank
    m = torch.zeros(rows_pad, r_pad, dtype=torch.bool)
    m[N:] = True
    m[:, -(-R // 4) * 4:] = True
    m = m.reshape(-1)
    tail = torch.zeros(r_pad, dtype=torch.bool) if eng.kl else m
    return torch.cat([m, tail]).to(eng.xbuf.device)


def call_offset(eng, idx: int) -> int:
    """Where in the packed buffer the tensor of collective ``idx`` of an H half-step starts."""
    return 0 if idx == 0 else eng._h_rows[0].plane


def poison_hook(engines):
    masks = [poison_mask(e) for e in engines]

    def hook(rank, idx, out):
        off = call_offset(engines[rank], idx)
        out[masks[rank][off:off + out.numel()]] = float('nan')
    return hook


def contribution(world, g: int, eng) -> torch.Tensor:
    """Rank g's whole packed buffer as recorded: the tensors of its collectives, in order."""
    n = 1 if eng._h_rows is None else 2
    return torch.cat([world.sent[(g, i)].reshape(-1) for i in range(n)]).cpu()


# ---- the checks -----------------------------------------------------------------------------------------------------
def emulate_rank(case, Xg, state, eng, sel, rounding):
    """Float64 numerator / denominator of one rank's contribution on the owner rows ``sel``, launch by launch: each launch of
    the row-halves form with its own M (the kernel computes ki from the launch's ``owner.rows`` and the WHOLE factor's
    column sums).  rounding=False: the plain algorithm on the masters (the CPU stand-in)."""
    beta, prec, R = case['beta'], case['precision'], case['R']
    K = Xg.shape[1]
    A, B = state['A'], state['B']
    kl = E.beta_kind(beta) == 'kl'
    out = dict(num=np.zeros((len(sel), R)), num_amb=np.zeros((len(sel), R)), den=None if kl else np.zeros((len(sel), R)),
               den_amb=np.zeros((len(sel), R)), ki=[])
    pick = lambda im, r: None if im is None else im[r][:, :R]
    for r0, rows, _ in launches(eng):
        idx = np.nonzero((sel >= r0) & (sel < r0 + rows))[0]
        out['ki'].append(E.scale_exponent(state['cs_o'], state['cs_p'], rows, K, beta, prec) if rounding else 0)
        if not len(idx):
            continue
        r = sel[idx]
        if rounding:
            em = E.half_step(Xg[r], None, None, beta, prec, M=rows, K=K, cs_owner=state['cs_o'], cs_panel=state['cs_p'],
                             A_img=(pick(A[0], r), pick(A[1], r)),
                             B_img=(pick(B[0], slice(0, K)), pick(B[1], slice(0, K))))
            assert em['ki'] == out['ki'][-1]
        else:
            em = E.half_step(Xg[r], pick(A[0], r), pick(B[0], slice(0, K)), beta, prec, rounding=False)
        out['num'][idx] = em['num']
        out['num_amb'][idx] = np.broadcast_to(em['num_amb'], em['num'].shape)
        if not kl:
            out['den'][idx] = em['den']
            out['den_amb'][idx] = np.broadcast_to(em['den_amb'], em['den'].shape)
    return out


def check_contributions(case, world, engines, states, ems, sel, tol):
    """Check 2: every rank's recorded packed buffer, plane by plane, against its emulation."""
    R = case['R']
    kl = E.beta_kind(case['beta']) == 'kl'
    worst = {'num': 0.0, 'den': 0.0, 'num_raw': 0.0, 'den_raw': 0.0}      # (_raw: without the ambiguity allowance)
    for g, (eng, stt, em) in enumerate(zip(engines, states, ems)):
        st = eng.step_h
        buf = contribution(world, g, eng)
        if buf.numel() != eng.xbuf.numel():
            _fail('contribution', f'rank {g}: {buf.numel()} floats went through the collectives, the packed buffer has '
                                  f'{eng.xbuf.numel()}')
        plane = st.plane
        num = buf[:plane].view(st.owner.rows_pad, st.r_pad).double().numpy()[sel, :R]
        e = float(E.elem_err(num, em['num'], em['num_amb']).max())
        worst['num'] = max(worst['num'], e)
        worst['num_raw'] = max(worst['num_raw'], float(E.elem_err(num, em['num']).max()))
        if not e <= tol:
            _fail('contribution', f'rank {g}: numerator plane off by {e:.3e} > {tol:.1e}')
        if kl:
            tail = buf[plane:]
            cs = torch.from_numpy(stt['cs_p'])
            if not bits_equal(tail, cs):
                _fail('contribution', f'rank {g}: the beta == 1 tail is not the column sums of this rank\'s W')
            if R < st.r_pad and float(tail[R:].abs().max()) != 0.0:
                _fail('contribution', f'rank {g}: padded ranks of the tail are not zero')
        else:
            den = buf[plane:].view(st.owner.rows_pad, st.r_pad).double().numpy()[sel, :R]
            e = float(E.elem_err(den, em['den'], em['den_amb']).max())
            worst['den'] = max(worst['den'], e)
            worst['den_raw'] = max(worst['den_raw'], float(E.elem_err(den, em['den']).max()))
            if not e <= tol:
                _fail('contribution', f'rank {g}: denominator plane off by {e:.3e} > {tol:.1e}')
    return worst


def check_reduced(world, engines):
    """Check 3: after the replay every rank's packed buffer is, bit for bit, the rank-order fp32 sum of the recorded
    contributions (NaN where the hook poisoned it): the replay keys, and the offsets of the two collectives."""
    bufs = [contribution(world, g, e) for g, e in enumerate(engines)]
    want = bufs[0].clone()
    for b in bufs[1:]:
        want += b
    for g, eng in enumerate(engines):
        mask = poison_mask(eng).cpu()
        got = eng.xbuf.detach().cpu()
        if not bool(torch.isnan(got[mask]).all()):
            _fail('reduced', f'rank {g}: the poison is not where it was put')
        if not bits_equal(got[~mask], want[~mask]):
            n = int((_bits(got[~mask]) != _bits(want[~mask])).sum())
            _fail('reduced', f'rank {g}: {n} words of the reduced buffer are not the rank-order sum of the contributions')


def summed(case, states, ems, leave_out=None):
    """Float64 sums over the ranks of the emulated planes, their ambiguities plus the allowance of the rank-order fp32 sum --
    (G - 1) 2^-24 sum_g |c_g| per element: each of the G - 1 additions rounds a partial sum no larger than sum |c_g| -- and
    the column sums of W (kl_den)."""
    G = len(ems)
    keep = [g for g in range(G) if g != leave_out]
    kl = E.beta_kind(case['beta']) == 'kl'
    num = sum(ems[g]['num'] for g in keep)
    amb_n = sum(ems[g]['num_amb'] for g in keep) + (G - 1) * U32 * sum(np.abs(ems[g]['num']) for g in keep)
    den = amb_d = None
    if not kl:
        den = sum(ems[g]['den'] for g in range(G))
        amb_d = sum(ems[g]['den_amb'] for g in range(G)) + (G - 1) * U32 * sum(np.abs(ems[g]['den']) for g in range(G))
    cs = sum(states[g]['cs_p'].astype(np.float64) for g in range(G))
    cs_abs = sum(np.abs(states[g]['cs_p'].astype(np.float64)) for g in range(G))
    return dict(num=num, den=den, num_amb=amb_n, den_amb=0.0 if amb_d is None else amb_d, kl_den=cs,
                kl_amb=(G - 1) * U32 * cs_abs)


def apply_reference(case, eng, theta, sm, kl_den=None):
    """(reference, allowance) of the new H rows from summed planes: ``mu_emulation.apply`` and ``apply_allowance``, plus --
    at beta == 1 -- what the rounded sum of the column sums can move the element by (d new / new = gamma d pos / pos)."""
    st = eng.step_h.struct
    beta, gamma, l1, l2 = case['beta'], float(st.gamma), float(st.l1), float(st.l2)
    R = case['R']
    kd = sm['kl_den'] if kl_den is None else kl_den
    ref = E.apply(theta, sm['num'], sm['den'], beta, gamma, l1, l2, kl_den=kd)
    allow = E.apply_allowance(ref, sm['num'], sm['den'], sm['num_amb'], sm['den_amb'], beta, gamma, l1=l1, l2=l2, theta=theta)
    if E.beta_kind(beta) == 'kl':
        pos = np.broadcast_to(kd[:R], theta.shape) + l1 + (l2 * theta if l2 > 0 else 0.0)
        allow = allow + np.abs(ref) * gamma * np.broadcast_to(sm['kl_amb'][:R], theta.shape) / pos
    return ref, allow


def check_apply(case, engines, states, ems, sel, tol):
    """Check 4 (masters): every element of every rank's new H against the apply of the float64 sums."""
    sm = summed(case, states, ems)
    worst, raw = 0.0, 0.0
    for g, eng in enumerate(engines):
        theta = states[g]['theta'][sel]
        ref, allow = apply_reference(case, eng, theta, sm)
        new = eng.fH.f.detach().cpu().double().numpy()[sel]
        e = float(E.elem_err(new, ref, allow).max())
        worst, raw = max(worst, e), max(raw, float(E.elem_err(new, ref).max()))
        if not e <= tol:
            _fail('apply', f'rank {g}: new H off by {e:.3e} > {tol:.1e}')
    return worst, raw


def check_replication(engines, images=True):
    """Check 5: H, its images and its column sums are bit-equal on all ranks."""
    e0 = engines[0]
    for g, e in enumerate(engines[1:], 1):
        if not bits_equal(e.fH.f, e0.fH.f):
            _fail('replication', f'H of rank {g} differs from rank 0')
        if not bits_equal(e.fH.colsum, e0.fH.colsum):
            _fail('replication', f'column sums of H on rank {g} differ from rank 0')
        if images:
            for name in ('p1_hi', 'p1_lo', 'p2_hi', 'p2_lo'):
                a, b = getattr(e.fH, name), getattr(e0.fH, name)
                if a is not None and not torch.equal(a, b):
                    _fail('replication', f'image {name} of H on rank {g} differs from rank 0')


def check_sensitivity(case, engines, states, ems, sel, tol):
    """Check 6: the case could tell the difference.  Against an apply whose kl_den is rank 0's column sums alone (beta == 1),
    or whose numerator leaves one rank out (every beta, every rank), most elements of the new H must be farther than tol."""
    sm = summed(case, states, ems)
    theta = states[0]['theta'][sel]
    new = engines[0].fH.f.detach().cpu().double().numpy()[sel]
    wrong = []
    if E.beta_kind(case['beta']) == 'kl':
        wrong.append(('local column sums', apply_reference(case, engines[0], theta, sm,
                                                           kl_den=states[0]['cs_p'].astype(np.float64))))
    for j in range(len(ems)):
        smj = dict(summed(case, states, ems, leave_out=j), den=sm['den'], den_amb=sm['den_amb'])
        wrong.append((f'numerator without rank {j}', apply_reference(case, engines[0], theta, smj)))
    least = 1.0
    for what, (ref, allow) in wrong:
        frac = float((E.elem_err(new, ref, allow) > tol).mean())
        least = min(least, frac)
        if not frac > 0.5:
            _fail('sensitivity', f'{what}: only {frac:.2f} of the elements are farther than {tol:.1e} from the wrong reference')
    return least


def checked_h_step(world, engines, case, V, reader, rounding, tol, sel=None, images=True):
    """One H half-step of the whole world under checks 2 to 6.  Returns the measured maxima, the states read before the
    half-step and the per-rank emulations (for the checks only the GPU test can make: images, column sums, loss)."""
    bounds = case_bounds(case)
    sel = sample_rows(case) if sel is None else sel
    box = {}

    def on_ready():
        box['states'] = read_state(engines, reader, case['precision'])
    world.h_step(engines, on_ready=on_ready, hook=poison_hook(engines))
    states = box['states']
    Vn = V.numpy()
    ems = [emulate_rank(case, Vn[:, s:e], states[g], engines[g], sel, rounding) for g, (s, e) in enumerate(bounds)]
    out = dict(check_contributions(case, world, engines, states, ems, sel, tol))
    check_reduced(world, engines)
    out['master'], out['master_raw'] = check_apply(case, engines, states, ems, sel, tol)
    check_replication(engines, images)
    out['wrong_refs_far'] = check_sensitivity(case, engines, states, ems, sel, tol)
    out['ki'] = [em['ki'] for em in ems]
    return out, states, ems


def build_engines(case, V, W0, H0, device, backend_factory=None, **kw):
    """One DenseMU per shard, each with its own clones of W[C_g] and H."""
    from torchnmf_amd.engine import DenseMU
    l1, l2 = case['regs']
    engines = []
    for s, e in case_bounds(case):
        be = None if backend_factory is None else backend_factory()
        eng = DenseMU(V[:, s:e].contiguous().to(device), W0[s:e].clone().to(device), H0.clone().to(device), case['beta'], l1, l2,
                      precision=case['precision'], group=GROUP, ar_direct=False, backend=be, **kw)
        if be is not None:
            be.eng = eng
        engines.append(eng)
    return engines
