"""CPU tests of tests/sparse_emulation.py: without rounding it is the oracle's sparse algorithm (oracle/mu_oracle.py
``sp_*``) and, for beta in {1, 2}, the dense algorithm on the densified target; its ``csr`` has the properties the engine's
must have; every case of the GPU matrix has the structure it is named for and a finite float64 reference with no element
left out; and the per-element check of tests/test_gpu_sparse_emulated_parity.py fails on eight seeded kernel faults.

The seeded faults against the bars of the older tests (tests/test_gpu_parity.py: relative norm of a whole factor below 1e-4
after 25 iterations on the 120 x 90 rank-5 golden problem, below 2e-2 after 5 iterations at 500 x 700, 7 %, rank 200) --
``test_seeded_faults_against_the_old_bars`` computes this table and asserts it:

    fault                                                   golden problem, 1e-4     rank 200, 2e-2
    (a) last partial group of the 4-entry unroll dropped    fails                    fails
    (b) rank columns >= 192 dropped                         passes (rank 5)          fails
    (c) numerator of an empty owner row left stale          fails (an empty column)  passes (no empty row)
    (d) last rows % 4 owner rows skipped                    fails (90 % 4 = 2)       passes (500, 700 % 4 = 0)
    (e) CSR of V^T sorted by the wrong key                  fails                    fails
    (f) + eps left out of s + eps                           passes                   passes
    (g) the owner's column sums as KL denominators          fails                    fails
    (h) the final Gram chunk dropped                        fails                    fails

(f) passes both old bars, (b), (c) and (d) one of them; all eight fail the per-element check.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
import mu_emulation as E
import sparse_emulation as S
from oracle import mu_oracle as O

BETAS = [1.0, 2.0, 0.5, 1.5, 3.0]


def _small(beta, stored_zero=False, seed=3):
    case = dict(layout='res', beta=beta, N=37, C=29, R=7, axis=0, density=0.1, dups=True, stored_zero=stored_zero,
                zero_owner=False, empty_col=False, nsplit=None, regs=(0.0, 0.0), sample=None, claims=())
    idx, vals, shape, W0, H0 = S.make_problem(case, seed)
    cidx, cvals = S.coalesce(idx, vals, shape)
    return cidx, cvals, shape, W0.double().numpy(), H0.double().numpy()


def _close(a, b, rtol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    scale = np.nanmax(np.abs(b)) if np.isfinite(b).any() else 1.0
    assert np.all(np.nan_to_num(np.abs(a - b)) <= rtol * scale), float(np.nanmax(np.abs(a - b)) / scale)


# ---- the emulation is the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('regs', [(0.0, 0.0), (0.1, 0.2)])
@pytest.mark.parametrize('stored_zero', [False, True])
def test_unrounded_emulation_is_the_oracle(beta, regs, stored_zero):
    l1, l2 = regs
    cidx, cvals, (N, C), W, H = _small(beta, stored_zero)
    gam = O.gamma_of(beta)
    ti, tv, tW, tH = torch.from_numpy(cidx), torch.from_numpy(cvals).double(), torch.from_numpy(W), torch.from_numpy(H)
    csr_h = S.csr(cidx[0], cidx[1], cvals, N)
    csr_w = S.csr(cidx[1], cidx[0], cvals, C)
    Wn, _, _ = S.half_step(csr_w, W, H, beta, gam, l1, l2)
    Wr = O.sp_w_step(ti, tv, (N, C), tW, tH, beta, gam, l1, l2).numpy()
    _close(Wn, Wr)
    Hn, _, _ = S.half_step(csr_h, H, Wn, beta, gam, l1, l2)
    Hr = O.sp_h_step(ti, tv, (N, C), torch.from_numpy(Wr), tH, beta, gam, l1, l2).numpy()
    _close(Hn, Hr)
    vn = S.v_norm(cvals, beta)
    _close(vn, float(O.sp_v_norm(tv, beta)))
    assert np.isnan(vn) == (stored_zero and beta == 1.0)       # 0 log 0, in the reference as well
    div = vn + S.loss_pos(Hn, Wn, beta)[0] - S.loss_neg(csr_h, Hn, Wn, beta)[0]
    _close(np.sqrt(2 * div), O.sp_fit_loss(ti, tv, torch.from_numpy(Wn), torch.from_numpy(Hn), beta), 1e-11)
    pos, neg = O.sp_terms(ti, tv, torch.from_numpy(Wn), torch.from_numpy(Hn), beta)
    _close(S.loss_pos(Hn, Wn, beta)[0], float(pos))
    _close(S.loss_neg(csr_h, Hn, Wn, beta)[0], float(neg))


@pytest.mark.parametrize('beta', [1.0, 2.0])
def test_sparse_numerator_is_the_dense_one_per_element(beta):
    """The reference's own property (its sparse test compares fitted factors) per numerator element."""
    cidx, cvals, (N, C), W, H = _small(beta)
    V = np.zeros((N, C))
    V[cidx[0], cidx[1]] = cvals
    for csr_, X, A, B in ((S.csr(cidx[0], cidx[1], cvals, N), V, H, W), (S.csr(cidx[1], cidx[0], cvals, C), V.T, W, H)):
        em = S.numerator(csr_, A, B, beta)
        dense = E.half_step(X, A, B, beta, 'f16x', rounding=False)
        _close(em['num'], dense['num'])
        if beta == 2.0:
            _close(S.rowmat(A, S.gram(B)[0], len(B))[0], dense['den'], 1e-11)


def test_csr_mirror_properties():
    case = dict(layout='res', beta=1.0, N=37, C=29, R=3, axis=0, density=0.1, dups=True, stored_zero=True, zero_owner=False,
                empty_col=False, nsplit=None, regs=(0.0, 0.0), sample=None, claims=())
    idx, vals, (N, C), _, _ = S.make_problem(case, 11)
    cidx, cvals = S.coalesce(idx, vals, (N, C))
    # duplicates are summed exactly as torch's coalesce sums them; explicit zeros stay
    tc = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals), (N, C)).coalesce()
    assert len(cvals) < len(vals) and (cvals == 0).any()
    assert np.array_equal(tc.indices().numpy(), cidx) and np.array_equal(tc.values().numpy(), cvals)
    rp, ci, cv = S.csr(cidx[0], cidx[1], cvals, N)
    rpt, cit, cvt = S.csr(cidx[1], cidx[0], cvals, C)
    for ptr, n in ((rp, N), (rpt, C)):
        assert ptr.dtype == np.int32 and len(ptr) == n + 1 and ptr[0] == 0 and ptr[-1] == len(cvals)
        assert np.all(np.diff(ptr.astype(np.int64)) >= 0)
    for ptr, col in ((rp, ci), (rpt, cit)):      # sorted by (row, col): columns ascend inside every row
        for a, b in zip(ptr[:-1], ptr[1:]):
            assert np.all(np.diff(col[a:b].astype(np.int64)) > 0)
    dense = np.zeros((N, C), np.float32)
    dense[S.row_of_entry(rp), ci] = cv
    dense_t = np.zeros((C, N), np.float32)
    dense_t[S.row_of_entry(rpt), cit] = cvt
    assert np.array_equal(dense_t, dense.T)       # the CSR of V^T is the transpose of the CSR of V
    # the engine's own host code on the CPU gives the same three arrays for both orientations (its input is the coalesced
    # order, which is what SparseMU and SparseTarget hand it)
    from torchnmf_amd.sparse_autograd import csr_csc
    got_csr, got_csc, _ = csr_csc(torch.from_numpy(cidx[0]), torch.from_numpy(cidx[1]), torch.from_numpy(cvals), N, C)
    for got, want in ((got_csr, (rp, ci, cv)), (got_csc, (rpt, cit, cvt))):
        for g_, w_ in zip(got, want):
            assert g_.numpy().dtype == w_.dtype and np.array_equal(g_.numpy(), w_)
    e = S.csr(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), 5)
    assert np.array_equal(e[0], np.zeros(6, np.int32)) and len(e[1]) == 0 and len(e[2]) == 0


# ---- the case matrix ----------------------------------------------------------------------------------------------------
def test_case_matrix_covers_what_it_must():
    cases = S.parity_cases()
    assert len({c['id'] for c in cases}) == len(cases)
    assert {c['R'] for c in cases} >= {1, 5, 32, 33, 64, 65, 100, 128, 129, 200, 256}
    assert {c['beta'] for c in cases} >= set(BETAS)
    claims = set().union(*(c['claims'] for c in cases))
    need = {'residues', 'empty_row', 'full_row', 'empty_col', 'duplicates', 'stored_zero', 'zero_owner', 'no_entries', 'split',
            'bf16x3', 'bf16', 'skewed', 'sparse1pct', 'rl1', 'rl2', 'rl4', 'rpad32', 'rpad64', 'rpad128', 'rpad256',
            'n_lt4', 'c_lt4', 'n_lt64', 'c_lt64'} | {f'{a}_mod4_{k}' for a in 'nc' for k in (1, 2, 3)}
    assert need <= claims, need - claims
    for beta in BETAS:
        regs = {c['regs'] != (0.0, 0.0) for c in cases if c['beta'] == beta}
        assert regs == {False, True}, beta
    for axis in (0, 1):
        assert any('residues' in c['claims'] and 'full_row' in c['claims'] and c['axis'] == axis for c in cases)
    gen = [c for c in cases if c['beta'] not in (1.0, 2.0)]
    assert any('split' in c['claims'] and 'bf16x3' in c['claims'] for c in gen)
    assert any('split' in c['claims'] and 'bf16' in c['claims'] for c in gen)


@pytest.mark.parametrize('case', S.parity_cases(), ids=lambda c: c['id'])
def test_case_is_what_it_says_and_its_reference_is_finite(case):
    """The claims hold on the generated problem, and the float64 reference of both half-steps and of the loss is finite in
    every element -- nothing has to be excluded from any check (the one NaN: V_norm with a stored zero at beta == 1)."""
    prob = S.make_problem(case)
    for cl in case['claims']:
        assert S.claim_holds(cl, case, prob), cl
    idx, vals, (N, C), W0, H0 = prob
    cidx, cvals = S.coalesce(idx, vals, (N, C))
    beta, (a1, a2) = case['beta'], case['regs']
    l1, l2 = a1 * a2, a1 * (1 - a2)
    gam = O.gamma_of(beta)
    csr_h, csr_w = S.csr(cidx[0], cidx[1], cvals, N), S.csr(cidx[1], cidx[0], cvals, C)
    W, H = W0.double().numpy(), H0.double().numpy()
    Wn, em, den = S.half_step(csr_w, W, H, beta, gam, l1, l2)
    Hn, em2, den2 = S.half_step(csr_h, H, Wn, beta, gam, l1, l2)
    for x in (Wn, Hn, em['num'], em2['num'], em['abs_sum'], em2['abs_sum'], S.numerator_bound(em), S.numerator_bound(em2)):
        assert np.isfinite(x).all()
    for d in (den, den2):
        assert d is None or np.isfinite(d).all()
    assert (Wn >= 0).all() and (Hn >= 0).all()
    neg, nb = S.loss_neg(csr_h, Hn, Wn, beta)
    pos, _ = S.loss_pos(Hn, Wn, beta)
    assert np.isfinite([neg, nb, pos]).all()
    assert np.isnan(S.v_norm(cvals, beta)) == (beta == 1.0 and bool((cvals == 0).any()))


# ---- seeded faults ------------------------------------------------------------------------------------------------------
FAULTS = 'abcdefgh'


def _drop_tail(csr_):
    """(a): every row loses the last partial group of the 4-entry unroll."""
    rp, ci, cv = csr_
    keep = np.concatenate([np.arange(a, a + (b - a) // 4 * 4) for a, b in zip(rp[:-1], rp[1:])] + [np.zeros(0, np.int64)])
    keep = keep.astype(np.int64)
    cnt = np.diff(rp.astype(np.int64)) // 4 * 4
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), ci[keep], cv[keep]


def _wrong_order_csr(rows, cols, vals, n_rows):
    """(e): row pointers of ``rows``, entries left in (col, row) order -- the sort key of the other orientation."""
    order = np.lexsort((rows, cols))
    rp = np.zeros(n_rows + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n_rows))
    return rp.astype(np.int32), cols[order].astype(np.int32), vals[order]


def _faulty_half_step(fault, csr_, owner, panel, beta, gam, l1, l2, prev):
    """One float64 half-step with one kernel fault; ``prev``: what the numerator buffer held before (stale rows)."""
    kind = E.beta_kind(beta)
    em = S.numerator(_drop_tail(csr_) if fault == 'a' else csr_, owner, panel, beta, eps=0.0 if fault == 'f' else S.EPS)
    num = em['num'].copy()
    if fault == 'b':
        num[:, 192:] = 0.0
    if fault == 'c':
        num[em['count'] == 0] = prev[em['count'] == 0]
    if fault == 'd' and len(num) % 4:
        num[-(len(num) % 4):] = prev[-(len(num) % 4):]
    den = kl_den = None
    if kind == 'kl':
        kl_den = S.colsum(owner if fault == 'g' else panel)
    elif kind == 'euc':
        den = S.rowmat(owner, S.gram(panel, drop_last_chunk=fault == 'h')[0], len(panel))[0]
    else:
        den = S.generic_den_exact(owner, panel, beta)
    return E.apply(owner, num, den, beta, gam, l1, l2, kl_den=kl_den), num


def _fit(cidx, cvals, shape, W, H, beta, iters, l1, l2, fault=None):
    N, C = shape
    gam = O.gamma_of(beta)
    csr_h = S.csr(cidx[0], cidx[1], cvals, N)
    csr_w = _wrong_order_csr(cidx[1], cidx[0], cvals, C) if fault == 'e' else S.csr(cidx[1], cidx[0], cvals, C)
    pw, ph = np.ones_like(W), np.ones_like(H)
    for _ in range(iters):
        with np.errstate(all='ignore'):
            W, pw = _faulty_half_step(fault, csr_w, W, H, beta, gam, l1, l2, pw)
            H, ph = _faulty_half_step(fault, csr_h, H, W, beta, gam, l1, l2, ph)
    return W, H


def _rel(a, b):
    d = np.linalg.norm(a - b) / np.linalg.norm(b)
    return d if np.isfinite(d) else np.inf


def _case(prefix):
    return next(c for c in S.parity_cases() if c['id'].startswith(prefix))


def _per_element(fault, case):
    """Largest numerator, Gram and master excess of one faulty W + H iteration of ``case`` over the bounds of the GPU test
    (> 1 fails), each half-step judged from the state it starts from."""
    idx, vals, (N, C), W0, H0 = S.make_problem(case)
    cidx, cvals = S.coalesce(idx, vals, (N, C))
    beta = case['beta']
    gam = O.gamma_of(beta)
    csr_h, csr_w = S.csr(cidx[0], cidx[1], cvals, N), S.csr(cidx[1], cidx[0], cvals, C)
    bad_w = _wrong_order_csr(cidx[1], cidx[0], cvals, C) if fault == 'e' else csr_w
    W, H = W0.double().numpy(), H0.double().numpy()
    worst = 0.0
    for good, bad, own, pan in ((csr_w, bad_w, W, H), (csr_h, csr_h, H, W)):
        ref, em, den = S.half_step(good, own, pan, beta, gam)
        with np.errstate(all='ignore'):
            got, num = _faulty_half_step(fault, bad, own, pan, beta, gam, 0.0, 0.0, np.ones_like(own))
        nb = S.numerator_bound(em)
        worst = max(worst, S.bound_err(num, em['num'], nb).max())
        db = 0.0
        if beta == 2.0:
            g, gb = S.gram(pan)
            worst = max(worst, S.bound_err(S.gram(pan, drop_last_chunk=fault == 'h')[0], g, gb).max())
            db = S.rowmat(own, g, len(pan))[1]
        allow = E.apply_allowance(ref, em['num'], den, nb, db, beta, gam)
        worst = max(worst, E.elem_err(got, ref, allow).max() / (S.APPLY_OPS * S.U))
    return worst


PER_ELEMENT_CASE = {'a': 'res-b1-61x130r5', 'b': 'rand-b1-70x90r200', 'c': 'res-b1-61x130r5', 'd': 'res-b1-61x130r5',
                    'e': 'res-b2-61x130r33', 'f': 'res-b1-61x130r5-dup-z-zo-ec', 'g': 'rand-b1-70x90r64',
                    'h': 'rand-b2-90x70r100'}


@pytest.mark.parametrize('fault', FAULTS)
def test_seeded_fault_fails_the_per_element_check(fault):
    case = _case(PER_ELEMENT_CASE[fault])
    assert _per_element(None, case) <= 1.0          # the check passes the float64 algorithm itself
    assert _per_element(fault, case) > 1.0


def test_seeded_faults_against_the_old_bars():
    """The table of the module docstring: which faults the relative-norm bars of tests/test_gpu_parity.py let through."""
    g = load_golden('g9_sparse')
    gi, gv = S.coalesce(g['indices'], g['values'], tuple(g['shape']))
    golden = (gi, gv, tuple(int(x) for x in g['shape']), g['W0'].astype(np.float64), g['H0'].astype(np.float64))
    assert golden[2] == (120, 90) and golden[3].shape[1] == 5
    tg = torch.Generator().manual_seed(200)           # test_fit_sparse_equals_dense at rank 200
    Vd = torch.rand(500, 700, generator=tg)
    Vd = torch.where(Vd > 0.93, Vd, torch.zeros(()))
    W0, H0 = torch.randn(700, 200, generator=tg).abs(), torch.randn(500, 200, generator=tg).abs()
    sp = Vd.to_sparse().coalesce()
    big = (sp.indices().numpy(), sp.values().numpy(), (500, 700), W0.double().numpy(), H0.double().numpy())
    passes = {}
    for name, prob, iters, l1, l2, bar in (('golden', golden, 25, 0.0, 0.0, 1e-4), ('rank200', big, 5, 0.05, 0.05, 2e-2)):
        for beta in (1.0, 2.0):
            Wr, Hr = _fit(*prob, beta, iters, l1, l2)
            for f in FAULTS:
                if (f in 'fg' and beta != 1.0) or (f == 'h' and beta != 2.0):
                    continue              # faults of one beta's code only
                W, H = _fit(*prob, beta, iters, l1, l2, fault=f)
                ok = _rel(W, Wr) < bar and _rel(H, Hr) < bar
                passes[(f, name)] = passes.get((f, name), True) and ok
    got = {name: ''.join(sorted(f for f in FAULTS if passes[(f, name)])) for name in ('golden', 'rank200')}
    assert got == {'golden': 'bf', 'rank200': 'cdf'}, got
