"""The normal-equations route of ``ntf.ntf_ccd_sweep(gram_rows=)`` / ``NTF.fit(solver='ccd', gram_rows=)`` on the device
(csrc/nmfmu_sparse_ntf_ccd_gram.hip), on the cases of tests/test_gpu_ntf_ccd.py: 5 and 257 owner rows over 23 x 29 panels.
1. per element, none left out: every coordinate against the float64 minimiser of the row's quadratic, ``Q`` and ``b`` summed in
   float64 from the fp32 ``q``, the coordinates before it from the device's own result and those after it from the old row,
   under the bound of DESIGN.md section 41, counted on the kernel's operations:
       |got - want| <= C u / (1 - C u) (b_k + l1 + sum_j f_j Q_jk) / (Q_kk + l2 + eps),   C = 2 D + c_s + 5,
   D = min(count, part) + parts - 1 (the chain inside a part, then the parts in order: the roundings a term of ``Q_jk`` or
   ``b_k`` can pass through; every term is >= 0), c_s = max(1, r_pad / 64) + 6 (a lane's chain and the butterfly of ``s``), 5 =
   two roundings each in numerator and denominator and the division; ``max(eps, .)`` is 1-Lipschitz;
2. mixed routing, bitwise: rows at or below ``gram_rows`` equal the sweep, rows above it the ``gram_rows=0`` run, repeatable,
   independent of ``_order``;
3. the fit against the float64 loop of tests/test_gpu_ntf_ccd.py."""
import numpy as np
import pytest
import torch

import ccd_emulation as E
from conftest import record, rel_err
from test_gpu_ccd import REG, TOL
from test_gpu_ntf_ccd import _case, _emulate, _fit, _objective, _problem, _run, dev      # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu


def _fractions(got, case, l1, l2, part):
    """|got - want| / bound for every element of the rows with entries (a [rows, rank] array, 0 elsewhere)."""
    F, _, _, ptr, _, _, vals, P_eff = case
    rank = F.shape[1]
    c_s = max(1, (32 if rank <= 32 else 64 if rank <= 64 else 128 if rank <= 128 else 256) // 64) + 6
    new = np.tri(rank, rank, -1, dtype=bool)                      # [k, j]: j < k, already updated when k is
    frac = np.zeros(F.shape)
    for i in np.nonzero(np.diff(ptr))[0]:
        q, count = P_eff[ptr[i]:ptr[i + 1]].astype(np.float64), ptr[i + 1] - ptr[i]
        Q, b = q.T @ q, vals[ptr[i]:ptr[i + 1]].astype(np.float64) @ q
        f = np.where(new, got[i].astype(np.float64), F[i].astype(np.float64))
        np.fill_diagonal(f, 0.0)
        s, den = (f * Q).sum(1), np.diag(Q) + l2 + E.EPS
        want = np.maximum(E.EPS, (b - l1 - s) / den)
        C = 2 * (min(count, part) + -(-count // part) - 1) + c_s + 5
        frac[i] = E.fraction(np.abs(got[i] - want), C * E.U / (1 - C * E.U) * (b + l1 + s) / den)
    return frac


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('rank', [1, 33, 64, 100, 256])      # every r_pad, the padded tail, both gather widths
def test_gram_per_element(dev, rank, mode):
    from torchnmf_amd import _capi
    eps32, worst = np.float32(E.EPS), 0.0
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for rows in (5, 257):
        case = _case(rows, rank)
        F, ptr = case[0], case[3]
        counts, z = np.diff(ptr), E.zero_row(np.diff(ptr))
        rule = _capi.load().nmfmu_sp_ntf_ccd_gram_part(int(counts.sum()), int((counts > 0).sum()), int(counts.max()), rank, cus)
        for reg in ((0.0, 0.0), REG):
            for part in (32, 0):                                  # 32: a 513-entry row is 17 parts, the last of one entry
                got = _run(dev, case, mode, reg, gram_rows=0, _part=part)
                assert np.isfinite(got).all() and (got >= eps32).all()
                frac = _fractions(got, case, *reg, part or rule)
                worst = max(worst, float(frac.max()))
                assert frac.max() <= 1.0, (rows, reg, part, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
                assert got[counts == 0].tobytes() == F[counts == 0].tobytes()      # a row without data is not touched
                assert (got[z] == eps32).all()                                      # the all-zero row ends on the floor
    record('ntf_ccd_gram_per_element', rank=rank, mode=mode, worst_fraction_of_bound=worst)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('rank', [33, 64])
def test_mixed_routing_bitwise(dev, rank, mode):
    case = _case(257, rank)
    counts = np.diff(case[3])
    long = counts > 128
    assert long.any() and (counts[~long] > 0).any()
    # (the library's part length is a function of the set of long rows; a row's bits depend on it, so it is pinned here)
    sweep, gram = _run(dev, case, mode, REG), _run(dev, case, mode, REG, gram_rows=0, _part=64)
    mixed = _run(dev, case, mode, REG, gram_rows=128, _part=64)
    assert mixed[~long].tobytes() == sweep[~long].tobytes() and mixed[long].tobytes() == gram[long].tobytes()
    assert sweep[long].tobytes() != gram[long].tobytes()          # (the two routes are told apart at all)
    assert _run(dev, case, mode, REG, gram_rows=128, _part=64).tobytes() == mixed.tobytes()
    order = torch.from_numpy(np.argsort(counts, kind='stable').astype(np.int32)).to(dev)      # shortest first
    assert _run(dev, case, mode, REG, gram_rows=128, _part=64, _order=order).tobytes() == mixed.tobytes()


@pytest.mark.parametrize('reg, train', [(False, (True,) * 3), (True, (True,) * 3), (False, (True, False, True))])
def test_fit_against_float64(dev, reg, train):
    idx, vals, shape, start = _problem(False)
    kw = dict(alpha=0.07, l1_ratio=0.3) if reg else {}        # l1 = 0.021, l2 = 0.049: REG
    r = REG if reg else (0.0, 0.0)
    trace = [_objective(idx, vals, _emulate(idx, vals, start, 0, *r, train), *r, train)]
    for n_iter in (1, 2, 3):
        got = _fit(dev, False, n_iter, train=train, gram_rows=0, **kw)
        trace.append(_objective(idx, vals, got, *r, train))
    errs = [rel_err(g, w) for g, w in zip(got, _emulate(idx, vals, start, 3, *r, train))]
    record('ntf_ccd_gram_fit_vs_float64', reg=reg, train=list(train), rel_err=errs, objective=trace, tol=TOL)
    assert max(errs) < TOL, errs
    assert all(np.array_equal(g, s) for g, s, on in zip(got, start, train) if not on)          # a frozen factor stays
    assert (np.diff(trace) <= 0).all(), trace                # the float64 objective of the device's factors never rises
