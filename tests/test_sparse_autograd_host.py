"""Host logic of ``sparse_beta_div`` (no GPU): the segment planner against a brute-force loop, the CSC -> CSR permutation, the
workspace rule, every argument error, and the float64 formulas of tests/sparse_autograd_reference.py against the
reference's recorded float64 loss and gradients (golden g19, part (a))."""
import numpy as np
import pytest
import torch

import sparse_autograd_reference as A
from conftest import load_golden

ROW_COUNTS = [0, 1, 511, 512, 513, 1024, 1025]


def _rowptr(counts):
    rp = torch.zeros(len(counts) + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
    return rp


def _brute(counts, chunk):
    """(row, p_begin, p_end, slot) per segment, (row, first slot, segments) per split row, slots used."""
    seg, multi, p, slot = [], [], 0, 0
    for row, n in enumerate(counts):
        cuts = [(a, min(a + chunk, n)) for a in range(0, n, chunk)] or [(0, 0)]
        if len(cuts) > 1:
            multi.append((row, slot, len(cuts)))
        for a, b in cuts:
            seg.append((row, p + a, p + b, slot if len(cuts) > 1 else -1))
            slot += len(cuts) > 1
        p += n
    return seg, multi, slot


@pytest.mark.parametrize('chunk', [1, 4, 512])
def test_planner_against_brute_force(chunk):
    from torchnmf_amd.sparse_autograd import plan_segments, plan_worklist
    for counts in (ROW_COUNTS, ROW_COUNTS[::-1], [0, 0, 0], [513], [3, 0, 1025, 0, 512]):
        rp = _rowptr(counts)
        seg_ref, multi_ref, slots = _brute(counts, chunk)
        seg3 = plan_segments(rp, chunk)
        assert seg3.dtype == torch.int32 and seg3.tolist() == [list(s[:3]) for s in seg_ref]
        seg, multi, n_ws = plan_worklist(rp, chunk)
        assert seg.dtype == torch.int32 and multi.dtype == torch.int32
        assert seg.tolist() == [list(s) for s in seg_ref]
        assert multi.tolist() == [list(m) for m in multi_ref] and n_ws == slots
        # a pure function of (rowptr, chunk); every entry in exactly one segment, every row in at least one, none too long
        assert torch.equal(plan_segments(rp.clone(), chunk), seg3)
        length = seg3[:, 2] - seg3[:, 1]
        assert int(length.max()) <= chunk and int(length.sum()) == sum(counts)
        assert sorted(set(seg3[:, 0].tolist())) == list(range(len(counts)))


def test_perm_round_trips_csc_to_csr():
    from torchnmf_amd.sparse_autograd import csr_csc
    g = torch.Generator().manual_seed(3)
    N, C, n = 23, 17, 300
    ii, jj = torch.randint(0, N, (n,), generator=g), torch.randint(0, C, (n,), generator=g)
    vals = (torch.randint(1, 1024, (n,), generator=g).float() / 1024)
    V = torch.sparse_coo_tensor(torch.stack([ii, jj]), vals, (N, C))
    assert V.coalesce()._nnz() < n                                   # the pattern has duplicates
    V = V.coalesce()
    idx, v = V.indices(), V.values()
    (rowptr, colidx, vcsr), (colptr, rowidx, vcsc), perm = csr_csc(idx[0], idx[1], v, N, C)
    nnz = v.numel()
    assert perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(nnz))
    assert torch.equal(vcsc, vcsr[perm.long()])
    rows_csr = torch.repeat_interleave(torch.arange(N), torch.diff(rowptr.long()))
    cols_csc = torch.repeat_interleave(torch.arange(C), torch.diff(colptr.long()))
    assert torch.equal(rows_csr[perm.long()], rowidx.long())         # CSC entry p is CSR entry perm[p]: same row,
    assert torch.equal(colidx.long()[perm.long()], cols_csc)         # same column
    assert torch.equal(V.to_dense().t()[cols_csc, rowidx.long()], vcsc)
    assert bool((torch.diff(cols_csc * N + rowidx.long()) > 0).all())     # sorted by (column, row), no duplicates


def test_workspace_rule():
    from torchnmf_amd import _capi
    from torchnmf_amd.sparse_autograd import plan_worklist, workspace_floats
    lib = _capi.load()
    for counts, chunk in ((ROW_COUNTS, 512), (ROW_COUNTS, 4), ([0, 1, 2], 4)):
        _, multi, n_ws = plan_worklist(_rowptr(counts), chunk)
        assert n_ws == int(multi[:, 2].sum()) if multi.numel() else n_ws == 0
        for r_pad in (32, 64, 128, 256):
            assert lib.nmfmu_sp_div_backward_ws(n_ws, r_pad) == workspace_floats(n_ws, r_pad) == n_ws * r_pad
    assert lib.nmfmu_sp_div_backward_ws(0, 64) == 0 and lib.nmfmu_sp_div_backward_ws(-1, 64) == 0


def _sparse(N=6, C=5, negative=False):
    V = torch.zeros(N, C)
    V[1, 2], V[3, 0], V[5, 4] = 0.5, 1.5, (-0.25 if negative else 0.25)
    return V.to_sparse()


def test_argument_errors():
    from torchnmf_amd import _capi
    from torchnmf_amd.metrics import SparseTarget, sparse_beta_div
    V = _sparse()
    H, W = torch.rand(6, 3), torch.rand(5, 3)
    for beta in (0, -1.0):
        with pytest.raises(ValueError, match='beta <= 0'):
            sparse_beta_div(H, W, V, beta)
    for beta in (0.5, 1.5, 3):
        with pytest.raises(NotImplementedError, match=r'dense pass over N x C.*beta_div\(m\(\), V\.to_dense\(\), beta\)'):
            sparse_beta_div(H, W, V, beta)
    with pytest.raises(NotImplementedError, match='rank 257'):
        sparse_beta_div(torch.rand(6, 257), torch.rand(5, 257), V, 2)
    with pytest.raises(_capi.NmfmuError):                  # CPU tensors
        sparse_beta_div(H, W, V, 2)
    with pytest.raises(_capi.NmfmuError):
        SparseTarget(V)
    with pytest.raises(AssertionError, match='Target should be non-negative.'):
        SparseTarget(_sparse(negative=True))
    with pytest.raises(AssertionError, match='Target should be non-negative.'):
        sparse_beta_div(H, W, _sparse(negative=True), 1)
    with pytest.raises(AssertionError):                    # a dense target
        sparse_beta_div(H, W, V.to_dense(), 2)
    with pytest.raises(AssertionError):
        SparseTarget(V.to_dense())
    with pytest.raises(AssertionError):                    # shape mismatches
        sparse_beta_div(torch.rand(7, 3), W, V, 2)
    with pytest.raises(AssertionError):
        sparse_beta_div(H, torch.rand(5, 4), V, 2)
    with pytest.raises(AssertionError):
        sparse_beta_div(H, torch.rand(4, 3), V, 1)


@pytest.mark.parametrize('beta', [1, 2])
def test_float64_formulas_against_golden(beta):
    g = load_golden('g19_sparse_autograd')
    shape = tuple(int(x) for x in g['shape'])
    for up in (1.0, -2.5):
        ref = A.evaluate(g['indices'], g['values'], shape, g['H0'], g['W0'], beta, up=up)
        loss, gH, gW = float(g[f'a_loss_b{beta}']), g[f'a_gH_b{beta}'], g[f'a_gW_b{beta}']
        assert abs(ref['loss'] - loss) <= 1e-14 * abs(loss)
        for got, want in ((ref['gH'], up * gH), (ref['gW'], up * gW)):
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
        for k in ('loss_bound', 'gH_bound', 'gW_bound'):
            assert np.all(np.isfinite(ref[k])) and np.all(np.asarray(ref[k]) > 0)
