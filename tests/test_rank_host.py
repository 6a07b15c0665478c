"""Host side of full-ranking evaluation (torchnmf_amd/scoring.py: rank_scores / ranking_metrics, the C entries of
csrc/nmfmu_rank.hip): the argument checks in their order on CPU tensors, the exported symbols and their header text, the status
codes the C entries answer before any device work, the workspace rule, and which models carry the methods.  No GPU."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import ROOT
from torchnmf_amd import _capi, metrics, scoring
from torchnmf_amd.nmf import NMF, NMF2D, NMFD
from torchnmf_amd.plca import PLCA, SIPLCA, SIPLCA2


def _factors(N=6, C=9, R=4, dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    return torch.rand(N, R, generator=g).to(dtype), torch.rand(C, R, generator=g).to(dtype)


def _sparse(N, C):
    return torch.sparse_coo_tensor(torch.tensor([[0, 1], [2, 3]]), torch.tensor([1.0, 0.0]), (N, C))


def test_exports():
    assert metrics.rank_scores is scoring.rank_scores and metrics.ranking_metrics is scoring.ranking_metrics
    assert 'rank_scores' in metrics.__all__ and 'ranking_metrics' in metrics.__all__
    assert scoring.Ranks._fields == ('rows', 'cols', 'ranks', 'scores', 'admissible')
    assert scoring.RANK_SCAN_ABOVE == 24
    src = open(os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'nmfmu_rank.hip')).read()
    assert f'kRkScanAbove = {scoring.RANK_SCAN_ABOVE};' in src
    assert f'kRkRows = {scoring.TILE_ROWS}, kRkCols = {scoring.TILE_COLS};' in src


# ---- the checks, in order -----------------------------------------------------------------------------------------------------
def test_ks_come_first():
    H, W = _factors(R=300)                       # rank too large as well: ks is still what is reported
    for ks in ((0,), (-1,), (2.0,), ('3',), (None,), (True,), (5, 0), 7, None):
        with pytest.raises(ValueError):
            scoring.ranking_metrics(H, W, _sparse(6, 9), ks=ks)
    with pytest.raises(NotImplementedError, match='256'):
        scoring.ranking_metrics(H, W, _sparse(6, 9), ks=(1, 10 ** 6))      # any positive int is a k


def test_rank_before_shapes():
    H, W = _factors(R=257)
    with pytest.raises(NotImplementedError, match='256'):
        scoring.rank_scores(H, W[:, :5], _sparse(6, 8))      # the ranks disagree and heldout has the wrong shape as well
    with pytest.raises(NotImplementedError, match='256'):
        scoring.ranking_metrics(H, W, torch.zeros(6, 9))
    H, W = _factors(R=256)                       # admitted: the next check answers
    with pytest.raises(_capi.NmfmuError):
        scoring.rank_scores(H, W, _sparse(6, 9))


def test_shapes_and_types_before_device():
    H, W = _factors()
    ok = _sparse(6, 9)
    for fn in (scoring.rank_scores, scoring.ranking_metrics):
        with pytest.raises(ValueError):
            fn(H, W[:, :3], ok)
        with pytest.raises(ValueError):
            fn(H[0], W, ok)
        with pytest.raises(ValueError):
            fn(H, W, _sparse(6, 8))
        with pytest.raises(ValueError):
            fn(H, W, torch.zeros(6, 9))              # dense: the wrong type
        with pytest.raises(ValueError):
            fn(H, W, None)
        with pytest.raises(ValueError):
            fn(H, W, ok, exclude=_sparse(5, 9))
        with pytest.raises(ValueError):
            fn(H, W, ok, exclude=torch.zeros(6, 9))
    with pytest.raises(TypeError):
        scoring.rank_scores(H.long(), W, ok)


def test_no_cpu_fallback_comes_last():
    H, W = _factors()
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        scoring.rank_scores(H, W, _sparse(6, 9))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        scoring.rank_scores(H.double(), W.half(), _sparse(6, 9), exclude=_sparse(6, 9))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        scoring.ranking_metrics(H, W, _sparse(6, 9), ks=(1, 200), exclude=_sparse(6, 9))


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    assert '#define NMFMU_ABI_VERSION 10 ' in hdr
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in ('nmfmu_rank_ws', 'nmfmu_rank_pairs', 'nmfmu_rank_pass'):
        assert name in _capi.SIGNATURES and hasattr(raw, name) and name + '(' in hdr
    assert 'nmfmu_rank_pairs / nmfmu_rank_pass / nmfmu_rank_ws (full-ranking evaluation' in hdr      # the ABI comment's line
    assert 'int64_t nmfmu_rank_ws(int64_t n_pairs, int n_rows, int nsplit);' in hdr
    assert _capi.SIGNATURES['nmfmu_rank_ws'][0] is ctypes.c_int64 and lib.nmfmu_rank_ws.restype is ctypes.c_int64
    assert _capi.SIGNATURES['nmfmu_rank_ws'][1][0] is ctypes.c_int64
    assert len(_capi.SIGNATURES['nmfmu_rank_pairs'][1]) == 17 and len(_capi.SIGNATURES['nmfmu_rank_pass'][1]) == 19
    # the scoring entries that were there keep their signatures
    assert len(_capi.SIGNATURES['nmfmu_topk'][1]) == 15 and len(_capi.SIGNATURES['nmfmu_score_pairs'][1]) == 10


def test_rank_ws():
    lib = _capi.load()
    assert lib.nmfmu_rank_ws(10, 5, 1) == 10 * 4                  # one int32 per (range, pair), also for one range
    assert lib.nmfmu_rank_ws(10, 5, 3) == 10 * 3 * 4
    assert lib.nmfmu_rank_ws(2 ** 30, 2 ** 20, 8) == 2 ** 35 > 2 ** 32
    assert lib.nmfmu_rank_ws(0, 5, 3) == 0 and lib.nmfmu_rank_ws(10, 0, 3) == 0 and lib.nmfmu_rank_ws(10, 5, 0) == 0
    assert lib.nmfmu_rank_ws(-1, 5, 3) == 0
    assert lib.nmfmu_rank_ws(10, 5, 3) == lib.nmfmu_rank_ws(10, 5, 3)


def test_c_entries_refuse_before_device_work():
    lib = _capi.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # never dereferenced: every call below is refused on its arguments
    ok = dict(H=p, N=4, row_ids=None, n_rows=4, W=p, C=4, rank=8, ho_rowptr=p, ho_colidx=p, ex_rowptr=None, ex_colidx=None,
              nsplit=1, ws=p, score=p, rnk=p, adm=p, stream=None)

    def pairs(**kw):
        return lib.nmfmu_rank_pairs(*{**ok, **kw}.values())

    def one(pass_=0, form=0, **kw):
        return lib.nmfmu_rank_pass(pass_, form, *{**ok, **kw}.values())
    bad = (dict(H=None), dict(W=None), dict(ho_rowptr=None), dict(ho_colidx=None), dict(ws=None), dict(score=None),
           dict(rnk=None), dict(adm=None), dict(rank=0), dict(nsplit=0), dict(n_rows=0), dict(N=0), dict(C=0), dict(ex_rowptr=p))
    for kw in bad:
        assert pairs(**kw) == _capi.ERR_ARG, kw
        for ps in (0, 1, 2):
            assert one(ps, **kw) == _capi.ERR_ARG, (ps, kw)
    assert pairs(rank=257) == _capi.ERR_UNSUPPORTED and one(1, rank=257) == _capi.ERR_UNSUPPORTED
    assert pairs(rank=257, H=None) == _capi.ERR_ARG
    for ps, form in ((-1, 0), (3, 0), (0, -1), (1, -2)):
        assert one(ps, form) == _capi.ERR_ARG


# ---- the models ---------------------------------------------------------------------------------------------------------------
def test_which_models_rank():
    for cls in (NMF, PLCA):
        assert list(inspect.signature(cls.rank_scores).parameters) == ['self', 'heldout', 'exclude']
        assert list(inspect.signature(cls.ranking_metrics).parameters) == ['self', 'heldout', 'ks', 'exclude']
        assert inspect.signature(cls.ranking_metrics).parameters['ks'].default == (10,)
    for cls in (NMFD, NMF2D, SIPLCA, SIPLCA2):
        assert not hasattr(cls, 'rank_scores') and not hasattr(cls, 'ranking_metrics')
    for m in (NMF((6, 9), rank=4), PLCA((6, 9), rank=4)):
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            m.rank_scores(_sparse(6, 9))
        with pytest.raises(ValueError):
            m.ranking_metrics(_sparse(6, 9), ks=(0,))
        with pytest.raises(ValueError):
            m.rank_scores(_sparse(6, 8))


def test_earlier_signatures_unchanged():
    assert list(inspect.signature(scoring.topk_scores).parameters) == ['H', 'W', 'k', 'rows', 'exclude', '_nsplit', '_fill']
    assert list(inspect.signature(scoring.score_pairs).parameters) == ['H', 'W', 'rows', 'cols']
    assert list(inspect.signature(scoring.rank_scores).parameters)[:4] == ['H', 'W', 'heldout', 'exclude']
    assert list(inspect.signature(scoring.ranking_metrics).parameters) == ['H', 'W', 'heldout', 'ks', 'exclude']
    assert scoring.MAX_K == 128
