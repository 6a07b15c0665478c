"""Host side of scoring (torchnmf_amd/scoring.py, the C entries of csrc/nmfmu_score.hip): the argument checks in their order
on CPU tensors, choose_nsplit, the workspace rule, the exported symbols and the status codes the C entries answer before any
device work, and which models carry predict / topk.  No GPU."""
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
    assert scoring.MAX_K == 128 and scoring.TILE_ROWS == 64 and scoring.TILE_COLS == 128
    assert metrics.score_pairs is scoring.score_pairs and metrics.topk_scores is scoring.topk_scores
    assert 'score_pairs' in metrics.__all__ and 'topk_scores' in metrics.__all__


# ---- the checks, in order -----------------------------------------------------------------------------------------------------
def test_k_checks_come_first():
    H, W = _factors(R=300)                       # rank too large as well: k is still what is reported
    for k in (0, -1, 2.0, '3', None, True):
        with pytest.raises(ValueError):
            scoring.topk_scores(H, W, k)
    with pytest.raises(NotImplementedError, match='128'):
        scoring.topk_scores(H, W, scoring.MAX_K + 1)


def test_rank_before_shapes():
    H, W = _factors(R=257)
    with pytest.raises(NotImplementedError, match='256'):
        scoring.topk_scores(H, W[:, :5], 3)      # the ranks also disagree
    with pytest.raises(NotImplementedError, match='256'):
        scoring.score_pairs(H, W, torch.zeros(2, 2), torch.zeros(3))
    H, W = _factors(R=256)                       # admitted: the next check answers
    with pytest.raises(_capi.NmfmuError):
        scoring.topk_scores(H, W, 3)


def test_shapes_before_dtypes():
    H, W = _factors()
    bad = torch.zeros(3)                         # a float index as well
    with pytest.raises(ValueError):
        scoring.topk_scores(H, W[:, :3], 2, rows=bad)
    with pytest.raises(ValueError):
        scoring.topk_scores(H, W, 2, exclude=_sparse(6, 8), rows=bad)
    with pytest.raises(ValueError):
        scoring.topk_scores(H, W, 2, rows=torch.zeros(2, 2))
    with pytest.raises(ValueError):
        scoring.topk_scores(H[0], W, 2)
    with pytest.raises(ValueError):
        scoring.score_pairs(H, W, torch.zeros(3), torch.zeros(4))
    with pytest.raises(ValueError):
        scoring.score_pairs(H, W, torch.zeros(2, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        scoring.score_pairs(H, W[:, :3], torch.zeros(3), torch.zeros(3))


def test_dtypes_before_device():
    H, W = _factors()
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.int16)):
        with pytest.raises(TypeError):
            scoring.topk_scores(H, W, 2, rows=bad)
        with pytest.raises(TypeError):
            scoring.score_pairs(H, W, torch.zeros(3, dtype=torch.int64), bad)
    with pytest.raises(TypeError):
        scoring.topk_scores(H, W, 2, exclude=torch.zeros(6, 9))


def test_no_cpu_fallback_comes_last():
    H, W = _factors()
    for dt in (torch.int32, torch.int64):
        far = torch.full((3,), 1000, dtype=dt)   # out of range as well: not looked at before the device check
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            scoring.score_pairs(H, W, far, far)
        with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
            scoring.topk_scores(H, W, 3, rows=far)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        scoring.topk_scores(H.double(), W.half(), 3, exclude=_sparse(6, 9))
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        scoring.score_pairs(H, W, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))


# ---- choose_nsplit ------------------------------------------------------------------------------------------------------------
def test_choose_nsplit():
    TR, TC = scoring.TILE_ROWS, scoring.TILE_COLS
    for n_rows in (1, TR - 1, TR, TR + 1, 1000, 65536, 10 ** 7):
        for C in (1, TC - 1, TC, TC + 1, 16384, 10 ** 6):
            for n_cu in (1, 64, 256):
                s = scoring.choose_nsplit(n_rows, C, n_cu)
                tiles, blocks = -(-C // TC), -(-n_rows // TR)
                assert isinstance(s, int) and 1 <= s <= tiles
                assert s == scoring.choose_nsplit(n_rows, C, n_cu)                       # pure
                assert s == tiles or s * blocks >= 2 * n_cu                              # about two workgroups per CU ...
                assert s == 1 or (s - 1) * blocks < 2 * n_cu                             # ... and no more splits than that needs
    assert scoring.choose_nsplit(65536, 16384, 256) == 1
    assert scoring.choose_nsplit(64, 16384, 256) == 128
    assert scoring.choose_nsplit(64, 100, 256) == 1


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    lib = _capi.load()
    assert lib.nmfmu_abi_version() == _capi.ABI_VERSION == 10
    hdr = open(os.path.join(ROOT, 'include', 'nmfmu.h')).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in ('nmfmu_score_pairs', 'nmfmu_topk_ws', 'nmfmu_topk'):
        assert name in _capi.SIGNATURES and hasattr(raw, name) and name + '(' in hdr
    assert _capi.SIGNATURES['nmfmu_topk_ws'][0] is ctypes.c_int64 and lib.nmfmu_topk_ws.restype is ctypes.c_int64
    assert len(_capi.SIGNATURES['nmfmu_topk'][1]) == 15 and len(_capi.SIGNATURES['nmfmu_score_pairs'][1]) == 10


def test_topk_ws():
    lib = _capi.load()
    assert lib.nmfmu_topk_ws(10, 5, 1) == 0                       # one range: the partial kernel writes the outputs
    assert lib.nmfmu_topk_ws(10, 5, 3) == 10 * 3 * 5 * 8          # (value, index) per (row, range, position)
    assert lib.nmfmu_topk_ws(2 ** 24, 128, 64) == 2 ** 24 * 128 * 64 * 8 > 2 ** 32
    assert lib.nmfmu_topk_ws(0, 5, 3) == 0 and lib.nmfmu_topk_ws(10, 0, 3) == 0
    assert lib.nmfmu_topk_ws(10, 5, 3) == lib.nmfmu_topk_ws(10, 5, 3)


def test_c_entries_refuse_before_device_work():
    lib = _capi.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # never dereferenced: every call below is refused on its arguments
    ok = dict(H=p, N=4, row_ids=None, n_rows=4, W=p, C=4, rank=8, k=2, rowptr=None, colidx=None, nsplit=1, ws=None, val=p,
              idx=p, stream=None)

    def topk(**kw):
        return lib.nmfmu_topk(*{**ok, **kw}.values())
    for kw in (dict(H=None), dict(W=None), dict(val=None), dict(idx=None), dict(rank=0), dict(k=0), dict(nsplit=0),
               dict(n_rows=0), dict(N=0), dict(C=0), dict(rowptr=p), dict(nsplit=2)):
        assert topk(**kw) == _capi.ERR_ARG, kw
    assert topk(rank=257) == _capi.ERR_UNSUPPORTED and topk(k=129) == _capi.ERR_UNSUPPORTED
    assert topk(rank=257, H=None) == _capi.ERR_ARG

    def pairs(rows=p, cols=p, n=3, H=p, N=4, W=p, C=4, rank=8, out=p):
        return lib.nmfmu_score_pairs(rows, cols, n, H, N, W, C, rank, out, None)
    for kw in (dict(rows=None), dict(cols=None), dict(H=None), dict(W=None), dict(out=None), dict(rank=0), dict(n=-1),
               dict(N=0), dict(C=0)):
        assert pairs(**kw) == _capi.ERR_ARG, kw
    assert pairs(rank=257) == _capi.ERR_UNSUPPORTED
    assert pairs(n=0) == _capi.OK                # nothing to do, nothing launched


# ---- the models ---------------------------------------------------------------------------------------------------------------
def test_which_models_score():
    for cls in (NMF, PLCA):
        assert callable(getattr(cls, 'predict')) and callable(getattr(cls, 'topk'))
    for cls in (NMFD, NMF2D, SIPLCA, SIPLCA2):
        assert not hasattr(cls, 'predict') and not hasattr(cls, 'topk')
    assert list(inspect.signature(NMF.predict).parameters) == ['self', 'rows', 'cols']
    assert list(inspect.signature(NMF.topk).parameters) == ['self', 'k', 'rows', 'exclude']
    assert list(inspect.signature(PLCA.predict).parameters) == ['self', 'rows', 'cols', 'norm']
    assert list(inspect.signature(PLCA.topk).parameters) == ['self', 'k', 'rows', 'exclude']
    m = NMF((6, 9), rank=4)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        m.topk(3)
    with pytest.raises(ValueError):
        m.topk(0)
    p = PLCA((6, 9), rank=4)
    with pytest.raises(_capi.NmfmuError, match='no CPU fallback'):
        p.predict(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), norm=3.0)
