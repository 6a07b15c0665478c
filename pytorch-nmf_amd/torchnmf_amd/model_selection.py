"""Model selection by masked cross-validation: which rank, how much regularisation (``holdout_masks``, ``cross_validate``).

Wold-style holdout (Owen & Perry 2009; Kanagal & Sindhwani 2010): deal the entries of ``V`` to ``K`` folds, fit on the entries
off a fold with the held-out ones weighted 0, score the fit on the held-out entries, and take the candidate whose held-out loss
per unit of weight is the smallest.  That is ``len(ranks) * len(alphas) * folds * n_init`` small weighted fits of ONE target:
per rank they are one ``batched.BatchedNMF`` fit -- the target shared through a batch stride of 0, the ``K`` fold masks shared
through ``weight_index``, ``alpha`` per problem -- so nothing of size ``B x N x C`` is ever allocated and no fit pays the launch
gaps of a loop of ``NMF.fit(V, weights=train_k)`` calls.
"""
from __future__ import annotations

from collections.abc import Iterable
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _capi
from .batched import MAX_RANK, BatchedNMF, target_like
from .wmu import check_weights

__all__ = ['holdout_masks', 'cross_validate', 'CVResult', 'problem_layout', 'draw_starts', 'summarise']


def holdout_masks(shape, folds: int, generator: Optional[torch.Generator] = None, device=None, weights=None):
    """``(train, test)``: two fp32 ``(folds, N, C)`` tensors on ``device`` (``weights``' device by default, else the CPU).

    Every entry that counts -- ``weights > 0``, or every entry without ``weights`` -- is dealt to exactly one fold by a
    permutation drawn from ``generator`` (the CPU generator by default), so the fold sizes differ by at most one.  ``test[k]``
    is the base weight (``weights``, or 1) on fold ``k`` and 0 elsewhere, ``train[k]`` the base weight off fold ``k``:
    ``train[k] + test[k] == base`` and ``sum_k test[k] == base`` exactly."""
    N, Cc = (int(x) for x in shape)
    folds = int(folds)
    if weights is not None:
        base = check_weights(target_like((N, Cc), weights.device if isinstance(weights, Tensor) else 'cpu'), weights)
        device = base.device if device is None else device
        base = base.cpu()
    else:
        base = torch.ones(N, Cc, dtype=torch.float32)
    counted = (base > 0).reshape(-1).nonzero().reshape(-1)
    if folds < 2 or folds > max(int(counted.numel()), 1):
        raise ValueError(f'folds must lie in [2, the number of entries that count = {int(counted.numel())}], got {folds}')
    where = generator.device if generator is not None else 'cpu'
    perm = torch.randperm(int(counted.numel()), generator=generator, device=where).cpu()
    fold = torch.full((N * Cc,), -1, dtype=torch.int64)
    fold[counted[perm]] = torch.arange(int(counted.numel())) % folds
    on = fold.reshape(1, N, Cc) == torch.arange(folds).reshape(folds, 1, 1)
    zero = torch.zeros((), dtype=torch.float32)
    test = torch.where(on, base, zero)
    train = torch.where(on, zero, base)
    return train.to(device), test.to(device)


@dataclass
class CVResult:
    """What ``cross_validate`` returns.  ``n_iter`` (int64), ``train_loss`` and ``test_loss`` (float64) are CPU tensors
    ``[len(ranks), len(alphas), folds, n_init]``; ``n_test`` ``[folds]`` holds the held-out weight totals; ``mean_test``
    ``[len(ranks), len(alphas)]`` is the mean over folds and starts of ``test_loss / n_test`` (a NaN never wins);
    ``best = (rank, alpha)`` is its argmin; ``masks = (train, test)`` lets a caller refit."""
    ranks: Tuple[int, ...]
    alphas: Tuple[float, ...]
    n_iter: Tensor
    train_loss: Tensor
    test_loss: Tensor
    n_test: Tensor
    mean_test: Tensor
    best: Tuple[int, float]
    masks: Tuple[Tensor, Tensor]


def problem_layout(n_alpha: int, folds: int, n_init: int):
    """``(alpha index, fold, start)`` of every problem of a rank's batch, three int64 ``[n_alpha * folds * n_init]`` tensors: the
    batch is ``[alpha][fold][start]`` flattened, the start fastest."""
    idx = torch.arange(n_alpha * folds * n_init)
    return idx // (folds * n_init), (idx // n_init) % folds, idx % n_init


def draw_starts(B: int, N: int, Cc: int, R: int, generator: Optional[torch.Generator]):
    """``(W0 [B, C, R], H0 [B, N, R])`` from ``|N(0, 1)|`` with ``generator`` (on its device, the CPU by default), W first."""
    where = generator.device if generator is not None else 'cpu'
    W0 = torch.randn(B, Cc, R, generator=generator, device=where).abs()
    H0 = torch.randn(B, N, R, generator=generator, device=where).abs()
    return W0, H0


@torch.no_grad()
def cross_validate(V: Tensor, ranks, beta: float = 1, folds: int = 5, n_init: int = 1, alpha=0, l1_ratio: float = 0,
                   tol: float = 1e-4, max_iter: int = 200, generator: Optional[torch.Generator] = None,
                   weights=None) -> CVResult:
    """Masked cross-validation of ``NMF`` over ``ranks`` and ``alpha`` (a float or a sequence of candidates) on a dense fp32
    device tensor ``V (N, C)``; ``weights`` (as in ``NMF.fit``) are base weights: an entry of weight 0 is never used.

    ``holdout_masks`` deals the entries to ``folds`` folds; per rank ONE ``BatchedNMF`` fit runs the ``len(alphas) * folds *
    n_init`` problems on the shared ``V`` with ``weights=train`` and ``weight_index`` = every problem's fold, from starts drawn
    from ``|N(0, 1)|`` with ``generator`` (masks first, then per rank W and H), and one ``loss(V, beta, weights=test, ...)``
    call scores it.  Returns a ``CVResult``; ``best`` minimises the held-out loss per unit of held-out weight.

    Against a loop of ``NMF.fit(V, weights=train_k)`` + ``weighted_beta_div`` calls: see DESIGN section 32 -- the batch wins
    where one problem cannot fill the device; at a target that fills it alone the loop's launches are hidden and the two are
    close (both run the same exact-fp32 weighted tile)."""
    if not isinstance(V, Tensor):
        raise ValueError(f'the target must be a tensor (N, C), got {type(V).__name__}')
    if V.is_sparse:
        raise NotImplementedError('cross_validate takes a dense target')
    if V.dim() != 2:
        raise ValueError(f'the target must be (N, C), got {tuple(V.shape)}')
    ranks = tuple(int(r) for r in (ranks if isinstance(ranks, Iterable) else (ranks,)))
    alphas = tuple(float(a) for a in (alpha.reshape(-1).tolist() if isinstance(alpha, Tensor) else
                                      alpha if isinstance(alpha, Iterable) else (alpha,)))
    folds, n_init = int(folds), int(n_init)
    if not ranks or not alphas or min(ranks) < 1 or n_init < 1:
        raise ValueError(f'cross_validate needs ranks >= 1, at least one alpha and n_init >= 1; got ranks {ranks}, alphas '
                         f'{alphas}, n_init {n_init}')
    if max(ranks) > MAX_RANK:
        raise NotImplementedError(f'cross_validate: rank {max(ranks)} > {MAX_RANK}, the limit of the exact-fp32 kernels')
    if V.dtype != torch.float32:
        raise NotImplementedError(f'cross_validate takes an fp32 target, got {V.dtype} (cast it once with V.float())')
    N, Cc = V.shape
    train, test = holdout_masks((N, Cc), folds, generator, device=V.device, weights=weights)
    if V.device.type != 'cuda':
        raise _capi.NmfmuError(f'cross_validate: the target lives on {V.device}; torchnmf_amd computes on an MI355X only -- '
                               f'move it with .cuda() (there is no CPU fallback)')
    a_of, k_of, _ = problem_layout(len(alphas), folds, n_init)
    B = a_of.numel()
    index = k_of.to(device=V.device, dtype=torch.int32)
    alpha_b = torch.tensor(alphas, dtype=torch.float64)[a_of]
    shape = (len(ranks), len(alphas), folds, n_init)
    n_iter = torch.empty(shape, dtype=torch.int64)
    train_loss = torch.empty(shape, dtype=torch.float64)
    test_loss = torch.empty(shape, dtype=torch.float64)
    for i, R in enumerate(ranks):
        W0, H0 = draw_starts(B, N, Cc, R, generator)
        m = BatchedNMF(W=W0, H=H0).to(V.device)
        n = m.fit(V, beta=beta, tol=tol, max_iter=max_iter, alpha=alpha_b, l1_ratio=l1_ratio, weights=train,
                  weight_index=index)
        n_iter[i] = n.reshape(shape[1:])
        train_loss[i] = m.last_loss.cpu().reshape(shape[1:])
        test_loss[i] = m.loss(V, beta, weights=test, weight_index=index).cpu().reshape(shape[1:])
    n_test = test.double().sum(dim=(1, 2)).cpu()
    mean_test, best = summarise(test_loss, n_test, ranks, alphas)
    return CVResult(ranks, alphas, n_iter, train_loss, test_loss, n_test, mean_test, best, (train, test))


def summarise(test_loss: Tensor, n_test: Tensor, ranks, alphas):
    """``(mean_test [ranks, alphas], best (rank, alpha))`` from ``test_loss [ranks, alphas, folds, n_init]`` and the held-out
    weight totals ``[folds]``; a NaN mean never wins, as in ``BatchedNMF.best``."""
    mean_test = (test_loss / n_test.reshape(1, 1, -1, 1)).mean(dim=(2, 3))
    flat = torch.where(torch.isnan(mean_test), torch.full_like(mean_test, float('inf')), mean_test).reshape(-1)
    at = int(flat.argmin())
    return mean_test, (ranks[at // len(alphas)], alphas[at % len(alphas)])
