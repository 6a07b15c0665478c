"""ARD-NMF: automatic relevance determination for the beta-divergence (Tan & Fevotte, IEEE TPAMI 2013) on the dense MU engine.

Over-provision the rank, tie column ``k`` of ``W`` and column ``k`` of ``H`` to a shared scale ``lambda_k`` and let the
multiplicative update shrink the components the data does not need (conventions of this code base: ``V ~ H W^T``,
``H [N, R]``, ``W [C, R]``)::

    Obj = D_beta(V | H W^T) / phi + sum_k [ (f(W[:, k]) + f(H[:, k]) + b) / lambda_k + c log lambda_k ]
    f(x) = ||x||_1,       c = N + C + a + 1          prior 'l1' (exponential)
    f(x) = 1/2 ||x||^2,   c = (N + C) / 2 + a + 1    prior 'l2' (half-normal)

One iteration = W half-step, H half-step, relevance update.  A half-step is ``nmfmu_mu_partial`` -- the numerator and
denominator slabs on whichever fused kernel the shape selects, in any precision mode, exactly as in ``NMF.fit`` -- followed by
``nmfmu_ard_apply``, the apply stage with the per-component penalty ``pen[k] = phi / lambda_k`` in its denominator
(``'l1'``: ``pos += pen[k]``; ``'l2'``: ``pos += pen[k] * f``) and the exponent ``ard_exponent(beta, prior)``.  The relevance
update ``lambda_k = (f(W[:, k]) + f(H[:, k]) + b) / c`` is one small launch (``nmfmu_ard_relevance``) that also leaves the
next penalties and the largest relative change of ``lambda`` on the device: the loop has no host sync of its own.
"""
from __future__ import annotations

import math

import torch

from .engine import DenseMU, mu_gamma

PRIORS = ('l1', 'l2')


def ard_exponent(beta: float, prior: str) -> float:
    """Exponent of the multiplicative update under which ``Obj`` does not increase: the paper's gamma(beta) for 'l1'
    (``engine.mu_gamma``), ``1 / (3 - beta)`` (beta <= 2) or ``1 / (beta - 1)`` (beta > 2) for 'l2'."""
    beta = float(beta)
    if prior == 'l1':
        return mu_gamma(beta)
    return 1.0 / (3.0 - beta) if beta <= 2 else 1.0 / (beta - 1.0)


def ard_c(n_rows: int, n_cols: int, a: float, prior: str) -> float:
    """``c`` of the objective: ``N + C + a + 1`` ('l1'), ``(N + C) / 2 + a + 1`` ('l2')."""
    return (n_rows + n_cols + a + 1.0) if prior == 'l1' else ((n_rows + n_cols) / 2.0 + a + 1.0)


def default_b(v_mean: float, rank: int, a: float, prior: str) -> float:
    """``b`` by moment matching ``mean(V) = R E[w] E[h]``: ``sqrt((a - 1)(a - 2) mean(V) / R)`` ('l1'),
    ``pi (a - 1) mean(V) / (2 R)`` ('l2')."""
    if prior == 'l1':
        return math.sqrt((a - 1.0) * (a - 2.0) * v_mean / rank)
    return math.pi * (a - 1.0) * v_mean / (2.0 * rank)


def check_prior(prior: str, a: float) -> None:
    if prior not in PRIORS:
        raise ValueError(f"prior must be 'l1' or 'l2', got {prior!r}")
    low = 2.0 if prior == 'l1' else 1.0
    if not float(a) > low:          # (a NaN fails too)
        raise ValueError(f"a must be > {low:g} for prior={prior!r} (the moment matching of b needs it), got {a!r}")


def prior_norm(F: torch.Tensor, prior: str) -> torch.Tensor:
    """``f`` of every column of ``F``, fp32 (summed in float64): what the apply kernel maintains from then on."""
    F64 = F.detach().double()
    return (F64.sum(0) if prior == 'l1' else 0.5 * (F64 * F64).sum(0)).float()


class ArdMU:
    """Engine of ``NMF.fit_ard``: a ``DenseMU`` (built as ``NMF._make_engine`` builds one for an unsharded dense fit, without
    the Gram path: the half-steps need both slabs) whose apply stage is ``ard_apply`` and whose exponent is ``ard_exponent``.

    ``lam`` (fp32 ``[R]``) starts from the initial factors.  A factor that is not updated keeps its norm in ``lambda``."""

    def __init__(self, V, W, H, beta, prior, phi, a, b, precision, backend=None, update_W=True, update_H=True):
        check_prior(prior, a)
        if not float(phi) > 0:
            raise ValueError(f'phi (the dispersion) must be > 0, got {phi!r}')
        if not float(b) > 0:
            raise ValueError(f'b must be > 0, got {b!r}')
        self.prior, self.phi, self.a, self.b = prior, float(phi), float(a), float(b)
        self.update_W, self.update_H = update_W, update_H
        eng = DenseMU(V, W, H, beta, 0.0, 0.0, precision=precision, backend=backend, update_W=update_W, update_H=update_H,
                      allow_f16=True, allow_gram=False)
        self.eng, self.be = eng, eng.be
        self.beta, self.rank, self.r_pad = eng.beta, eng.rank, eng.r_pad
        self.precision_name = eng.precision_name
        self.exponent = ard_exponent(self.beta, prior)
        for st in (eng.step_w, eng.step_h):
            if st is not None:
                st.struct.gamma = self.exponent
        N, Cc = H.shape[0], W.shape[0]
        self.c = ard_c(N, Cc, self.a, prior)
        self.bound = self.b / self.c                      # B: the floor of lambda
        dev = W.device
        zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        self.norm_w, self.norm_h = zeros(self.r_pad), zeros(self.r_pad)
        self.norm_w[:self.rank] = prior_norm(W, prior)
        self.norm_h[:self.rank] = prior_norm(H, prior)
        l2 = prior == 'l2'
        self.part_w = zeros(eng.fW.colsum_part.numel()) if l2 and update_W else None
        self.part_h = zeros(eng.fH.colsum_part.numel()) if l2 and update_H else None
        self._lam, self.pen, self.delta = torch.ones(self.r_pad, dtype=torch.float32, device=dev), zeros(self.r_pad), zeros(1)
        self.relevance_step()                             # lambda of the initial factors (its delta means nothing)

    # -- the iteration
    def _half_step(self, st, other, norm_part, norm, tag):
        self.eng._partial(st, tag)
        self.be.ard_apply(st, other.colsum if self.eng.kl else None, self.pen, self.prior, norm_part, norm)

    def w_step(self):
        self._half_step(self.eng.step_w, self.eng.fH, self.part_w, self.norm_w, 'w')

    def h_step(self):
        self._half_step(self.eng.step_h, self.eng.fW, self.part_h, self.norm_h, 'h')

    def relevance_step(self):
        self.be.ard_relevance(self.norm_w, self.norm_h, self.rank, self.r_pad, self.b, self.c, self.phi, self._lam, self.pen,
                              self.delta)

    # -- what the caller reads
    @property
    def lam(self) -> torch.Tensor:
        return self._lam[:self.rank]

    def relative_relevance(self) -> torch.Tensor:
        """``(lambda_k - B) / B``: about 0 for a pruned component."""
        return (self.lam - self.bound) / self.bound

    def divergence(self) -> float:
        return self.eng.divergence()

    def objective(self) -> float:
        """``Obj`` above: the engine's divergence / phi plus the R-length terms in float64 from the device norms and lambda.
        One host sync."""
        lam = self.lam.double()
        nrm = self.norm_w[:self.rank].double() + self.norm_h[:self.rank].double() + self.b
        tail = float((nrm / lam + self.c * lam.log()).sum())
        return self.eng.divergence() / self.phi + tail

    def target_flags(self):
        return self.eng.target_flags()

    def left_f16_range(self) -> bool:
        return self.eng.left_f16_range()
