"""float64 references and error bounds of the PLCA / SIPLCA backward (CPU, plain torch), shared by test_plca_autograd_host.py
(which checks them against the reference's own gradients in tests/golden/g18_plca_autograd.npz) and test_gpu_plca_autograd.py.

With G = d loss / d out and the UNSCALED products rawH = backward_H(G, W), rawW = backward_W(G, H):
    grad_H = Z[r] rawH        grad_W = Z[r] rawW        grad_Z[r] = sum rawW W  ( = sum rawH H )
u = 2^-24.  First-order bounds, valid for any summation order (K = the product's contraction length, P = the number of terms of
the Z dot product; absH / absW are the same products with |G| and the non-negative factors):
    |grad_F - ref| <= (K + 3) u |Z[r]| abs_F              (K + 2) u of an fp32 dot product plus the one rounding of the scale
    |grad_Z - ref| <= (K + P + 3) u sum abs_F |F|         either half: K_h + P_h = K_w + P_w = C prod(T) + B prod(Lh)
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


def raw_products(G, H, W):
    """(rawH, rawW, K_h, K_w) in float64 for 2-D factors (dense) or (B, R, *Lh) / (C, R, *T) factors (shift-invariant)."""
    G, H, W = G.double(), H.double(), W.double()
    if W.dim() == 2:
        return G @ W, G.t() @ H, W.shape[0], H.shape[0]
    nd = H.dim() - 2
    conv = (F.conv1d, F.conv2d, F.conv3d)[nd - 1]
    Hr, Wr = H.clone().requires_grad_(), W.clone().requires_grad_()
    out = conv(Hr, Wr.flip(tuple(range(2, 2 + nd))), padding=tuple(t - 1 for t in W.shape[2:]))
    assert out.shape == G.shape, (out.shape, G.shape)
    rawH, rawW = torch.autograd.grad(out, (Hr, Wr), G)
    return rawH, rawW, W.shape[0] * _prod(W.shape[2:]), H.shape[0] * _prod(H.shape[2:])


def _zview(Z, like):
    return Z.double().view(1, -1, *([1] * (like.dim() - 2)))


def _rank_sum(x):
    return x.sum([d for d in range(x.dim()) if d != 1])


def reference(G, H, W, Z):
    """dict of float64 gradients (gH, gW, gZ) and bounds (bH, bW, bZ) for the upstream gradient G (all CPU tensors)."""
    rawH, rawW, k_h, k_w = raw_products(G, H, W)
    absH, absW, _, _ = raw_products(G.abs(), H.abs(), W.abs())
    zH, zW = _zview(Z, H), _zview(Z, W)
    return dict(gH=rawH * zH, gW=rawW * zW, gZ=_rank_sum(rawW * W.double()),
                gZ_from_H=_rank_sum(rawH * H.double()),
                bH=(k_h + 3) * U * zH.abs() * absH, bW=(k_w + 3) * U * zW.abs() * absW,
                bZ=(k_h + k_w + 3) * U * _rank_sum(absW * W.double().abs()))
