"""Float64 numpy restatement of the batched Hoyer projection (include/nmfmu.h, nmfmu_hoyer_project), written from that
description -- not from the kernel and not from the reference's text.  One slice at a time, no attempt at speed.

Hoyer 2004, section 3.3: find the closest point to s with sum v = k1, sum v^2 = k2, v >= 0.  Start on the hyperplane
sum v = k1; move away from the uniform point of the coordinates still free until the L2 constraint holds; coordinates that
went negative are fixed at zero and the rest is put back on the hyperplane; repeat.  Two details follow the reference's
behaviour rather than the paper, because the golden vectors come from it: the hyperplane re-shift is added to the coordinates
already fixed at zero as well (they are clamped again afterwards), and the search direction of a fixed coordinate is its
own value instead of 0.
"""
import numpy as np


def project_slice(s, k1, k2):
    """(projected slice, passes) for a 1-D array s; float64 throughout.  ``passes`` counts the L2 steps, capped at n."""
    v = np.asarray(s, dtype=np.float64).reshape(-1).copy()
    n = v.size
    k1, k2 = float(k1), float(k2)
    with np.errstate(all='ignore'):
        v += (k1 - v.sum()) / n                               # 1. onto the hyperplane
        fixed = np.zeros(n, dtype=bool)
        passes = 0
        while True:
            mid = k1 / (n - int(fixed.sum()))                 # 2. the uniform point of the free coordinates
            w = np.where(fixed, v, v - mid)
            a, b, c = w @ w, 2.0 * (w @ v), v @ v - k2
            alpha = (-b + np.sqrt(max(b * b - 4.0 * a * c, 0.0))) / (2.0 * a)      # the larger root
            v = v + alpha * w
            passes += 1
            neg = v < 0                                       # 3. (a NaN compares false: the loop ends)
            if not neg.any() or passes >= n:
                break
            fixed |= neg                                      # 4. fix, clamp, back onto the hyperplane, clamp
            v[neg] = 0.0
            v += (k1 - v.sum()) / (n - int(fixed.sum()))
            v = np.where(v < 0, 0.0, v)
    return v, passes


def project(x, k1, k2, dim=1):
    """Every slice of x along ``dim`` projected with its own (k1[j], k2[j]); returns (float64 array of x's shape, passes[J])."""
    x = np.asarray(x, dtype=np.float64)
    J = x.shape[dim]
    k1 = np.broadcast_to(np.asarray(k1, dtype=np.float64), (J,))
    k2 = np.broadcast_to(np.asarray(k2, dtype=np.float64), (J,))
    out = np.empty_like(x)
    passes = np.zeros(J, dtype=np.int64)
    for j in range(J):
        idx = (slice(None),) * dim + (j,)
        sl = x[idx]
        v, passes[j] = project_slice(sl, k1[j], k2[j])
        out[idx] = v.reshape(sl.shape)
    return out, passes
