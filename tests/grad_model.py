"""The model of pgmg_gradient and pgmg_gradient_grid (include/pgmg.h "Gradient of the solution"),
in numpy.  Not a test module.

gradient(phi, h, order, scale, dtype): (gx, gy) = scale * grad(phi) on all N x N points, frame
    included, by the central differences of the given order and one-sided differences of the same
    order on the frame (order 4: also next to it).  Every expression is evaluated left to right as
    written in arrays of `dtype`, one rounding per operation; the factor w is formed in double
    (scale * 0.5 / h, or scale / (12.0 * h)) and then converted.  Along one line v[0 .. n-1]:

    order 2:  g[k]   = (v[k+1] - v[k-1]) * w                                   1 <= k <= n-2
              g[0]   = (4 v[1] - 3 v[0] - v[2]) * w
              g[n-1] = (3 v[n-1] - 4 v[n-2] + v[n-3]) * w
    order 4:  g[k]   = (8 (v[k+1] - v[k-1]) - (v[k+2] - v[k-2])) * w           2 <= k <= n-3
              g[0]   = (48 v[1] - 25 v[0] - 36 v[2] + 16 v[3] - 3 v[4]) * w
              g[1]   = (18 v[2] - 10 v[1] - 3 v[0] - 6 v[3] + v[4]) * w
              g[n-1] = (25 v[n-1] - 48 v[n-2] + 36 v[n-3] - 16 v[n-4] + 3 v[n-5]) * w
              g[n-2] = (10 v[n-2] - 18 v[n-3] + 3 v[n-1] + 6 v[n-4] - v[n-5]) * w

    The results are returned as float64 (a float32 result widened, as the library stores it).
norm(gx, gy): sqrt of the sum over all points of gx^2 + gy^2, every term squared and summed in
    double; either component may be None (that component was not computed).
"""
import numpy as np


def weight(h, order, scale, dtype=np.float64):
    """The factor w: the double expression, left to right, then converted to dtype."""
    h, scale = np.float64(h), np.float64(scale)
    with np.errstate(all="ignore"):
        w = scale * np.float64(0.5) / h if order == 2 else scale / (np.float64(12.0) * h)
    return np.dtype(dtype).type(w)


def _along_last(v, w, order):
    """The difference along the last axis of v (an array of w's type)."""
    t = v.dtype.type
    g = np.empty_like(v)
    if order == 2:
        g[..., 1:-1] = (v[..., 2:] - v[..., :-2]) * w
        g[..., 0] = (t(4) * v[..., 1] - t(3) * v[..., 0] - v[..., 2]) * w
        g[..., -1] = (t(3) * v[..., -1] - t(4) * v[..., -2] + v[..., -3]) * w
        return g
    g[..., 2:-2] = (t(8) * (v[..., 3:-1] - v[..., 1:-3]) - (v[..., 4:] - v[..., :-4])) * w
    g[..., 0] = (t(48) * v[..., 1] - t(25) * v[..., 0] - t(36) * v[..., 2] + t(16) * v[..., 3]
                 - t(3) * v[..., 4]) * w
    g[..., 1] = (t(18) * v[..., 2] - t(10) * v[..., 1] - t(3) * v[..., 0] - t(6) * v[..., 3]
                 + v[..., 4]) * w
    g[..., -1] = (t(25) * v[..., -1] - t(48) * v[..., -2] + t(36) * v[..., -3] - t(16) * v[..., -4]
                  + t(3) * v[..., -5]) * w
    g[..., -2] = (t(10) * v[..., -2] - t(18) * v[..., -3] + t(3) * v[..., -1] + t(6) * v[..., -4]
                  - v[..., -5]) * w
    return g


def gradient(phi, h, order=4, scale=1.0, dtype=np.float64):
    """(gx, gy) as float64 arrays; phi (N x N, N >= 5) is converted to dtype first and left
    untouched."""
    assert order in (2, 4), order
    v = np.ascontiguousarray(phi).astype(dtype)
    N = v.shape[0]
    assert v.shape == (N, N) and N >= 5, v.shape
    w = weight(h, order, scale, dtype)
    with np.errstate(all="ignore"):   # (the special-value fixtures: Inf - Inf, 0 * Inf)
        gx = _along_last(v, w, order)
        gy = np.ascontiguousarray(_along_last(np.ascontiguousarray(v.T), w, order).T)
    return gx.astype(np.float64), gy.astype(np.float64)


def norm(gx, gy):
    s = 0.0
    with np.errstate(all="ignore"):
        for g in (gx, gy):
            if g is not None:
                g = np.asarray(g, dtype=np.float64)
                s += float(np.sum(g * g))
    return float(np.sqrt(s))
