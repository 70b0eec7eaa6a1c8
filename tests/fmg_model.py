"""The model of pgmg_fmg (include/pgmg.h "Full multigrid"), in numpy over the CPU oracle.

fmg(N, f, nu) is what every FMG test compares against:

1. f_0 = f; f_{l+1} = restrict_full_weighting(f_l) (orc_restrict: interior points, boundary 0)
   down to the first N_L <= n_coarse; N_{l+1} = (N_l - 1) / 2 + 1, h_l = h_0 * 2^l.
2. u_L = 0, then nu x v_cycle(u_L, f_L, N_L, h_L).
3. for l = L-1 .. 0: u_l = cubic(u_{l+1}), then nu x v_cycle(u_l, f_l, N_l, h_l).

cubic() is the tensor-product cubic interpolation from Nc to 2 Nc - 1 points per side: first
along x on every coarse row, then along y on the x-interpolated rows; every operation in the
array's dtype, one rounding per operation, left to right (no fused multiply-add).
"""
import ctypes as C

import numpy as np

import oracle


def _interp_rows(c):
    """c: (..., Nc) -> (..., 2 Nc - 1) along the last axis."""
    dt = c.dtype.type
    Nc = c.shape[-1]
    assert Nc >= 5, Nc
    Nf = 2 * Nc - 1
    out = np.empty(c.shape[:-1] + (Nf,), dtype=c.dtype)
    out[..., 0::2] = c
    k9, k5, k15, s = dt(9.0), dt(5.0), dt(15.0), dt(0.0625)
    # interior odd positions 3 .. Nf-4: a, b, c, d at (k-3)/2, (k-1)/2, (k+1)/2, (k+3)/2
    a, b, cc, d = c[..., 0:Nc - 3], c[..., 1:Nc - 2], c[..., 2:Nc - 1], c[..., 3:Nc]
    out[..., 3:Nf - 3:2] = (k9 * (b + cc) - (a + d)) * s
    out[..., 1] = (k5 * c[..., 0] + k15 * c[..., 1] - k5 * c[..., 2] + c[..., 3]) * s
    out[..., Nf - 2] = (k5 * c[..., Nc - 1] + k15 * c[..., Nc - 2] - k5 * c[..., Nc - 3]
                        + c[..., Nc - 4]) * s
    return out


def cubic(coarse):
    """Tensor-product cubic interpolation of an (Nc, Nc) grid to (2 Nc - 1, 2 Nc - 1)."""
    coarse = np.ascontiguousarray(coarse)
    x = _interp_rows(coarse)                       # along x on every coarse row
    return np.ascontiguousarray(_interp_rows(x.T).T)   # along y on the x-interpolated rows


def bilinear(coarse, o):
    """The reference's prolongation into a zeroed grid (orc_prolong: row / column 1 stay 0)."""
    Nc = coarse.shape[0]
    Nf = 2 * Nc - 1
    fine = np.zeros((Nf, Nf), dtype=coarse.dtype)
    o.L.orc_prolong(fine.ctypes.data_as(C.c_void_p), coarse.ctypes.data_as(C.c_void_p), Nf, Nc)
    return fine


def restrict(fine, o):
    Nf = fine.shape[0]
    Nc = (Nf - 1) // 2 + 1
    c = np.zeros((Nc, Nc), dtype=fine.dtype)
    o.L.orc_restrict(fine.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), Nf, Nc)
    return c


def fmg(o, f, nu=2, h0=None, interp="cubic"):
    """The FMG solution of (f, h0) with oracle `o` (its eps, n_coarse, sweeps counters and
    element type).  f: (N, N) array of o.dt, left untouched.  Returns u_0 (dtype o.dt)."""
    f = np.ascontiguousarray(f, dtype=o.dt)
    N = f.shape[0]
    h = o.c.a / (N - 1) if h0 is None else h0
    fs, hs = [f], [h]
    while fs[-1].shape[0] > o.c.n_coarse:
        fs.append(restrict(fs[-1], o))
        hs.append(2 * hs[-1])
    assert fs[-1].shape[0] >= 5, "the coarsest level needs 5 points per side"
    u = np.zeros_like(fs[-1])
    for _ in range(nu):
        o.v_cycle(u, fs[-1], hs[-1])
    for l in range(len(fs) - 2, -1, -1):
        u = cubic(u) if interp == "cubic" else bilinear(u, o)
        for _ in range(nu):
            o.v_cycle(u, fs[l], hs[l])
    return u


def fmg_analytic(N, nu=2, eps=1e-7, dtype="f64", interp="cubic", **kw):
    """(u_0, oracle) for the analytic problem of size N."""
    o = oracle.Oracle(eps=eps, dtype=dtype, **kw)
    return fmg(o, o.rhs(N), nu, interp=interp), o
