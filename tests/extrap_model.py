"""The model of pgmg_extrap_grid and pgmg_solve_extrap (include/pgmg.h "Fourth-order solves by
Richardson extrapolation"), in numpy over the CPU oracle.  Not a test module.

extrapolate(fine, coarse):
    D = (fine[::2, ::2] - coarse) * K3     K3 the double nearest 1/3: two roundings
    E = fmg_model.cubic(D)                 pgmg_fmg's cubic interpolation
    fine[1:-1, 1:-1] + E[1:-1, 1:-1]       one rounding; the frame of fine is kept
solve_extrap(...): on the grid and on the grid of every second point (phi0[::2, ::2], f[::2, ::2],
    2 h) fmg_bc_model.fmg_bc(nu, omega), then damp_model.solve_damped(omega) from it; the two
    results extrapolated.  The fine solve runs at the context's mesh width h0 (None: a / (N - 1)),
    the half-resolution one at 2 h0 (exact), both with the same oracle fields (a, p, q, alpha,
    n_coarse, coarse_iter, v1, v2): pgmg_solve_extrap copies the parent's configuration.
"""
from types import SimpleNamespace

import numpy as np

import damp_model
import fmg_bc_model
import fmg_model
import oracle

K3 = np.array([0x3FD5555555555555], dtype=np.uint64).view(np.float64)[0]


def extrapolate(fine, coarse):
    """The extrapolated fine grid; fine and coarse are left untouched."""
    fine = np.ascontiguousarray(fine, dtype=np.float64)
    coarse = np.ascontiguousarray(coarse, dtype=np.float64)
    Nf, Nc = fine.shape[0], coarse.shape[0]
    assert fine.shape == (Nf, Nf) and coarse.shape == (Nc, Nc) and Nf == 2 * Nc - 1 and Nc >= 5
    with np.errstate(all="ignore"):   # (the special-value fixtures: Inf - Inf, 0 * Inf)
        d = (fine[::2, ::2] - coarse) * K3
        e = fmg_model.cubic(d)
        out = fine.copy()
        out[1:-1, 1:-1] = fine[1:-1, 1:-1] + e[1:-1, 1:-1]
    return out


def _solve(N, f, phi0, nu, omega, eps, h0, okw, rule):
    o = oracle.Oracle(eps=eps, **okw)
    u = fmg_bc_model.fmg_bc(o, phi0, f, nu, omega, h0=h0)
    r = damp_model.solve_damped(N, f=f, phi0=u, omega=omega, eps=eps, h0=h0, **okw, **rule)
    r.sweeps += o.sweeps            # the context's statistics continue from the FMG's
    r.exits = o.cut_exits + r.oracle.cut_exits
    return r


def solve_extrap(N, f, phi0, nu=2, omega=0.5, eps=1e-7, h0=None, a=1.0, p=1.0, q=1.0, alpha=3,
                 n_coarse=5, coarse_iter=10, v1=1, v2=1, **rule):
    """pgmg_solve_extrap on (f, phi0), both (N, N) float64, left untouched, on a context with the
    mesh width h0 (None: a / (N - 1)) and the oracle's fields a .. v2.  Returns a namespace:
    phi (the extrapolated solution), phi2 (the fine second-order solution it was made from),
    fine and coarse (damp_model.solve_damped's namespaces, sweeps and exits including the FMG's)."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    phi0 = np.ascontiguousarray(phi0, dtype=np.float64)
    okw = dict(a=a, p=p, q=q, alpha=alpha, n_coarse=n_coarse, coarse_iter=coarse_iter, v1=v1, v2=v2)
    h = a / (N - 1) if h0 is None else h0
    Nc = (N + 1) // 2
    coarse = _solve(Nc, np.ascontiguousarray(f[::2, ::2]), np.ascontiguousarray(phi0[::2, ::2]),
                    nu, omega, eps, 2 * h, okw, rule)
    fine = _solve(N, f, phi0, nu, omega, eps, h, okw, rule)
    return SimpleNamespace(phi=extrapolate(fine.phi, coarse.phi), phi2=fine.phi, fine=fine,
                           coarse=coarse)
