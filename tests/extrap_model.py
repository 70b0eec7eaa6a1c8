"""The model of pgmg_extrap_grid and pgmg_solve_extrap (include/pgmg.h "Fourth-order solves by
Richardson extrapolation"), in numpy over the CPU oracle.  Not a test module.

extrapolate(fine, coarse):
    D = (fine[::2, ::2] - coarse) * K3     K3 the double nearest 1/3: two roundings
    E = fmg_model.cubic(D)                 pgmg_fmg's cubic interpolation
    fine[1:-1, 1:-1] + E[1:-1, 1:-1]       one rounding; the frame of fine is kept
solve_extrap(...): on the grid and on the grid of every second point (phi0[::2, ::2], f[::2, ::2],
    2 h) fmg_bc_model.fmg_bc(nu, omega), then damp_model.solve_damped(omega) from it; the two
    results extrapolated.  a = 1 (h = 1 / (N - 1), as damp_model.solve_damped takes it).
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


def _solve(N, f, phi0, nu, omega, eps, rule):
    o = oracle.Oracle(eps=eps)
    u = fmg_bc_model.fmg_bc(o, phi0, f, nu, omega)
    r = damp_model.solve_damped(N, f=f, phi0=u, omega=omega, eps=eps, **rule)
    r.sweeps += o.sweeps            # the context's statistics continue from the FMG's
    r.exits = o.cut_exits + r.oracle.cut_exits
    return r


def solve_extrap(N, f, phi0, nu=2, omega=0.5, eps=1e-7, **rule):
    """pgmg_solve_extrap on (f, phi0), both (N, N) float64, left untouched.  Returns a namespace:
    phi (the extrapolated solution), phi2 (the fine second-order solution it was made from),
    fine and coarse (damp_model.solve_damped's namespaces, sweeps including the FMG's)."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    phi0 = np.ascontiguousarray(phi0, dtype=np.float64)
    Nc = (N + 1) // 2
    coarse = _solve(Nc, np.ascontiguousarray(f[::2, ::2]), np.ascontiguousarray(phi0[::2, ::2]),
                    nu, omega, eps, rule)
    fine = _solve(N, f, phi0, nu, omega, eps, rule)
    return SimpleNamespace(phi=extrapolate(fine.phi, coarse.phi), phi2=fine.phi, fine=fine,
                           coarse=coarse)
