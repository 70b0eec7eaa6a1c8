"""The model of pgmg_vorticity_grid, pgmg_wall_vorticity_grid and pgmg_vorticity_step
(include/pgmg.h "Vorticity transport"), in numpy over the CPU oracle.  Not a test module.

step(P, W, h, dt, nu): (out, vmax).  out is W + dt (nu lap - adv) on the interior, every operation
    rounded once in the header's order, and W's words on the frame; vmax is the maximum of
    |px| + |py| over the interior with NaN terms skipped (np.fmax), 0.0 when every term is NaN.
wall(P, W, h, walls, free): a copy of W with its frame set by Thom's formula (walls = ub, ut, vl,
    vr) or to +0.0 (free); the corners +0.0 either way.
vorticity_step(N, psi, w, dt, nu, walls, free, nsteps, omega, **rule): per step wall(), step(),
    then damp_model.solve_damped(N, f=W, phi0=P, omega, ...); after the last step one more wall().
    Returns a namespace: phi, f, last (the last solve's namespace), cycles and sweeps (summed),
    cfl, diffusion.  Nothing of what it is given is changed.
"""
from types import SimpleNamespace

import numpy as np

import damp_model


def step(P, W, h, dt, nu):
    P = np.asarray(P, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    h, dt, nu = np.float64(h), np.float64(dt), np.float64(nu)
    wgt = np.float64(0.5) / h
    ih = np.float64(1.0) / (h * h)
    c = (slice(1, -1), slice(1, -1))
    l, r = (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))
    d, u = (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
    with np.errstate(all="ignore"):   # (the special-value fixtures)
        px = (P[r] - P[l]) * wgt
        py = (P[u] - P[d]) * wgt
        wx = (W[r] - W[l]) * wgt
        wy = (W[u] - W[d]) * wgt
        adv = py * wx - px * wy
        lap = (W[l] + W[r] + W[d] + W[u] - np.float64(4.0) * W[c]) * ih
        out = W.copy()
        out[c] = W[c] + dt * (nu * lap - adv)
        vmax = float(np.fmax.reduce((np.abs(px) + np.abs(py)).ravel(), initial=0.0))
    return out, vmax


def wall(P, W, h, walls=(0.0, 0.0, 0.0, 0.0), free=False):
    P = np.asarray(P, dtype=np.float64)
    out = np.array(W, dtype=np.float64, order="C")
    h = np.float64(h)
    if free:
        out[0, :] = out[-1, :] = 0.0
        out[:, 0] = out[:, -1] = 0.0
        return out
    ub, ut, vl, vr = (np.float64(x) for x in walls)
    c = np.float64(2.0) * (np.float64(1.0) / (h * h))
    d = np.float64(2.0) / h
    with np.errstate(all="ignore"):
        out[0, 1:-1] = (P[0, 1:-1] - P[1, 1:-1]) * c + ub * d
        out[-1, 1:-1] = (P[-1, 1:-1] - P[-2, 1:-1]) * c - ut * d
        out[1:-1, 0] = (P[1:-1, 0] - P[1:-1, 1]) * c - vl * d
        out[1:-1, -1] = (P[1:-1, -1] - P[1:-1, -2]) * c + vr * d
    out[0, 0] = out[0, -1] = out[-1, 0] = out[-1, -1] = 0.0
    return out


def vorticity_step(N, psi, w, dt, nu, walls=(0.0, 0.0, 0.0, 0.0), free=False, nsteps=1, omega=0.5,
                   eps=-1.0, h0=None, a=1.0, solve=None, **rule):
    """pgmg_vorticity_step on a context whose phi is psi and whose f is w.  solve: None is the
    library's damped multigrid solve; otherwise a function (W, P) -> psi that replaces it (the CPU
    tests' direct solver), and last is None."""
    P = np.array(psi, dtype=np.float64, order="C")
    W = np.array(w, dtype=np.float64, order="C")
    h = a / (N - 1) if h0 is None else h0
    cycles = sweeps = 0
    last, vmax = None, 0.0
    for _ in range(nsteps):
        W = wall(P, W, h, walls, free)
        W, vmax = step(P, W, h, dt, nu)
        if solve is not None:
            P = solve(W, P)
            continue
        last = damp_model.solve_damped(N, f=W, phi0=P, omega=omega, eps=eps, h0=h0, a=a, **rule)
        P = last.phi
        cycles += last.cycles
        sweeps += last.sweeps
    W = wall(P, W, h, walls, free)
    return SimpleNamespace(phi=P, f=W, last=last, cycles=cycles, sweeps=sweeps,
                           cfl=dt * vmax / abs(h), diffusion=4.0 * nu * dt / (h * h))
