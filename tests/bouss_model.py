"""The model of pgmg_boussinesq_grid, pgmg_wall_scalar_grid and pgmg_boussinesq_step
(include/pgmg.h "Buoyancy-driven flow"), in numpy over vort_model and the CPU oracle.  Not a test
module.

step(P, W, T, h, dt, nu, kappa, buoy): (Wout, Tout, vmax).  Wout is W + dt ((nu lapw - advw) + src)
    and Tout is T + dt (kappa lapt - advt) on the interior, every operation rounded once in the
    header's order, and the words of W and of T on the frames; vmax is vort_model.step's.
wall_scalar(T, mask): a copy of T with the walls whose PGMG_TWALL_* bit is set in mask made
    adiabatic by the one-sided formula; the corners and the other walls keep their words.
boussinesq_step(N, psi, w, T, dt, nu, kappa, buoy, walls, free, adiabatic, nsteps, omega, **rule):
    per step vort_model.wall(), wall_scalar(), step(), then damp_model.solve_damped(N, f=W,
    phi0=P, omega, ...); after the last step both wall passes once more.  Returns a namespace:
    phi, f, T, last (the last solve's namespace), cycles and sweeps (summed), cfl, diffusion,
    diffusion_t.  Nothing of what it is given is changed.
"""
from types import SimpleNamespace

import numpy as np

import damp_model
import vort_model

BOTTOM, TOP, LEFT, RIGHT = 1, 2, 4, 8
K3 = np.array([0x3FD5555555555555], dtype=np.uint64).view(np.float64)[0]   # the double nearest 1/3


def step(P, W, T, h, dt, nu, kappa, buoy):
    P = np.asarray(P, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    h, dt, nu, kappa = np.float64(h), np.float64(dt), np.float64(nu), np.float64(kappa)
    bx, by = np.float64(buoy[0]), np.float64(buoy[1])
    wgt = np.float64(0.5) / h
    ih = np.float64(1.0) / (h * h)
    c = (slice(1, -1), slice(1, -1))
    l, r = (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))
    d, u = (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
    four = np.float64(4.0)
    with np.errstate(all="ignore"):   # (the special-value fixtures)
        px = (P[r] - P[l]) * wgt
        py = (P[u] - P[d]) * wgt
        wx = (W[r] - W[l]) * wgt
        wy = (W[u] - W[d]) * wgt
        tx = (T[r] - T[l]) * wgt
        ty = (T[u] - T[d]) * wgt
        advw = py * wx - px * wy
        advt = py * tx - px * ty
        lapw = (W[l] + W[r] + W[d] + W[u] - four * W[c]) * ih
        lapt = (T[l] + T[r] + T[d] + T[u] - four * T[c]) * ih
        src = by * tx - bx * ty
        Wout, Tout = W.copy(), T.copy()
        Wout[c] = W[c] + dt * ((nu * lapw - advw) + src)
        Tout[c] = T[c] + dt * (kappa * lapt - advt)
        vmax = float(np.fmax.reduce((np.abs(px) + np.abs(py)).ravel(), initial=0.0))
    return Wout, Tout, vmax


def wall_scalar(T, mask):
    out = np.array(T, dtype=np.float64, order="C")
    i = slice(1, -1)
    with np.errstate(all="ignore"):
        # (every value read is an interior value of T: the walls do not depend on each other)
        if mask & BOTTOM:
            out[0, i] = T[1, i] + (T[1, i] - T[2, i]) * K3
        if mask & TOP:
            out[-1, i] = T[-2, i] + (T[-2, i] - T[-3, i]) * K3
        if mask & LEFT:
            out[i, 0] = T[i, 1] + (T[i, 1] - T[i, 2]) * K3
        if mask & RIGHT:
            out[i, -1] = T[i, -2] + (T[i, -2] - T[i, -3]) * K3
    return out


def boussinesq_step(N, psi, w, T, dt, nu, kappa, buoy=(0.0, 1.0), walls=(0.0, 0.0, 0.0, 0.0),
                    free=False, adiabatic=BOTTOM | TOP, nsteps=1, omega=0.5, eps=-1.0, h0=None, a=1.0,
                    solve=None, **rule):
    """pgmg_boussinesq_step on a context whose phi is psi and whose f is w, with the caller's T.
    solve: None is the library's damped multigrid solve; otherwise a function (W, P) -> psi that
    replaces it (the CPU tests' direct solver), and last is None."""
    P = np.array(psi, dtype=np.float64, order="C")
    W = np.array(w, dtype=np.float64, order="C")
    T = np.array(T, dtype=np.float64, order="C")
    h = a / (N - 1) if h0 is None else h0
    cycles = sweeps = 0
    last, vmax = None, 0.0
    for _ in range(nsteps):
        W = vort_model.wall(P, W, h, walls, free)
        T = wall_scalar(T, adiabatic)
        W, T, vmax = step(P, W, T, h, dt, nu, kappa, buoy)
        if solve is not None:
            P = solve(W, P)
            continue
        last = damp_model.solve_damped(N, f=W, phi0=P, omega=omega, eps=eps, h0=h0, a=a, **rule)
        P = last.phi
        cycles += last.cycles
        sweeps += last.sweeps
    W = vort_model.wall(P, W, h, walls, free)
    T = wall_scalar(T, adiabatic)
    return SimpleNamespace(phi=P, f=W, T=T, last=last, cycles=cycles, sweeps=sweeps,
                           cfl=dt * vmax / abs(h), diffusion=4.0 * nu * dt / (h * h),
                           diffusion_t=4.0 * kappa * dt / (h * h))
