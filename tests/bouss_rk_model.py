"""The model of pgmg_boussinesq_stage_grid and pgmg_boussinesq_step_rk (include/pgmg.h "Runge-Kutta
buoyancy-driven flow"), in numpy over tests/bouss_model.py, tests/vort_model.py and
tests/damp_model.py.  Not a test module.

K3, B3, STAGES: vort_rk_model's (the same coefficient pairs serve w and T).
stage(P, W, T, W0, T0, h, dt, nu, kappa, buoy, a, b): (Wout, Tout, vmax).  Wout is a * W0 + b * ew
    and Tout is a * T0 + b * et on the interior, ew and et bouss_model.step(P, W, T, ...)'s values,
    two products and one sum each, every one rounded once; W's and T's words on the frames (the
    frames of W0 and T0 have no part in it); vmax is bouss_model.step's.
boussinesq_step_rk(N, psi, w, T, dt, nu, kappa, buoy, walls, free, adiabatic, order, nsteps, omega,
    **rule): per step and per stage k = 1 .. order: vort_model.wall() and bouss_model.wall_scalar();
    for k = 1, W0 and T0 = the fields after the wall passes and the Euler step, otherwise stage()
    with STAGES[order][k - 2]; then the solve, warm-started from the current psi.  After the last
    step both wall passes once more.  Returns bouss_model.boussinesq_step's namespace: cycles and
    sweeps summed over all stage solves, last the last stage's solve, cfl from the last stage's
    vmax.  solve= as in bouss_model.boussinesq_step.  Nothing of what it is given is changed.
"""
from types import SimpleNamespace

import numpy as np

import bouss_model
import damp_model
import vort_model
from vort_rk_model import B3, K3, STAGES  # noqa: F401  (re-exported)


def stage(P, W, T, W0, T0, h, dt, nu, kappa, buoy, a, b):
    W = np.asarray(W, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    W0 = np.asarray(W0, dtype=np.float64)
    T0 = np.asarray(T0, dtype=np.float64)
    a, b = np.float64(a), np.float64(b)
    ew, et, vmax = bouss_model.step(P, W, T, h, dt, nu, kappa, buoy)
    c = (slice(1, -1), slice(1, -1))
    Wout, Tout = W.copy(), T.copy()
    with np.errstate(all="ignore"):   # (the special-value fixtures)
        Wout[c] = a * W0[c] + b * ew[c]
        Tout[c] = a * T0[c] + b * et[c]
    return Wout, Tout, vmax


def boussinesq_step_rk(N, psi, w, T, dt, nu, kappa, buoy=(0.0, 1.0), walls=(0.0, 0.0, 0.0, 0.0),
                       free=False, adiabatic=bouss_model.BOTTOM | bouss_model.TOP, order=1, nsteps=1,
                       omega=0.5, eps=-1.0, h0=None, a=1.0, solve=None, **rule):
    """pgmg_boussinesq_step_rk on a context whose phi is psi and whose f is w, with the caller's T."""
    P = np.array(psi, dtype=np.float64, order="C")
    W = np.array(w, dtype=np.float64, order="C")
    T = np.array(T, dtype=np.float64, order="C")
    h = a / (N - 1) if h0 is None else h0
    cycles = sweeps = 0
    last, vmax = None, 0.0
    for _ in range(nsteps):
        W0 = T0 = None
        for k in range(order):
            W = vort_model.wall(P, W, h, walls, free)
            T = bouss_model.wall_scalar(T, adiabatic)
            if k == 0:
                W0, T0 = W, T
                W, T, vmax = bouss_model.step(P, W, T, h, dt, nu, kappa, buoy)
            else:
                W, T, vmax = stage(P, W, T, W0, T0, h, dt, nu, kappa, buoy, *STAGES[order][k - 1])
            if solve is not None:
                P = solve(W, P)
                continue
            last = damp_model.solve_damped(N, f=W, phi0=P, omega=omega, eps=eps, h0=h0, a=a, **rule)
            P = last.phi
            cycles += last.cycles
            sweeps += last.sweeps
    W = vort_model.wall(P, W, h, walls, free)
    T = bouss_model.wall_scalar(T, adiabatic)
    return SimpleNamespace(phi=P, f=W, T=T, last=last, cycles=cycles, sweeps=sweeps,
                           cfl=dt * vmax / abs(h), diffusion=4.0 * nu * dt / (h * h),
                           diffusion_t=4.0 * kappa * dt / (h * h))
