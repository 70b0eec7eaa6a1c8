"""The model of pgmg_vorticity_stage_grid and pgmg_vorticity_step_rk (include/pgmg.h "Runge-Kutta
vorticity transport"), in numpy over tests/vort_model.py and tests/damp_model.py.  Not a test
module.

K3, B3: the doubles nearest 1/3 and 2/3.  STAGES[order]: the coefficient pairs (a, b) of the
    stages after the first (stage 1 of every order is the plain Euler step).
stage(P, W, W0, h, dt, nu, a, b): (out, vmax).  out is a * W0 + b * e on the interior, e =
    vort_model.step(P, W, ...)'s value, two products and one sum, each rounded once; W's words on
    the frame (W0's frame has no part in it); vmax is vort_model.step's.
vorticity_step_rk(N, psi, w, dt, nu, walls, free, order, nsteps, omega, **rule): per step and per
    stage k = 1 .. order: vort_model.wall(); for k = 1, W0 = the vorticity after the wall pass and
    the Euler step, otherwise stage() with STAGES[order][k - 2]; then the solve, warm-started from
    the current psi.  After the last step one more wall().  Returns vort_model.vorticity_step's
    namespace: cycles and sweeps summed over all stage solves, last the last stage's solve, cfl
    from the last stage's vmax.  solve= as in vort_model.vorticity_step.  Nothing of what it is
    given is changed.
"""
from types import SimpleNamespace

import numpy as np

import damp_model
import vort_model

K3 = float.fromhex("0x1.5555555555555p-2")
B3 = float.fromhex("0x1.5555555555555p-1")
STAGES = {1: (), 2: ((0.5, 0.5),), 3: ((0.75, 0.25), (K3, B3))}


def stage(P, W, W0, h, dt, nu, a, b):
    W = np.asarray(W, dtype=np.float64)
    W0 = np.asarray(W0, dtype=np.float64)
    a, b = np.float64(a), np.float64(b)
    e, vmax = vort_model.step(P, W, h, dt, nu)
    c = (slice(1, -1), slice(1, -1))
    out = W.copy()
    with np.errstate(all="ignore"):   # (the special-value fixtures)
        out[c] = a * W0[c] + b * e[c]
    return out, vmax


def vorticity_step_rk(N, psi, w, dt, nu, walls=(0.0, 0.0, 0.0, 0.0), free=False, order=1, nsteps=1,
                      omega=0.5, eps=-1.0, h0=None, a=1.0, solve=None, **rule):
    """pgmg_vorticity_step_rk on a context whose phi is psi and whose f is w."""
    P = np.array(psi, dtype=np.float64, order="C")
    W = np.array(w, dtype=np.float64, order="C")
    h = a / (N - 1) if h0 is None else h0
    cycles = sweeps = 0
    last, vmax = None, 0.0
    for _ in range(nsteps):
        W0 = None
        for k in range(order):
            W = vort_model.wall(P, W, h, walls, free)
            if k == 0:
                W0 = W
                W, vmax = vort_model.step(P, W, h, dt, nu)
            else:
                W, vmax = stage(P, W, W0, h, dt, nu, *STAGES[order][k - 1])
            if solve is not None:
                P = solve(W, P)
                continue
            last = damp_model.solve_damped(N, f=W, phi0=P, omega=omega, eps=eps, h0=h0, a=a, **rule)
            P = last.phi
            cycles += last.cycles
            sweeps += last.sweeps
    W = vort_model.wall(P, W, h, walls, free)
    return SimpleNamespace(phi=P, f=W, last=last, cycles=cycles, sweeps=sweeps,
                           cfl=dt * vmax / abs(h), diffusion=4.0 * nu * dt / (h * h))
