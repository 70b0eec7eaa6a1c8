"""The model of pgmg_fmg_damped (include/pgmg.h "Damped full multigrid"), in numpy over the CPU
oracle.  Not a test module.

fmg_damped(o, f, nu, omega) is fmg_model.fmg with a damping pass after every V-cycle of the climb:

1. f_0 = f; f_{l+1} = restrict_full_weighting(f_l) down to the first N_L <= n_coarse.
2. u_L = 0, then nu x v_cycle(u_L, f_L, N_L, h_L)           (the coarsest level is not damped).
3. for l = L-1 .. 0: u_l = cubic(u_{l+1}), then
   nu x { v_cycle(u_l, f_l, N_l, h_l); u_l <- damp(u_l, f_l, h_l, omega) }.

restrict and cubic are fmg_model's, v_cycle the oracle's, damp damp_model's (the level's h, the
oracle's element type).
"""
import numpy as np

import damp_model
import fmg_model
import oracle


def fmg_damped(o, f, nu=2, omega=0.5, h0=None):
    """The damped FMG solution of (f, h0) with oracle `o` (its eps, n_coarse, sweep counters and
    element type).  f: (N, N), left untouched.  Returns u_0 (dtype o.dt)."""
    f = np.ascontiguousarray(f, dtype=o.dt)
    N = f.shape[0]
    h = o.c.a / (N - 1) if h0 is None else h0
    dtype = "f32" if o.dt is np.float32 or o.dt == np.float32 else "f64"
    fs, hs = [f], [h]
    while fs[-1].shape[0] > o.c.n_coarse:
        fs.append(fmg_model.restrict(fs[-1], o))
        hs.append(2 * hs[-1])
    assert fs[-1].shape[0] >= 5, "the coarsest level needs 5 points per side"
    u = np.zeros_like(fs[-1])
    for _ in range(nu):
        o.v_cycle(u, fs[-1], hs[-1])
    for l in range(len(fs) - 2, -1, -1):
        u = fmg_model.cubic(u)
        for _ in range(nu):
            o.v_cycle(u, fs[l], hs[l])
            u, _ = damp_model.damp(u, fs[l], hs[l], omega, dtype)
    return u


def fmg_damped_analytic(N, nu=2, omega=0.5, eps=1e-7, dtype="f64", **kw):
    """(u_0, oracle) for the analytic problem of size N."""
    o = oracle.Oracle(eps=eps, dtype=dtype, **kw)
    return fmg_damped(o, o.rhs(N), nu, omega), o


def rel_residual(u, f, h):
    """||f - A u|| / ||f|| over the interior points, in double."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    r = oracle.residual(u, f, h)[1:-1, 1:-1]
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(f[1:-1, 1:-1] ** 2)))
