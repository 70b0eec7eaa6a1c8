"""The model of pgmg_fmg_bc (include/pgmg.h "Full multigrid with Dirichlet data"), in numpy over
the CPU oracle.  Not a test module.

fmg_bc(o, phi0, f, nu, omega) is fmg_model.fmg (omega = 0) or fmg_damped_model.fmg_damped
(omega > 0) with the frame g of phi0 -- rows 0 and N-1, columns 0 and N-1 -- carried on every level:

1. f_0 = f; f_{l+1} = restrict_full_weighting(f_l) down to the first N_L <= n_coarse;
   g_0 = g; g_{l+1} = g_l[::2, ::2] (injection: only its frame points are used).
2. u_L = 0 on the interior, g_L on the frame, then nu x v_cycle(u_L, f_L, N_L, h_L).
3. for l = L-1 .. 0: u_l = cubic(u_{l+1}), frame included; the frame of u_l <- g_l; then
   nu x { v_cycle(u_l, f_l, N_l, h_l); if omega > 0: u_l <- damp(u_l, f_l, h_l, omega) }.

The interior of phi0 is never read.  restrict and cubic are fmg_model's, v_cycle the oracle's,
damp damp_model's (the level's h, the oracle's element type).
"""
import numpy as np

import damp_model
import fmg_model


def set_frame(u, g):
    """Rows 0 and -1 and columns 0 and -1 of u <- those of g (same shape), in place."""
    u[0, :] = g[0, :]
    u[-1, :] = g[-1, :]
    u[:, 0] = g[:, 0]
    u[:, -1] = g[:, -1]
    return u


def fmg_bc(o, phi0, f, nu=2, omega=0.0, h0=None):
    """The FMG solution of (f, h0) with the Dirichlet frame of phi0, oracle `o` (its eps,
    n_coarse, sweep counters and element type).  phi0, f: (N, N), left untouched.  Returns u_0
    (dtype o.dt), whose frame is phi0's converted to o.dt."""
    f = np.ascontiguousarray(f, dtype=o.dt)
    g = np.ascontiguousarray(phi0, dtype=o.dt)
    N = f.shape[0]
    assert g.shape == f.shape == (N, N), (g.shape, f.shape)
    h = o.c.a / (N - 1) if h0 is None else h0
    dtype = "f32" if o.dt is np.float32 or o.dt == np.float32 else "f64"
    fs, gs, hs = [f], [g], [h]
    while fs[-1].shape[0] > o.c.n_coarse:
        fs.append(fmg_model.restrict(fs[-1], o))
        gs.append(np.ascontiguousarray(gs[-1][::2, ::2]))
        hs.append(2 * hs[-1])
    assert fs[-1].shape[0] >= 5, "the coarsest level needs 5 points per side"
    u = set_frame(np.zeros_like(fs[-1]), gs[-1])
    for _ in range(nu):
        o.v_cycle(u, fs[-1], hs[-1])
    for l in range(len(fs) - 2, -1, -1):
        u = set_frame(fmg_model.cubic(u), gs[l])
        for _ in range(nu):
            o.v_cycle(u, fs[l], hs[l])
            if omega > 0.0:
                u = damp_model.damp(u, fs[l], hs[l], omega, dtype)[0]
    return u
