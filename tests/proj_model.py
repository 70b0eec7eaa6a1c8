"""The model of pgmg_divergence_grid, pgmg_gradient_add_grid and pgmg_project (include/pgmg.h
"Projection"), in numpy over the CPU oracle.  Not a test module.

divergence(u, v, h, order, scale): dx + dy on all N x N points, dx = grad_model's difference of u
    along x, dy = its difference of v along y, each rounded after its factor w, then one add.
gradient_add(phi, h, u, v, order, scale): (u + gx, v + gy), (gx, gy) = grad_model.gradient(phi);
    either of u, v may be None (and comes back None).
project(N, u, v, phi0, order, nu, omega, eps, **rule): f = divergence(u, v, h, order, -1); the
    problem (f, phi0's frame) solved as fmg_bc_model.fmg_bc(nu, omega) followed by
    damp_model.solve_damped(omega) (order 2) or as extrap_model.solve_extrap (order 4); then
    gradient_add(phi, h, u, v, order, -1).  Nothing of what it is given is changed.
table_fields(p, q, N): the fields of the issue's table.
"""
from types import SimpleNamespace

import numpy as np

import damp_model
import extrap_model
import fmg_bc_model
import grad_model
import oracle


def divergence(u, v, h, order=4, scale=1.0):
    with np.errstate(all="ignore"):   # (the special-value fixtures: Inf - Inf)
        return grad_model.gradient(u, h, order, scale)[0] + grad_model.gradient(v, h, order, scale)[1]


def norm(d):
    """sqrt of the sum over all points of d^2, in double."""
    return grad_model.norm(d, None)


def gradient_add(phi, h, u=None, v=None, order=4, scale=1.0):
    gx, gy = grad_model.gradient(phi, h, order, scale)
    with np.errstate(all="ignore"):
        return (None if u is None else np.asarray(u, dtype=np.float64) + gx,
                None if v is None else np.asarray(v, dtype=np.float64) + gy)


def project(N, u, v, phi0, order=4, nu=2, omega=0.5, eps=1e-7, h0=None, a=1.0, alpha=3,
            n_coarse=5, coarse_iter=10, v1=1, v2=1, **rule):
    """pgmg_project on the field (u, v) and a context whose phi is phi0 (its frame is the
    Dirichlet data), with the mesh width h0 (None: a / (N - 1)) and the oracle's fields.  Returns a
    namespace: phi, u, v, f, div_before, div_after, fine and coarse (damp_model.solve_damped's
    namespaces, sweeps and exits including the FMG's; coarse is None at order 2)."""
    assert order in (2, 4), order
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    phi0 = np.ascontiguousarray(phi0, dtype=np.float64)
    h = a / (N - 1) if h0 is None else h0
    okw = dict(a=a, alpha=alpha, n_coarse=n_coarse, coarse_iter=coarse_iter, v1=v1, v2=v2)
    f = divergence(u, v, h, order, -1.0)
    if order == 4:
        r = extrap_model.solve_extrap(N, f, phi0, nu, omega, eps=eps, h0=h0, **okw, **rule)
        phi, fine, coarse = r.phi, r.fine, r.coarse
    else:
        o = oracle.Oracle(eps=eps, **okw)
        start = fmg_bc_model.fmg_bc(o, phi0, f, nu, omega, h0=h0)
        fine = damp_model.solve_damped(N, f=f, phi0=start, omega=omega, eps=eps, h0=h0, **okw, **rule)
        fine.sweeps += o.sweeps            # the context's statistics continue from the FMG's
        fine.exits = o.cut_exits + fine.oracle.cut_exits
        phi, coarse = fine.phi, None
    un, vn = gradient_add(phi, h, u, v, order, -1.0)
    return SimpleNamespace(phi=phi, u=un, v=vn, f=f, div_before=norm(f),
                           div_after=norm(divergence(un, vn, h, order, -1.0)), fine=fine,
                           coarse=coarse)


def table_fields(p, q, N):
    """(u*, v*, w_x, w_y, phi0) on the unit square, element (j, i) at x = i h, y = j h: the field
    w + grad psi, psi = sin(p pi x) sin(q pi y), its divergence-free part w = (s_y, -s_x) of the
    stream function s = sin(1.3 pi x + 0.2) cos(0.7 pi y), and a phi of zeros that carries psi's
    frame"""
    t = np.arange(N) / (N - 1)
    x, y = t[None, :], t[:, None]
    pi = np.pi
    psi = np.sin(p * pi * x) * np.sin(q * pi * y)
    px = p * pi * np.cos(p * pi * x) * np.sin(q * pi * y)
    py = q * pi * np.sin(p * pi * x) * np.cos(q * pi * y)
    wx = -0.7 * pi * np.sin(1.3 * pi * x + 0.2) * np.sin(0.7 * pi * y)
    wy = -1.3 * pi * np.cos(1.3 * pi * x + 0.2) * np.cos(0.7 * pi * y)
    return wx + px, wy + py, wx, wy, fmg_bc_model.set_frame(np.zeros((N, N)), psi)
