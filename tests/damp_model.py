"""The model of pgmg_damp and pgmg_solve_damped (include/pgmg.h "Damping pass and damped
solve"), in numpy over the CPU oracle.  Not a test module.

damp():   phi[1:-1, 1:-1] + w * r[1:-1, 1:-1] with r the oracle's residual of the matching element
          type, w = dtype(omega * 0.25 * (h * h)) (the double product left to right, then
          converted), the product and the sum each rounded once in dtype; the boundary is kept.
          The norm returned is the oracle's sequential residual norm of phi BEFORE the update.
solve_damped():  pgmg_solve's loop (tests/solve_rule.simulate's rule) with every check made by
          damp(): at check i the norm of the iterate as the cycles left it, then the correction,
          then the rule, then the next chunk of oracle cycles.  The context's mesh width h0 and
          the oracle's fields (a, p, q, alpha, n_coarse, coarse_iter, v1, v2) are arguments; the
          defaults are pgmg_config's.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import oracle
import solve_rule


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _dt(dtype):
    return np.float32 if dtype in ("f32", np.float32) else np.float64


def damp(phi, f, h, omega, dtype="f64"):
    """(damped phi, residual norm of phi before the update); phi and f are left untouched."""
    dt = _dt(dtype)
    x = np.ascontiguousarray(phi, dtype=dt)
    ff = np.ascontiguousarray(f, dtype=dt)
    N = x.shape[0]
    if dt is np.float64:
        r = oracle.residual(x, ff, h)
    else:
        r = np.zeros_like(x)
        oracle.lib("f32").orc_residual(_p(r), _p(x), _p(ff), N, N, h)
    norm = oracle.lib(dtype).orc_residual_norm(_p(x), _p(ff), N, h)
    w = dt(omega * 0.25 * (h * h))
    out = x.copy()
    out[1:-1, 1:-1] = x[1:-1, 1:-1] + w * r[1:-1, 1:-1]
    assert out.dtype == dt
    return out, norm


def solve_damped(N, f=None, phi0=None, kind="V", omega=0.5, dtype="f64", eps=1e-7, error=False,
                 h0=None, a=1.0, p=1.0, q=1.0, alpha=3, n_coarse=5, coarse_iter=10, v1=1, v2=1,
                 **rule):
    """The damped solve of (f, phi0) (None: the analytic f, zero) on a context with the mesh width
    h0 (None: a / (N - 1)) and the oracle's fields a .. v2.  kind: "V", "W" (with alpha = 1 the
    oracle's v_cycle, as the library runs it) or "F" (the F-cycle's own chain of mesh widths).
    Returns a namespace with cycles, reason, checks, history [(cycles, norm, rel_error or nan)],
    phi (the final, damped iterate), sweeps, exits (o.cut_exits: what pgmg_stats counts) and
    margin (the smallest relative margin of any comparison the rule made)."""
    o = oracle.Oracle(eps=eps, dtype=dtype, a=a, p=p, q=q, alpha=alpha, n_coarse=n_coarse,
                      coarse_iter=coarse_iter, v1=v1, v2=v2)
    h = a / (N - 1) if h0 is None else h0
    ff = o.rhs(N, h) if f is None else np.ascontiguousarray(f, dtype=o.dt)
    st = SimpleNamespace(phi=np.zeros((N, N), dtype=o.dt) if phi0 is None
                         else np.array(phi0, dtype=o.dt, order="C"), k=0, rel=[])
    if kind not in ("V", "W", "F"):
        raise ValueError(kind)
    step = o.v_cycle if kind == "V" or (kind == "W" and alpha == 1) else o.w_cycle

    def res_at(i, k):
        while st.k < k:
            if kind == "F":
                o.f_cycle_outer(st.phi)
            else:
                step(st.phi, ff, h)
            st.k += 1
        st.rel.append(o.rel_error(st.phi, h) if error else float("nan"))
        st.phi, r = damp(st.phi, ff, h, omega, dtype)
        return r

    cycles, reason, recs, margin = solve_rule.simulate(res_at, **rule)
    return SimpleNamespace(cycles=cycles, reason=reason, checks=len(recs),
                           history=[(k, r, e) for (k, r), e in zip(recs, st.rel)],
                           phi=st.phi, sweeps=o.sweeps, exits=o.cut_exits, margin=margin, f=ff,
                           oracle=o)
