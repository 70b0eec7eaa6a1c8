"""The model of pgmg_defect_grid, pgmg_correct_grid and pgmg_solve_mixed (include/pgmg.h
"Mixed-precision refinement"), in numpy over the CPU oracle.  Not a test module.

defect(x, f, h, s):   r = oracle.residual(x, f, h) (the monitor's fp64 expression);
                      g[1:-1, 1:-1] = float32(r * s): one double product, then numpy's conversion
                      (IEEE round-to-nearest-even, overflow to Inf, gradual underflow); the frame
                      of g is +0.  The norm returned is the oracle's sequential residual norm.
correct(x, e, t):     x[1:-1, 1:-1] + float64(e) * t, two roundings; the frame of x is kept.
scale(rho, N):        2^(-ilogb(rho / (N - 2))), the exponent clamped to [-1022, 1022]; 1.0 when
                      the quotient is 0 or not finite.  Also how far the quotient lies from a power
                      of two, relative: a norm that close to one could pick another s on the
                      device, whose norm differs in summation order.
solve_mixed(...):     pgmg_solve's rule (solve_rule.simulate) over the steps: at check i the defect
                      of the current phi scaled by s_i (from the previous check's norm; check 0:
                      from phi's own), then the rule, then e = fmg_damped_model.fmg_damped of g_i
                      with an fp32 Oracle(eps=-1) and the correction by 1 / s_i.
"""
import math
from types import SimpleNamespace

import numpy as np

import fmg_damped_model
import oracle
import solve_rule


def scale(rho, N):
    """(s, relative distance of rho / (N - 2) from a power of two; inf where s is 1.0 by rule)"""
    q = rho / (N - 2)
    if q == 0.0 or not math.isfinite(q):
        return 1.0, math.inf
    m, e = math.frexp(q)          # q = m 2^e, 0.5 <= m < 1: ilogb(q) = e - 1
    e = min(max(e - 1, -1022), 1022)
    m *= 2.0                      # 1 <= m < 2
    return math.ldexp(1.0, -e), min(m - 1.0, 2.0 - m) / m


def defect(x, f, h, s=1.0):
    """(g float32, residual norm of x); x and f are left untouched."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    N = x.shape[0]
    with np.errstate(all="ignore"):   # (the special-value fixtures; the conversion's overflow)
        r = oracle.residual(x, f, h)
        g = np.zeros((N, N), dtype=np.float32)
        g[1:-1, 1:-1] = (r[1:-1, 1:-1] * np.float64(s)).astype(np.float32)
    return g, solve_rule.oracle_res_norm(oracle, x, f, "f64", h)


def correct(x, e, t=1.0):
    """The corrected x; x and e are left untouched."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert e.dtype == np.float32 and e.shape == x.shape
    out = x.copy()
    with np.errstate(all="ignore"):
        out[1:-1, 1:-1] = x[1:-1, 1:-1] + e[1:-1, 1:-1].astype(np.float64) * np.float64(t)
    return out


def solve_mixed(N, f, phi0, nu=2, omega=0.5, h0=None, a=1.0, p=1.0, q=1.0, alpha=3, n_coarse=5,
                coarse_iter=10, v1=1, v2=1, max_steps=8, rtol=0.0, atol=0.0, stall_ratio=0.0,
                stall_checks=2):
    """pgmg_solve_mixed on (f, phi0), both (N, N) float64, left untouched, on a context with the
    mesh width h0 (None: a / (N - 1)) and the oracle's fields a .. v2.  Returns a namespace: phi,
    steps, reason, checks, history [(steps, norm)], margin (solve_rule.simulate's), inner_sweeps
    (the fp32 oracle's), scales [s_i per check] and pow2_dist (the smallest relative distance of any
    rho_i / (N - 2) from a power of two)."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    h = a / (N - 1) if h0 is None else h0
    o32 = oracle.Oracle(eps=-1.0, dtype="f32", a=a, p=p, q=q, alpha=alpha, n_coarse=n_coarse,
                        coarse_iter=coarse_iter, v1=v1, v2=v2)
    st = SimpleNamespace(phi=np.array(phi0, dtype=np.float64, order="C"), k=0, g=None, s=None,
                         rho=None, scales=[], dist=math.inf)
    st.rho = solve_rule.oracle_res_norm(oracle, st.phi, f, "f64", h)

    def res_at(i, k):
        while st.k < k:
            e = fmg_damped_model.fmg_damped(o32, st.g, nu, omega, h0=h)
            st.phi = correct(st.phi, e, 1.0 / st.s)
            st.k += 1
        st.s, d = scale(st.rho, N)
        st.scales.append(st.s)
        st.dist = min(st.dist, d)
        st.g, r = defect(st.phi, f, h, st.s)
        st.rho = r
        return r

    steps, reason, recs, margin = solve_rule.simulate(res_at, max_cycles=max_steps, check_every=1,
                                                      rtol=rtol, atol=atol, stall_ratio=stall_ratio,
                                                      stall_checks=stall_checks)
    return SimpleNamespace(phi=st.phi, steps=steps, reason=reason, checks=len(recs), history=recs,
                           margin=margin, inner_sweeps=o32.sweeps, scales=st.scales,
                           pow2_dist=st.dist)
