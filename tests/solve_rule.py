"""Python restatement of pgmg_solve's stop rule (include/pgmg.h, csrc/pgmg_stop.h), shared by
tests/test_solve_cpu.py and the GPU solve / monitor tests, and the oracle's norms they compare
against.  Not a test module."""
import ctypes as C
import math

import numpy as np

CONVERGED, MAX_CYCLES, STALLED, NONFINITE = 1, 2, 3, 4
REASON = {1: "CONVERGED", 2: "MAX_CYCLES", 3: "STALLED", 4: "NONFINITE"}


def _margin(a, b):
    """relative distance of the two sides of a comparison the rule made"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else math.inf


def simulate(res_at, max_cycles=30, check_every=1, rtol=1e-3, atol=0.0, stall_ratio=0.0,
             stall_checks=2):
    """Run the rule on norms res_at(check index, cycles run).  Returns (cycles, reason,
    [(cycles, norm) per check], smallest relative margin of any comparison of two norms made;
    inf when none was).  res_at may return None: the history ran out (reason 0)."""
    k, streak, r0, prev = 0, 0, None, None
    recs, margin = [], math.inf
    i = 0
    while True:
        r = res_at(i, k)
        if r is None:
            return k, 0, recs, margin
        recs.append((k, r))
        if i == 0:
            r0 = r
        if not math.isfinite(r):
            return k, NONFINITE, recs, margin
        target = max(atol, rtol * r0)
        if not (r == 0 and target == 0):   # (0 <= 0: exact zeros on both sides, nothing to round)
            margin = min(margin, _margin(r, target))
        if r <= target:
            return k, CONVERGED, recs, margin
        if i >= 1 and stall_ratio > 0:
            margin = min(margin, _margin(r, stall_ratio * prev))
            streak = streak + 1 if r > stall_ratio * prev else 0
            if streak >= stall_checks:
                return k, STALLED, recs, margin
        if k >= max_cycles:
            return k, MAX_CYCLES, recs, margin
        prev = r
        k += min(check_every, max_cycles - k)
        i += 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def norm_tol(N):
    """Two summation orders of n non-negative terms differ by at most (n - 1) 2^-52 relative;
    the monitor's per-point terms are the oracle's, so norms agree within N^2 2^-52."""
    return N * N * 2.0 ** -52


def close(got, want, N):
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= norm_tol(N) * abs(want)


def oracle_res_norm(oracle_mod, phi, f, dtype="f64", h=None):
    """orc_residual_norm of the matching dtype library"""
    dt = np.float32 if dtype == "f32" else np.float64
    N = phi.shape[0]
    x = np.ascontiguousarray(phi, dtype=dt)
    ff = np.ascontiguousarray(f, dtype=dt)
    return oracle_mod.lib(dtype).orc_residual_norm(_p(x), _p(ff), N, 1.0 / (N - 1) if h is None else h)


def oracle_history(oracle_mod, kind, N, f=None, dtype="f64", eps=1e-7):
    """res_at for simulate(): the oracle's residual norm after k cycles of `kind` from
    phi = 0 (computed on demand, cached); .phi(k) is the iterate and .sweeps(k) the sweeps."""
    o = oracle_mod.Oracle(eps=eps, dtype=dtype)
    ff = o.rhs(N) if f is None else np.ascontiguousarray(f, dtype=o.dt)
    state = {"phi": np.zeros((N, N), dtype=o.dt), "k": 0}
    cache, phis, sweeps = {}, {}, {}

    def advance(k):
        while state["k"] < k:
            if kind == "V":
                o.v_cycle(state["phi"], ff)
            elif kind == "W":
                o.w_cycle(state["phi"], ff)
            else:
                o.f_cycle_outer(state["phi"])
            state["k"] += 1
        assert state["k"] == k

    def res_at(i, k):
        if k not in cache:
            advance(k)
            cache[k] = oracle_res_norm(oracle_mod, state["phi"], ff, dtype)
            phis[k] = state["phi"].copy()
            sweeps[k] = o.sweeps
        return cache[k]

    res_at.phi = lambda k: phis[k]
    res_at.sweeps = lambda k: sweeps[k]
    res_at.f = ff
    res_at.oracle = o
    return res_at
