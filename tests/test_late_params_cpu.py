"""CPU: the models of the late entries with explicit parameters, and the conditions on the inputs
of tests/test_gpu_late_params.py -- from the models over the CPU oracle alone.

1. damp_model.solve_damped and extrap_model.solve_extrap take the context's mesh width and the
   oracle's fields; with none given, or with pgmg_config's defaults spelled out, they return the
   bits they returned before they took them.
2. The case tables of the GPU module's solves (SOLVE_CASES, EX_CASES): every solve, fine and
   half-resolution, ends with PGMG_STOP_CONVERGED (the one F case at its cycle cap); the smallest
   margin of any comparison the stop rule made exceeds 100 * norm_tol(N), so that the device's
   decisions, taken on norms summed in another order, are comparable with the model's at all;
   among the eps = 1e-7 cases at least a third cut smoother calls short and at least one cuts
   none.  A case that fails a condition is replaced in the table, never skipped.
3. What the parameter sets are there for: asymmetric results where p != q, a non-zero frame
   where the table says so.
"""
import numpy as np
import pytest

import damp_model
import extrap_model
import fmg_bc_model
import oracle
from conftest import assert_bitwise
from solve_rule import CONVERGED, MAX_CYCLES, norm_tol
from test_gpu_late_params import (EX_CASES, FMG_SETS, SOLVE_CASES, _ex_model, _ex_problem,
                                  _fmg_problem, _id, _solve_start)
from test_gpu_problem_params import prm


def _defaults(N):
    return dict(a=1.0, p=1.0, q=1.0, h0=1.0 / (N - 1), alpha=3, n_coarse=5, coarse_iter=10, v1=1,
                v2=1)


def _same_solve(a, b, what):
    assert_bitwise(a.phi, b.phi, what)
    assert a.history == b.history or repr(a.history) == repr(b.history), what   # (nan entries)
    assert (a.cycles, a.reason, a.checks) == (b.cycles, b.reason, b.checks), what
    assert (a.sweeps, a.exits) == (b.sweeps, b.exits), what


@pytest.mark.parametrize("kind,N,dtype,mt,error", [("V", 65, "f64", False, True),
                                                   ("W", 65, "f64", True, False),
                                                   ("V", 129, "f32", False, False),
                                                   ("V", 33, "f64", True, False)])
def test_solve_damped_explicit_defaults_are_the_defaults(kind, N, dtype, mt, error):
    f = oracle.rhs_mt64(N, dtype=dtype) if mt else None
    rule = dict(rtol=1e-3 if dtype == "f32" else 1e-6, max_cycles=30)
    plain = damp_model.solve_damped(N, f=f, kind=kind, dtype=dtype, error=error, **rule)
    spelt = damp_model.solve_damped(N, f=f, kind=kind, dtype=dtype, error=error, **_defaults(N),
                                    **rule)
    assert plain.cycles >= 3
    _same_solve(plain, spelt, f"solve_damped {kind} N={N} {dtype}")
    assert plain.exits == plain.oracle.cut_exits


@pytest.mark.parametrize("N,mt,eps", [(33, True, 1e-7), (65, False, -1.0), (65, True, 1e-7)])
def test_solve_extrap_explicit_defaults_are_the_defaults(N, mt, eps):
    if mt:
        f, phi0 = np.array(oracle.rhs_mt64(N)), np.zeros((N, N))
    else:
        o = oracle.Oracle(p=0.5, q=0.5)
        f, phi0 = o.rhs(N), fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    rule = dict(rtol=0.0, atol=1e-10 * float(np.linalg.norm(f[1:-1, 1:-1])), max_cycles=40)
    plain = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=eps, **rule)
    spelt = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=eps, **_defaults(N), **rule)
    assert_bitwise(plain.phi, spelt.phi, "the extrapolated phi")
    assert_bitwise(plain.phi2, spelt.phi2, "the fine second-order phi")
    _same_solve(plain.fine, spelt.fine, f"fine N={N}")
    _same_solve(plain.coarse, spelt.coarse, f"coarse N={N}")


def _solves():
    """(id, N, eps, the model's namespace, capped) of every solve the GPU module compares"""
    out = []
    for c in SOLVE_CASES:
        out.append((f"solve_damped {_id(c)}", c.N, c.eps, _solve_start(c)[1], c.capped))
    for c in EX_CASES:
        m = _ex_model(c)
        out.append((f"solve_extrap {_id(c)} fine", c.N, c.eps, m.fine, False))
        out.append((f"solve_extrap {_id(c)} coarse", (c.N + 1) // 2, c.eps, m.coarse, False))
    return out


def test_every_solve_converges_with_a_comparable_margin():
    worst = (np.inf, None)
    for what, N, eps, m, capped in _solves():
        print(f"{what}: {m.cycles} cycles, reason {m.reason}, margin {m.margin:.3e}, "
              f"{m.exits} exits")
        assert m.reason == (MAX_CYCLES if capped else CONVERGED), (what, m.reason, m.cycles)
        assert m.margin > 100 * norm_tol(N), (what, m.margin)
        assert capped or m.cycles >= 2, (what, m.cycles)    # (a solve with nothing to decide)
        worst = min(worst, (m.margin, what))
    print("smallest margin:", worst)
    assert sum(1 for s in _solves() if s[4]) == 1


def test_exits_are_mixed_among_the_eps_1e7_cases():
    """The solves' own exits (damp_model's oracle; the FMG start has its own counters)."""
    for table, get in ((SOLVE_CASES, lambda c: _solve_start(c)[1].oracle.cut_exits),
                       (EX_CASES, lambda c: _ex_model(c).fine.oracle.cut_exits)):
        exits = [get(c) for c in table if c.eps == 1e-7]
        print(exits)
        assert 3 * sum(1 for e in exits if e > 0) >= len(exits), exits
    exits = [_solve_start(c)[1].oracle.cut_exits for c in SOLVE_CASES if c.eps == 1e-7] + \
            [_ex_model(c).fine.oracle.cut_exits for c in EX_CASES if c.eps == 1e-7]
    assert any(e == 0 for e in exits), exits
    # eps < 0: no check fires
    assert all(_ex_model(c).fine.exits == 0 and _ex_model(c).coarse.exits == 0
               for c in EX_CASES if c.eps < 0)


def test_asymmetric_cases_have_asymmetric_results():
    checked = 0
    for c in SOLVE_CASES:
        kw = prm(c.name, c.N)
        if kw["p"] != kw["q"]:
            phi = _solve_start(c)[1].phi
            assert not np.array_equal(phi, phi.T), _id(c)
            checked += 1
    for c in EX_CASES:
        kw = prm(c.name, c.N)
        if kw["p"] != kw["q"] and c.f == "analytic":
            phi = _ex_model(c).phi
            assert not np.array_equal(phi, phi.T), _id(c)
            checked += 1
    assert checked >= 30, checked


def test_frames_are_nonzero_where_the_tables_say_so():
    """The analytic problems' frame (the exact solution): ~1e-13 at most for integer p, q at the
    default mesh width; for P5 and every H set above 0.01 somewhere on row and on column N - 1
    (H2 is the smallest: sin(p pi (N - 1) / N) ~ p pi / N >= 0.024 up to N = 257)."""
    for name in FMG_SETS:
        for N, dtype in ((65, "f64"), (129, "f32"), (257, "f64")):
            g = _fmg_problem(N, name, dtype, "analytic")[0]
            far = max(np.abs(g[N - 1]).max(), np.abs(g[:, N - 1]).max())
            if "+H" in name or name == "P5":
                assert np.abs(g[N - 1]).max() > 0.01 and np.abs(g[:, N - 1]).max() > 0.01, (name, N)
            else:
                assert far < 1e-9, (name, N, far)
    for c in EX_CASES:
        if c.f == "analytic" and "+H" in c.name:
            g = _ex_problem(c.N, c.name, c.f)[1]
            assert np.abs(g[c.N - 1]).max() > 0.01 and np.abs(g[:, c.N - 1]).max() > 0.01, _id(c)
