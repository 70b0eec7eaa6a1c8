"""CPU: the damping pass and the damped solve without a GPU (include/pgmg.h "Damping pass and
damped solve").

* the model (tests/damp_model.py, numpy over the oracle) shows what the feature is for: on the
  robustness right-hand side (oracle.rhs_mt64) plain V-cycles do not reach rtol 1e-6 in 30
  cycles, a damping pass with omega = 1/2 before each cycle does, and the phi a damped solve
  returns (its last check's correction applied) has a residual norm no larger than the last
  check reported;
* the three entries refuse null arguments with PGMG_ERR_ARG before they touch a device;
* pgmg_solve_opts and pgmg_solve_info kept their layout (the damped solve takes omega as an
  argument of its own).
"""
import ctypes as C
import functools
import subprocess

import pytest

from conftest import ROOT
import damp_model
import solve_rule

ERR_ARG = -1


@functools.lru_cache(maxsize=None)
def _damped(N, omega):
    import oracle
    return damp_model.solve_damped(N, f=oracle.rhs_mt64(N), omega=omega, rtol=1e-6, max_cycles=30)


@pytest.mark.parametrize("N", [17, 65, 257])
def test_plain_cycles_stall_and_damped_ones_converge(oracle_mod, N):
    f = oracle_mod.rhs_mt64(N)
    plain = solve_rule.oracle_history(oracle_mod, "V", N, f=f)
    cycles, reason, recs, _ = solve_rule.simulate(plain, rtol=1e-6, max_cycles=30)
    print(f"N={N} plain: {cycles} cycles, reason {reason}, r/r0 {recs[-1][1] / recs[0][1]:.3e}")
    assert (cycles, reason) == (30, solve_rule.MAX_CYCLES)
    m = _damped(N, 0.5)
    print(f"N={N} omega=0.5: {m.cycles} cycles, reason {m.reason}, "
          f"r/r0 {m.history[-1][1] / m.history[0][1]:.3e}")
    assert m.reason == solve_rule.CONVERGED and m.cycles < 30
    assert m.checks == m.cycles + 1 == len(m.history)


@pytest.mark.parametrize("N", [17, 65, 257])
def test_returned_phi_is_no_worse_than_the_last_check(oracle_mod, N):
    m = _damped(N, 0.5)
    after = solve_rule.oracle_res_norm(oracle_mod, m.phi, m.f)
    last = m.history[-1][1]
    print(f"N={N}: last check {last:.6e}, returned phi {after:.6e} ({after / last:.3f} x)")
    assert after <= last * (1 + 1e-12)


def test_damp_model_keeps_the_boundary_and_its_inputs(oracle_mod):
    import numpy as np
    N = 17
    rng = np.random.default_rng(3)
    phi = rng.standard_normal((N, N))
    f = oracle_mod.rhs_mt64(N)
    keep = phi.copy()
    out, norm = damp_model.damp(phi, f, 1.0 / (N - 1), 0.5)
    assert np.array_equal(phi, keep)
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert np.array_equal(out[edge], phi[edge])
    assert norm == solve_rule.oracle_res_norm(oracle_mod, phi, f)
    # omega = 1 on the interior is one Jacobi sweep: x + (h^2/4) (f - A x) = (h^2 f + sum of 4) / 4
    one, _ = damp_model.damp(phi, f, 1.0 / (N - 1), 1.0)
    h = 1.0 / (N - 1)
    jac = phi.copy()
    jac[1:-1, 1:-1] = 0.25 * (h * h * f[1:-1, 1:-1] + phi[1:-1, :-2] + phi[1:-1, 2:]
                              + phi[:-2, 1:-1] + phi[2:, 1:-1])
    assert np.allclose(one, jac, rtol=0, atol=1e-12)


def test_null_arguments(pgmg):
    lib = pgmg.load()
    o, info, v = pgmg.PgmgSolveOpts(), pgmg.PgmgSolveInfo(), C.c_double()
    lib.pgmg_solve_opts_default(C.byref(o))
    assert lib.pgmg_damp(None, 0.5, C.byref(v)) == ERR_ARG
    assert lib.pgmg_damp(None, 0.5, None) == ERR_ARG
    assert lib.pgmg_solve_damped(None, C.byref(o), 0.5, C.byref(info)) == ERR_ARG
    assert lib.pgmg_solve_damped(None, None, 0.5, None) == ERR_ARG
    assert lib.pgmg_damp_time(None, 0.5, 1, C.byref(v), None) == ERR_ARG
    assert lib.pgmg_damp_time(None, 0.5, 0, None, None) == ERR_ARG
    assert b"null" in lib.pgmg_last_error() or b"bad" in lib.pgmg_last_error()


def test_solver_has_the_entries(pgmg):
    import inspect
    assert inspect.signature(pgmg.Solver.solve).parameters["damp"].default == 0.0
    assert inspect.signature(pgmg.Solver.damp).parameters["omega"].default == 0.5
    assert callable(pgmg.Solver.damp_time)


@pytest.mark.parametrize("cname,pyname,size", [("pgmg_solve_opts", "PgmgSolveOpts", 48),
                                               ("pgmg_solve_info", "PgmgSolveInfo", 48)])
def test_struct_layout_unchanged(pgmg, tmp_path, cname, pyname, size):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "pgmg.h"\n'
                   f'int main(void){{printf("%zu", sizeof({cname}));return 0;}}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert got == C.sizeof(getattr(pgmg, pyname)) == size
