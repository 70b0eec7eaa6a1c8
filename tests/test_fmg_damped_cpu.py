"""CPU: the model of pgmg_fmg_damped (tests/fmg_damped_model.py) -- why the entry exists.

||r|| / ||f|| over the interior points after FMG with nu = 2 on oracle.rhs_mt64, measured with
the models (fp64, eps 1e-7, omega = 1/2):

    N      plain FMG   damped FMG   ratio
    17     9.6e-2      1.18e-3      82
    33     9.0e-2      1.19e-3      76
    65     1.32e-1     1.03e-3      129
    129    1.42e-1     9.5e-4       149
    257    1.36e-1     9.0e-4       152
    513    1.39e-1     8.9e-4       156

The undamped smoother leaves the checkerboard error of every level untouched; one damping pass
after each V-cycle of the climb removes it.  On the analytic problem nothing is lost: damped FMG
lands at 0.90 x the discretisation error, as plain FMG does (tests/test_fmg_cpu.py).
omega -> 0 is not compared with plain FMG: the entry rejects omega = 0.
"""
import functools

import numpy as np
import pytest

import fmg_damped_model
import fmg_model


@functools.lru_cache(maxsize=None)
def _mt(N):
    import oracle
    f = oracle.rhs_mt64(N)
    h = 1.0 / (N - 1)
    damped = fmg_damped_model.fmg_damped(oracle.Oracle(), f, 2, 0.5)
    plain = fmg_model.fmg(oracle.Oracle(), f, 2)
    return (fmg_damped_model.rel_residual(damped, f, h), fmg_damped_model.rel_residual(plain, f, h))


@pytest.mark.parametrize("N", [17, 33, 65, 129])
def test_damped_fmg_residual_on_a_general_f(oracle_mod, N):
    damped, plain = _mt(N)
    print(f"N={N}: damped {damped:.3e}, plain {plain:.3e}, ratio {plain / damped:.0f}")
    assert damped <= 2e-3, (N, damped)


@pytest.mark.parametrize("N", [17, 33, 65, 129])
def test_plain_fmg_stops_short_on_a_general_f(oracle_mod, N):
    damped, plain = _mt(N)
    assert plain >= 5e-2, (N, plain)


@pytest.mark.parametrize("N", [33, 129])
def test_damped_fmg_reaches_discretisation_error(oracle_mod, N):
    phi, o = oracle_mod.run_cycles("V", N, 40)
    disc = o.rel_error(phi)
    u, od = fmg_damped_model.fmg_damped_analytic(N, nu=2, omega=0.5)
    ratio = od.rel_error(u) / disc
    print(f"N={N}: disc {disc:.4e}, damped FMG {ratio:.3f} x disc")
    assert 0.85 <= ratio <= 0.95, (N, ratio)


def test_model_damps_every_cycle_of_the_climb_only(oracle_mod):
    """The model by hand at N = 9 (n_coarse 5: one climb step), nu = 2: the coarsest level is
    fmg_model's, each cycle of level 0 is followed by damp_model.damp with that level's h."""
    import damp_model
    o = oracle_mod.Oracle(n_coarse=5)
    f = oracle_mod.rhs_mt64(9)
    h = 1.0 / 8
    f1 = fmg_model.restrict(f, o)
    u = np.zeros_like(f1)
    for _ in range(2):
        o.v_cycle(u, f1, 2 * h)
    u = fmg_model.cubic(u)
    for _ in range(2):
        o.v_cycle(u, f, h)
        u, _ = damp_model.damp(u, f, h, 0.5)
    o2 = oracle_mod.Oracle(n_coarse=5)
    got = fmg_damped_model.fmg_damped(o2, f, 2, 0.5)
    assert np.array_equal(got, u) and o2.sweeps == o.sweeps
    assert not np.array_equal(got, fmg_model.fmg(oracle_mod.Oracle(n_coarse=5), f, 2))
