"""CPU: the model of pgmg_fmg_bc (tests/fmg_bc_model.py) -- full multigrid that keeps phi's
Dirichlet frame -- and why the entry exists.

The analytic problem with non-integer p, q has an exact solution that is not zero on the far
boundary.  rel_error is ||phi - u|| / ||u|| as orc_rel_error computes it; "disc", the
discretisation error, is the same quantity after 40 oracle V-cycles from the zero interior with
the exact frame.  Measured with the models (fp64, nu = 2, eps 1e-7), error / disc:

    p, q        fmg_bc N=33   N=129   N=257     zero-frame fmg, N=257
    0.5, 0.5    0.921         0.921   0.921     1.5e6
    1.5, 0.5    0.970         0.971   0.971     4.0e4
    0.3, 2.7    0.994         0.997   0.997     8.4e3
"""
import functools

import numpy as np
import pytest

import fmg_bc_model
import fmg_damped_model
import fmg_model
from conftest import assert_bitwise

PQ = [(0.5, 0.5), (1.5, 0.5), (0.3, 2.7)]


def _bits_equal(a, b, what):
    assert a.dtype == b.dtype, (what, a.dtype, b.dtype)
    assert_bitwise(a.astype(np.float64), b.astype(np.float64), what)


def _f(oracle_mod, kind, N, dtype="f64"):
    if kind == "mt":
        return oracle_mod.rhs_mt64(N, dtype=dtype)
    return oracle_mod.Oracle(dtype=dtype).rhs(N)


@pytest.mark.parametrize("kind,N,dtype", [("analytic", 33, "f64"), ("analytic", 129, "f64"),
                                          ("mt", 129, "f64"), ("analytic", 33, "f32")])
@pytest.mark.parametrize("omega", [0.0, 0.5])
def test_zero_frame_is_the_zero_boundary_model(oracle_mod, kind, N, dtype, omega):
    """With a frame of +0.0 the new model is fmg_model.fmg (omega = 0) or
    fmg_damped_model.fmg_damped bit for bit, sweeps and exits included; the interior of phi0 is
    random to show it is not read."""
    f = _f(oracle_mod, kind, N, dtype)
    phi0 = np.random.default_rng(N).uniform(-1, 1, (N, N))
    phi0[0, :] = phi0[-1, :] = phi0[:, 0] = phi0[:, -1] = 0.0
    a, b = oracle_mod.Oracle(dtype=dtype), oracle_mod.Oracle(dtype=dtype)
    got = fmg_bc_model.fmg_bc(a, phi0, f, 2, omega)
    want = fmg_model.fmg(b, f, 2) if omega == 0.0 else fmg_damped_model.fmg_damped(b, f, 2, omega)
    _bits_equal(got, want, f"{kind} N={N} {dtype} omega={omega}")
    assert (a.sweeps, a.early_exits) == (b.sweeps, b.early_exits)


@pytest.mark.parametrize("omega", [0.0, 0.5])
@pytest.mark.parametrize("N", [33, 129])
def test_frame_comes_back_bitwise_and_the_interior_is_ignored(oracle_mod, N, omega):
    o = oracle_mod.Oracle(p=0.5, q=0.5)
    f = o.rhs(N)
    rng = np.random.default_rng(11)
    phi0 = rng.uniform(-1, 1, (N, N))
    fmg_bc_model.set_frame(phi0, o.exact(N))
    keep = phi0.copy()
    u = fmg_bc_model.fmg_bc(o, phi0, f, 2, omega)
    assert_bitwise(phi0, keep, "phi0 is left untouched")
    for name, sl in (("top", np.s_[0, :]), ("bottom", np.s_[-1, :]), ("left", np.s_[:, 0]),
                     ("right", np.s_[:, -1])):
        assert_bitwise(u[sl], phi0[sl], f"{name} line of the frame, N={N}")
    other = phi0.copy()
    other[1:-1, 1:-1] = rng.uniform(-5, 5, (N - 2, N - 2))
    u2 = fmg_bc_model.fmg_bc(oracle_mod.Oracle(p=0.5, q=0.5), other, f, 2, omega)
    assert_bitwise(u2, u, "another interior of phi0")


@functools.lru_cache(maxsize=None)
def _disc(N, p, q):
    """The discretisation error: 40 oracle V-cycles from the start fmg_bc is given."""
    import oracle
    o = oracle.Oracle(p=p, q=q)
    f = o.rhs(N)
    phi = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    for _ in range(40):
        o.v_cycle(phi, f)
    return o.rel_error(phi)


def _ratio(oracle_mod, N, p, q, omega=0.0):
    o = oracle_mod.Oracle(p=p, q=q)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    u = fmg_bc_model.fmg_bc(o, phi0, o.rhs(N), 2, omega)
    return o.rel_error(u), _disc(N, p, q)


@pytest.mark.parametrize("N", [33, 129, 257])
@pytest.mark.parametrize("p,q", PQ)
def test_fmg_bc_reaches_discretisation_error(oracle_mod, p, q, N):
    err, disc = _ratio(oracle_mod, N, p, q)
    print(f"p={p} q={q} N={N}: error {err:.4e}, disc {disc:.4e}, ratio {err / disc:.3f}")
    assert err <= disc, (p, q, N, err, disc)


@pytest.mark.parametrize("p,q", PQ)
def test_damped_fmg_bc_reaches_discretisation_error(oracle_mod, p, q):
    N = 129
    err, disc = _ratio(oracle_mod, N, p, q, omega=0.5)
    print(f"damped p={p} q={q} N={N}: error {err:.4e}, disc {disc:.4e}, ratio {err / disc:.3f}")
    assert err <= disc, (p, q, N, err, disc)


def test_zero_frame_fmg_misses_the_problem_with_boundary_data(oracle_mod):
    """The gap the entry closes (it holds before and after): the zero-boundary climb on
    p = q = 0.5 at N = 129 is more than 100 x the discretisation error away."""
    N, p, q = 129, 0.5, 0.5
    o = oracle_mod.Oracle(p=p, q=q)
    u = fmg_model.fmg(o, o.rhs(N), 2)
    err, disc = o.rel_error(u), _disc(N, p, q)
    print(f"zero-frame fmg p={p} q={q} N={N}: error {err:.4e} = {err / disc:.3e} x disc")
    assert err > 100 * disc, (err, disc)


@pytest.mark.parametrize("N,p,q,want_hash,sweeps", [(33, 0.5, 0.5, "cd6ebd4b92c4f889", 136),
                                                    (129, 0.3, 2.7, "c81e68d5fbebf373", 252)])
def test_model_checkpoints(oracle_mod, N, p, q, want_hash, sweeps):
    o = oracle_mod.Oracle(p=p, q=q)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    u = fmg_bc_model.fmg_bc(o, phi0, o.rhs(N), 2)
    assert oracle_mod.fnv_hash(u) == want_hash
    assert (o.sweeps, o.early_exits) == (sweeps, 0)
