"""CPU: the model of pgmg_solve_extrap (tests/extrap_model.py) -- Richardson extrapolation of two
damped second-order solves to fourth order -- and why the entry is built the way it is.

The analytic problem u = sin(p pi x) sin(q pi y) with the exact solution as the frame, eps < 0,
nu = 2, omega = 0.5, rtol = 0, atol = 1e-10 ||f||_2 (interior points of the fine grid; the entry
gives both solves the same options), 40 cycles at most.  e2 is the oracle's rel_error of the fine
second-order solution, e4 that of the extrapolated one.  Measured with the models (fp64):

    p, q       N     e2          e4          e2 / e4    e4(previous N) / e4(N)
    1, 1       33    8.036e-4    1.524e-6    5.3e2
    1, 1       65    2.008e-4    9.638e-8    2.1e3      15.81
    1, 1       129   5.020e-5    6.042e-9    8.3e3      15.95
    1, 1       257   1.255e-5    3.778e-10   3.3e4      15.99
    0.5, 0.5   33    3.610e-5    7.863e-8    4.6e2
    0.5, 0.5   65    9.167e-6    5.068e-9    1.8e3      15.52
    0.5, 0.5   129   2.310e-6    3.211e-10   7.2e3      15.79
    0.5, 0.5   257   5.797e-7    2.019e-11   2.9e4      15.90
    0.3, 2.7   33    4.101e-3    3.598e-5    1.1e2
    0.3, 2.7   65    1.039e-3    2.336e-6    4.4e2      15.40
    0.3, 2.7   129   2.615e-4    1.489e-7    1.8e3      15.69
    0.3, 2.7   257   6.561e-5    9.378e-9    7.0e3      15.88

Both solves take 10-14 damped V-cycles (test_order_table prints the table with -s).
"""
import functools

import numpy as np
import pytest

import extrap_model
import fmg_bc_model
from conftest import assert_bitwise, bits

PQ = [(1.0, 1.0), (0.5, 0.5), (0.3, 2.7)]
SIZES = [33, 65, 129, 257]
RULE = dict(max_cycles=40, rtol=0.0)


def _problem(p, q, N):
    import oracle
    o = oracle.Oracle(p=p, q=q)
    f = o.rhs(N)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    return o, f, phi0


@functools.lru_cache(maxsize=None)
def _run(p, q, N):
    """(e2, e4, cycles of the fine solve, cycles of the coarse solve) of the damped pipeline"""
    o, f, phi0 = _problem(p, q, N)
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    r = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=-1.0, atol=atol, **RULE)
    assert r.fine.reason == r.coarse.reason == 1, (r.fine.reason, r.coarse.reason)
    return o.rel_error(r.phi2), o.rel_error(r.phi), r.fine.cycles, r.coarse.cycles


@pytest.mark.parametrize("p,q", PQ)
def test_order_table(oracle_mod, p, q):
    """Every ratio e4(N) / e4(2N - 1) over N = 33 .. 257 is at least 14 (the limit is 16; the
    margin covers the pre-asymptotic 33 -> 65 step), and at N = 129 the extrapolated error is
    at most 1/1000 of the second-order one."""
    rows = [_run(p, q, N) for N in SIZES]
    for N, (e2, e4, kf, kc) in zip(SIZES, rows):
        print(f"p={p} q={q} N={N}: e2 {e2:.4e} e4 {e4:.4e} gain {e2 / e4:.4e} "
              f"cycles fine {kf} coarse {kc}")
    for (Na, a), (Nb, b) in zip(zip(SIZES, rows), zip(SIZES[1:], rows[1:])):
        print(f"p={p} q={q}: e4({Na}) / e4({Nb}) = {a[1] / b[1]:.3f}")
        assert a[1] / b[1] >= 14.0, (p, q, Na, Nb, a[1], b[1])
    e2, e4 = rows[SIZES.index(129)][:2]
    assert e4 <= e2 / 1000.0, (p, q, e2, e4)


def test_undamped_cycles_cannot_feed_the_extrapolation(oracle_mod):
    """Why omega is mandatory: 150 plain V-cycles on both grids (N = 129, p = q = 0.5, eps < 0, the
    exact frame) leave an algebraic error that the extrapolation inherits: e4 is more than 10
    times the damped pipeline's (measured 1.97e-8 against 3.21e-10 in the issue's run)."""
    p = q = 0.5
    N = 129
    sols = []
    for n in ((N + 1) // 2, N):
        o = oracle_mod.Oracle(eps=-1.0, p=p, q=q)
        f = o.rhs(n)
        phi = fmg_bc_model.set_frame(np.zeros((n, n)), o.exact(n))
        for _ in range(150):
            o.v_cycle(phi, f)
        sols.append(phi)
    o = oracle_mod.Oracle(p=p, q=q)
    e4_plain = o.rel_error(extrap_model.extrapolate(sols[1], sols[0]))
    e4_damped = _run(p, q, N)[1]
    print(f"undamped e4 {e4_plain:.4e}, damped e4 {e4_damped:.4e}, x{e4_plain / e4_damped:.1f}")
    assert e4_plain > 10.0 * e4_damped, (e4_plain, e4_damped)


def test_injected_problem_is_the_half_resolution_problem(oracle_mod):
    """f[::2, ::2] and the injected frame are bit for bit the analytic problem of (N + 1) / 2
    points: h is a power of two, so 2i * h and i * (2h) are the same double."""
    for p, q in PQ:
        o, f, phi0 = _problem(p, q, 65)
        oc, fc, phic = _problem(p, q, 33)
        assert_bitwise(np.ascontiguousarray(f[::2, ::2]), fc, f"f p={p} q={q}")
        assert_bitwise(np.ascontiguousarray(phi0[::2, ::2]), phic, f"frame p={p} q={q}")


@pytest.mark.parametrize("Nc", [5, 9, 33])
def test_extrapolate_keeps_the_frame_and_its_inputs(oracle_mod, Nc):
    Nf = 2 * Nc - 1
    rng = np.random.default_rng(Nc)
    fine, coarse = rng.standard_normal((Nf, Nf)), rng.standard_normal((Nc, Nc))
    fine[0, 3] = fine[-1, 0] = fine[2, 0] = fine[4, -1] = -0.0
    keep_f, keep_c = fine.copy(), coarse.copy()
    out = extrap_model.extrapolate(fine, coarse)
    assert_bitwise(fine, keep_f, "fine is left untouched")
    assert_bitwise(coarse, keep_c, "coarse is left untouched")
    for name, sl in (("top", np.s_[0, :]), ("bottom", np.s_[-1, :]), ("left", np.s_[:, 0]),
                     ("right", np.s_[:, -1])):
        assert np.array_equal(bits(out[sl]), bits(fine[sl])), name
    # the coincident interior points: F + (F - C) * K3, nothing interpolated
    want = fine[2:-1:2, 2:-1:2] + (fine[2:-1:2, 2:-1:2] - coarse[1:-1, 1:-1]) * extrap_model.K3
    assert_bitwise(np.ascontiguousarray(out[2:-1:2, 2:-1:2]), np.ascontiguousarray(want),
                   "coincident points")
    # a cubic polynomial of the difference is reproduced: with coarse = fine[::2, ::2] - 3 P the
    # correction is P itself up to rounding
    y, x = np.meshgrid(np.linspace(0, 1, Nf), np.linspace(0, 1, Nf), indexing="ij")
    P = 1.0 + x - 2.0 * y + x * y + x ** 3 - y ** 3 + x ** 2 * y
    out = extrap_model.extrapolate(fine, fine[::2, ::2] - 3.0 * P[::2, ::2])
    assert np.max(np.abs(out[1:-1, 1:-1] - (fine + P)[1:-1, 1:-1])) < 1e-13


def test_k3_is_the_double_nearest_a_third():
    assert extrap_model.K3 == 1.0 / 3.0 and bits(np.array([extrap_model.K3]))[0] == 0x3FD5555555555555


@pytest.mark.parametrize("N,p,q,eps,want_hash,sweeps", [
    (33, 0.5, 0.5, -1.0, "12323d708e87e6c2", (412, 299)),
    (65, 0.3, 2.7, 1e-7, "5dd579abb34f2730", (408, 310)),
])
def test_model_checkpoints(oracle_mod, N, p, q, eps, want_hash, sweeps):
    o, f, phi0 = _problem(p, q, N)
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    r = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=eps, atol=atol, **RULE)
    print(N, oracle_mod.fnv_hash(r.phi), (r.fine.sweeps, r.coarse.sweeps))
    assert oracle_mod.fnv_hash(r.phi) == want_hash
    assert (r.fine.sweeps, r.coarse.sweeps) == sweeps
