"""CPU: the model of pgmg_gradient (tests/grad_model.py) and what the field of a solve is worth.

The analytic problem u = sin(p pi x) sin(q pi y) with the exact solution as the frame, solved as
tests/test_extrap_cpu.py solves it (nu = 2, omega = 0.5, eps < 0, atol = 1e-10 ||f||, at most 40
cycles).  phi2 is the second-order solution, phi4 the extrapolated one, o2 / o4 the order of the
gradient's stencils.  The error is sqrt(sum (gx - u_x)^2 + (gy - u_y)^2) / sqrt(sum u_x^2 + u_y^2)
over all N^2 points, frame included.  Measured with the models (fp64; test_field_table prints
the table with -s):

    p, q       N     phi2, o2    phi2, o4    phi4, o2    phi4, o4    phi4/o4 ratio to previous N
    1, 1       33    1.568e-3    7.996e-4    1.866e-3    8.087e-6
    1, 1       65    3.145e-4    2.006e-4    4.365e-4    4.149e-7    19.49
    1, 1       129   6.619e-5    5.019e-5    1.049e-4    2.244e-8    18.49
    1, 1       257   1.470e-5    1.255e-5    2.568e-5    1.276e-9    17.58
    0.5, 0.5   33    4.236e-4    8.073e-5    4.365e-4    6.026e-7
    0.5, 0.5   65    1.005e-4    1.994e-5    1.049e-4    3.655e-8    16.49
    0.5, 0.5   129   2.438e-5    4.954e-6    2.568e-5    2.286e-9    15.99
    0.5, 0.5   257   6.000e-6    1.234e-6    6.348e-6    1.451e-10   15.76
    0.3, 2.7   33    1.089e-2    4.651e-3    1.254e-2    3.188e-4
    0.3, 2.7   65    2.433e-3    1.182e-3    3.031e-3    1.696e-5    18.80
    0.3, 2.7   129   5.599e-4    2.965e-4    7.393e-4    9.281e-7    18.28
    0.3, 2.7   257   1.330e-4    7.413e-5    1.822e-4    5.311e-8    17.47

Only the fourth-order gradient of the fourth-order solve is fourth order.
"""
import functools

import numpy as np
import pytest

import extrap_model
import fmg_bc_model
import grad_model
from conftest import bits

PQ = [(1.0, 1.0), (0.5, 0.5), (0.3, 2.7)]
SIZES = [33, 65, 129, 257]
RULE = dict(max_cycles=40, rtol=0.0)

# the issue's table: (p, q, N) -> (phi2/o2, phi2/o4, phi4/o2, phi4/o4), four digits each
TABLE = {
    (1.0, 1.0, 33): (1.568e-3, 7.996e-4, 1.866e-3, 8.087e-6),
    (1.0, 1.0, 65): (3.145e-4, 2.006e-4, 4.365e-4, 4.149e-7),
    (1.0, 1.0, 129): (6.619e-5, 5.019e-5, 1.049e-4, 2.244e-8),
    (1.0, 1.0, 257): (1.470e-5, 1.255e-5, 2.568e-5, 1.276e-9),
    (0.5, 0.5, 33): (4.236e-4, 8.073e-5, 4.365e-4, 6.026e-7),
    (0.5, 0.5, 65): (1.005e-4, 1.994e-5, 1.049e-4, 3.655e-8),
    (0.5, 0.5, 129): (2.438e-5, 4.954e-6, 2.568e-5, 2.286e-9),
    (0.5, 0.5, 257): (6.000e-6, 1.234e-6, 6.348e-6, 1.451e-10),
    (0.3, 2.7, 33): (1.089e-2, 4.651e-3, 1.254e-2, 3.188e-4),
    (0.3, 2.7, 65): (2.433e-3, 1.182e-3, 3.031e-3, 1.696e-5),
    (0.3, 2.7, 129): (5.599e-4, 2.965e-4, 7.393e-4, 9.281e-7),
    (0.3, 2.7, 257): (1.330e-4, 7.413e-5, 1.822e-4, 5.311e-8),
}


def exact_gradient(p, q, N):
    """(u_x, u_y) of u = sin(p pi x) sin(q pi y) on the N x N grid of the unit square, element
    (j, i) at x = i h, y = j h."""
    t = np.arange(N) / (N - 1)
    sx, cx = np.sin(p * np.pi * t), np.cos(p * np.pi * t)
    sy, cy = np.sin(q * np.pi * t), np.cos(q * np.pi * t)
    return p * np.pi * np.outer(sy, cx), q * np.pi * np.outer(cy, sx)


def field_error(phi, p, q, order):
    N = phi.shape[0]
    gx, gy = grad_model.gradient(phi, 1.0 / (N - 1), order)
    ux, uy = exact_gradient(p, q, N)
    return float(np.sqrt(np.sum((gx - ux) ** 2 + (gy - uy) ** 2)) / np.sqrt(np.sum(ux ** 2 + uy ** 2)))


@functools.lru_cache(maxsize=None)
def _row(p, q, N):
    """(phi2/o2, phi2/o4, phi4/o2, phi4/o4) of the damped pipeline"""
    import oracle
    o = oracle.Oracle(p=p, q=q)
    f = o.rhs(N)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    r = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=-1.0, atol=atol, **RULE)
    assert r.fine.reason == r.coarse.reason == 1, (r.fine.reason, r.coarse.reason)
    return (field_error(r.phi2, p, q, 2), field_error(r.phi2, p, q, 4),
            field_error(r.phi, p, q, 2), field_error(r.phi, p, q, 4))


@pytest.mark.parametrize("p,q", PQ)
def test_field_table(oracle_mod, p, q):
    """The issue's table, to its four digits; every phi4/o4 ratio per doubling is at least 14 (the
    limit is 16), at N = 257 phi4/o4 is at most 1/1000 of phi2/o2, and the mixed pairs (phi4/o2,
    phi2/o4) are second order: ratios between 3.5 and 5."""
    rows = [_row(p, q, N) for N in SIZES]
    for N, r in zip(SIZES, rows):
        print(f"p={p} q={q} N={N}: phi2/o2 {r[0]:.3e} phi2/o4 {r[1]:.3e} phi4/o2 {r[2]:.3e} "
              f"phi4/o4 {r[3]:.3e}")
        for got, want in zip(r, TABLE[p, q, N]):
            assert abs(got - want) <= 1e-3 * want, (p, q, N, r, TABLE[p, q, N])
    for (Na, a), (Nb, b) in zip(zip(SIZES, rows), zip(SIZES[1:], rows[1:])):
        print(f"p={p} q={q} {Na} -> {Nb}: phi4/o4 x{a[3] / b[3]:.2f}, phi4/o2 x{a[2] / b[2]:.2f}, "
              f"phi2/o4 x{a[1] / b[1]:.2f}")
        assert a[3] / b[3] >= 14.0, (p, q, Na, Nb, a[3], b[3])
        assert 3.5 <= a[2] / b[2] <= 5.0, (p, q, Na, Nb, a[2], b[2])
        assert 3.5 <= a[1] / b[1] <= 5.0, (p, q, Na, Nb, a[1], b[1])
    last = rows[SIZES.index(257)]
    assert last[3] <= last[0] / 1000.0, (p, q, last)


@pytest.mark.parametrize("p,q", PQ)
def test_order_on_the_exact_solution(oracle_mod, p, q):
    """On the exact u the stencils alone: ratios per doubling >= 14 (order 4) and >= 3.8
    (order 2) over N = 33 .. 257."""
    err = {}
    for N in SIZES:
        u = oracle_mod.Oracle(p=p, q=q).exact(N)
        err[N] = (field_error(u, p, q, 2), field_error(u, p, q, 4))
    for Na, Nb in zip(SIZES, SIZES[1:]):
        r2, r4 = err[Na][0] / err[Nb][0], err[Na][1] / err[Nb][1]
        print(f"p={p} q={q} {Na} -> {Nb}: order 2 x{r2:.2f}, order 4 x{r4:.2f}")
        assert r2 >= 3.8 and r4 >= 14.0, (p, q, Na, Nb, r2, r4)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("N", [5, 9, 33])
def test_exact_on_polynomials(order, N):
    """Order 2 reproduces the gradient of x^2 y, order 4 that of x^4 + x^3 y^2, on a non-dyadic h,
    within 1e-12 relative, the frame included (the one-sided stencils have the same order)."""
    h = 0.7 / (N - 1)
    y, x = np.meshgrid(np.arange(N) * h, np.arange(N) * h, indexing="ij")
    if order == 2:
        u, ux, uy = x ** 2 * y, 2 * x * y, x ** 2
    else:
        u, ux, uy = x ** 4 + x ** 3 * y ** 2, 4 * x ** 3 + 3 * x ** 2 * y ** 2, 2 * x ** 3 * y
    gx, gy = grad_model.gradient(u, h, order)
    for g, want, name in ((gx, ux, "gx"), (gy, uy, "gy")):
        assert np.max(np.abs(g - want)) <= 1e-12 * np.max(np.abs(want)), (name, order, N)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", [2, 4])
def test_scale_minus_one_flips_the_sign_bit(order, dtype):
    rng = np.random.default_rng(order)
    phi = rng.standard_normal((17, 17))
    phi[2:10, 3:11] = 0.0       # differences of exactly zero: +0 and -0
    phi[13, 13], phi[12, 2], phi[0, 7] = np.inf, np.nan, -np.inf
    a = grad_model.gradient(phi, 0.7 / 16, order, 1.0, dtype)
    b = grad_model.gradient(phi, 0.7 / 16, order, -1.0, dtype)
    for ga, gb in zip(a, b):
        ok = ~np.isnan(ga)
        assert np.array_equal(np.isnan(ga), np.isnan(gb))
        assert ok.sum() > 200 and np.count_nonzero(ga[ok] == 0) >= 4
        assert np.array_equal(bits(ga)[ok] ^ np.uint64(1 << 63), bits(gb)[ok])


def test_model_leaves_phi_alone_and_norm_is_the_double_sum():
    rng = np.random.default_rng(7)
    phi = rng.standard_normal((9, 9))
    keep = phi.copy()
    gx, gy = grad_model.gradient(phi, 0.125, 4, 0.37)
    assert np.array_equal(bits(phi), bits(keep))
    assert grad_model.norm(gx, gy) == float(np.sqrt(np.sum(gx * gx) + np.sum(gy * gy)))
    assert grad_model.norm(gx, None) == float(np.sqrt(np.sum(gx * gx)))
    # the fp32 model computes in float32 and returns the widened values
    g32 = grad_model.gradient(phi, 0.125, 4, 0.37, np.float32)[0]
    assert np.array_equal(g32, g32.astype(np.float32).astype(np.float64)) and not np.array_equal(g32, gx)
