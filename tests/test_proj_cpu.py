"""CPU: the model of pgmg_project (tests/proj_model.py) and what the projection is worth.

On the unit square, element (j, i) at x = i h, y = j h: psi = sin(p pi x) sin(q pi y), whose exact
frame is phi's frame; the divergence-free field w = (s_y, -s_x) of the stream function
s = sin(1.3 pi x + 0.2) cos(0.7 pi y); (u*, v*) = w + grad psi.  Projected as tests/test_grad_cpu.py
solves (nu = 2, omega = 0.5, eps < 0, atol = 1e-10 ||f||, at most 40 cycles).  The error is
sqrt(sum (u - w_x)^2 + (v - w_y)^2) / sqrt(sum w_x^2 + w_y^2) over all N^2 points.  Measured with
the models (fp64; test_projection_table prints the table with -s):

    p, q       N     order 2     ratio    order 4     ratio
    1, 1       33    2.137e-3             8.972e-6
    1, 1       65    5.217e-4    4.10     4.891e-7    18.34
    1, 1       129   1.286e-4    4.06     2.773e-8    17.64
    1, 1       257   3.193e-5    4.03     1.630e-9    17.01
    0.5, 1.5   33    4.795e-3             3.715e-5
    0.5, 1.5   65    1.182e-3    4.06     2.041e-6    18.20
    0.5, 1.5   129   2.933e-4    4.03     1.178e-7    17.32
    0.5, 1.5   257   7.307e-5    4.01     7.055e-9    16.70
"""
import functools

import numpy as np
import pytest

import proj_model
from conftest import bits

PQ = [(1.0, 1.0), (0.5, 1.5)]
SIZES = [33, 65, 129, 257]
RULE = dict(max_cycles=40, rtol=0.0)

# the issue's table: (p, q, N) -> (order 2, order 4), four digits each
TABLE = {
    (1.0, 1.0, 33): (2.137e-3, 8.972e-6),
    (1.0, 1.0, 65): (5.217e-4, 4.891e-7),
    (1.0, 1.0, 129): (1.286e-4, 2.773e-8),
    (1.0, 1.0, 257): (3.193e-5, 1.630e-9),
    (0.5, 1.5, 33): (4.795e-3, 3.715e-5),
    (0.5, 1.5, 65): (1.182e-3, 2.041e-6),
    (0.5, 1.5, 129): (2.933e-4, 1.178e-7),
    (0.5, 1.5, 257): (7.307e-5, 7.055e-9),
}


fields = proj_model.table_fields


def field_error(u, v, wx, wy):
    return float(np.sqrt(np.sum((u - wx) ** 2 + (v - wy) ** 2)) / np.sqrt(np.sum(wx ** 2 + wy ** 2)))


@functools.lru_cache(maxsize=None)
def _row(p, q, N):
    """(order-2 error, order-4 error) of the projection"""
    us, vs, wx, wy, phi0 = fields(p, q, N)
    out = []
    for order in (2, 4):
        f = proj_model.divergence(us, vs, 1.0 / (N - 1), order, -1.0)
        atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
        r = proj_model.project(N, us, vs, phi0, order, 2, 0.5, eps=-1.0, atol=atol, **RULE)
        assert r.fine.reason == 1 and (r.coarse is None or r.coarse.reason == 1), (p, q, N, order)
        assert r.div_after < r.div_before
        out.append(field_error(r.u, r.v, wx, wy))
    return tuple(out)


@pytest.mark.parametrize("p,q", PQ)
def test_projection_table(oracle_mod, p, q):
    """The issue's table to 1e-3 relative; every order-4 ratio per doubling is at least 14, every
    order-2 ratio between 3.5 and 5 (tests/test_grad_cpu.py's bounds), and at N = 257 the order-4
    error is at most 1/1000 of the order-2 error."""
    rows = [_row(p, q, N) for N in SIZES]
    for N, r in zip(SIZES, rows):
        print(f"p={p} q={q} N={N}: order 2 {r[0]:.3e} order 4 {r[1]:.3e}")
        for got, want in zip(r, TABLE[p, q, N]):
            assert abs(got - want) <= 1e-3 * want, (p, q, N, r, TABLE[p, q, N])
    for (Na, a), (Nb, b) in zip(zip(SIZES, rows), zip(SIZES[1:], rows[1:])):
        print(f"p={p} q={q} {Na} -> {Nb}: order 2 x{a[0] / b[0]:.2f}, order 4 x{a[1] / b[1]:.2f}")
        assert a[1] / b[1] >= 14.0, (p, q, Na, Nb, a[1], b[1])
        assert 3.5 <= a[0] / b[0] <= 5.0, (p, q, Na, Nb, a[0], b[0])
    last = rows[SIZES.index(257)]
    assert last[1] <= last[0] / 1000.0, (p, q, last)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("N", [5, 9, 33])
def test_divergence_exact_on_polynomials(order, N):
    """Order 2 reproduces the divergence of (x^2 y, x y^2), order 4 that of a quartic field, on a
    non-dyadic h, within 1e-12 relative, the frame included."""
    h = 0.7 / (N - 1)
    y, x = np.meshgrid(np.arange(N) * h, np.arange(N) * h, indexing="ij")
    if order == 2:
        u, v, want = x ** 2 * y, x * y ** 2, 4 * x * y
    else:
        u, v = x ** 4 + x ** 3 * y, y ** 4 + x ** 2 * y ** 2
        want = 4 * x ** 3 + 3 * x ** 2 * y + 4 * y ** 3 + 2 * x ** 2 * y
    d = proj_model.divergence(u, v, h, order, 1.0)
    assert np.max(np.abs(d - want)) <= 1e-12 * np.max(np.abs(want)), (order, N)


def _specials(seed):
    a = np.random.default_rng(seed).standard_normal((17, 17))
    a[2:10, 3:11] = 0.0       # differences of exactly zero: +0 and -0
    a[13, 13], a[12, 2], a[0, 7] = np.inf, np.nan, -np.inf
    return a


@pytest.mark.parametrize("order", [2, 4])
def test_scale_minus_one_flips_the_sign_bit(order):
    """... of every non-NaN word of the divergence.  The one exception is arithmetic's: where dx
    and dy are zeros of opposite sign their sum is +0 at either scale, so those words are +0 in
    both results (the terms themselves flip: tests/test_grad_cpu.py)."""
    u, v = _specials(order), _specials(order + 10)
    a = proj_model.divergence(u, v, 0.7 / 16, order, 1.0)
    b = proj_model.divergence(u, v, 0.7 / 16, order, -1.0)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    # the terms flip exactly (grad_model's test); a sum of two zeros of opposite sign does not
    gx1, gy1 = proj_model.grad_model.gradient(u, 0.7 / 16, order, 1.0)[0], \
        proj_model.grad_model.gradient(v, 0.7 / 16, order, 1.0)[1]
    mixed = ok & (gx1 == 0) & (gy1 == 0) & (np.signbit(gx1) != np.signbit(gy1))
    flip = ok & ~mixed
    assert flip.sum() > 200 and np.count_nonzero(a[flip] == 0) >= 4
    assert np.array_equal(bits(a)[flip] ^ np.uint64(1 << 63), bits(b)[flip])
    assert np.all(bits(a)[mixed] == 0) and np.all(bits(b)[mixed] == 0)
    # the update: u + scale * gx flips nothing as a whole, but what is added does
    phi = _specials(3)
    for s in (1.0, -1.0):
        un, vn = proj_model.gradient_add(phi, 0.7 / 16, u, v, order, s)
        gx, gy = proj_model.grad_model.gradient(phi, 0.7 / 16, order, s)
        with np.errstate(all="ignore"):
            wu, wv = u + gx, v + gy
        assert np.array_equal(bits(un)[~np.isnan(wu)], bits(wu)[~np.isnan(wu)])
        assert np.array_equal(bits(vn)[~np.isnan(wv)], bits(wv)[~np.isnan(wv)])


def test_model_leaves_its_inputs_alone(oracle_mod):
    rng = np.random.default_rng(7)
    N = 9
    u, v, phi = (rng.standard_normal((N, N)) for _ in range(3))
    keep = [a.copy() for a in (u, v, phi)]
    proj_model.divergence(u, v, 0.125, 4, 0.37)
    proj_model.gradient_add(phi, 0.125, u, v, 2, -1.0)
    assert proj_model.gradient_add(phi, 0.125, u, None)[1] is None
    for order in (2, 4):
        r = proj_model.project(N, u, v, phi, order, 2, 0.5, eps=-1.0, atol=1e-9, **RULE)
        frame = np.concatenate([r.phi[0], r.phi[-1], r.phi[:, 0], r.phi[:, -1]])
        want = np.concatenate([phi[0], phi[-1], phi[:, 0], phi[:, -1]])
        assert np.array_equal(bits(frame), bits(want))
        assert r.div_before == proj_model.norm(r.f) and np.isfinite(r.div_after)
    for a, k in zip((u, v, phi), keep):
        assert np.array_equal(bits(a), bits(k))
