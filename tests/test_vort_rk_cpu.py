"""CPU: the model of the Runge-Kutta vorticity transport (tests/vort_rk_model.py; include/pgmg.h
"Runge-Kutta vorticity transport") against what the scheme must do, with no GPU: (a) order 1 is the
Euler model bit for bit; (b) a stage value, the constants and the frame rule by hand; (c) the
temporal orders 1, 2 and 3; (d) order 3 stays bounded at a cell Reynolds number where orders 1 and 2
blow up; (e) the multigrid solves in place of the direct one.

The flow of (c), (d) and (e) is test_vort_cpu.py's three-mode flow at full amplitude under free
slip: psi0 = s1(x) s1(y) + 0.5 s2(x) s1(y) + 0.3 s1(x) s2(y), w0 its discrete -lap_h, N = 17; the
direct solver is that file's dense sine transform.
"""
import functools

import numpy as np
import pytest

import vort_model
import vort_rk_model
from conftest import bits
from test_vort_cpu import RULE, _atol, _direct, _grid, _minus_lap

N = 17


@functools.lru_cache(maxsize=None)
def _flow(N=N):
    h = 1.0 / (N - 1)
    x, y = _grid(N)
    s = lambda k, t: np.sin(k * np.pi * t)
    psi0 = s(1, x) * s(1, y) + 0.5 * s(2, x) * s(1, y) + 0.3 * s(1, x) * s(2, y)
    psi0[0, :] = psi0[-1, :] = 0.0
    psi0[:, 0] = psi0[:, -1] = 0.0
    w0 = _minus_lap(psi0, h)
    for a in (psi0, w0):
        a.setflags(write=False)
    return psi0, w0


@functools.lru_cache(maxsize=None)
def _run(order, n, T, nu):
    psi0, w0 = _flow()
    return vort_rk_model.vorticity_step_rk(N, psi0, w0, T / n, nu, free=True, order=order, nsteps=n,
                                           solve=_direct(N))


def test_order_1_is_the_euler_model():
    """(a) Order 1 of the model against vort_model.vorticity_step, bitwise: the lid cavity from
    rest with the multigrid solves, and the free-slip flow with the direct one."""
    Nc = 17
    psi0, w0 = np.zeros((Nc, Nc)), np.zeros((Nc, Nc))
    psi0[0, 3] = -0.0
    kw = dict(walls=(0.0, 1.0, 0.0, 0.0), nsteps=3, omega=0.5, eps=-1.0, atol=1e-8, **RULE)
    a = vort_model.vorticity_step(Nc, psi0, w0, 0.01, 0.01, **kw)
    b = vort_rk_model.vorticity_step_rk(Nc, psi0, w0, 0.01, 0.01, order=1, **kw)
    assert np.array_equal(bits(a.phi), bits(b.phi)) and np.array_equal(bits(a.f), bits(b.f))
    assert (a.cycles, a.sweeps) == (b.cycles, b.sweeps) and a.cycles >= 3
    assert (a.cfl, a.diffusion) == (b.cfl, b.diffusion) and a.cfl > 0.0
    assert np.array_equal(bits(a.last.phi), bits(b.last.phi))
    psi0, w0 = _flow()
    a = vort_model.vorticity_step(N, psi0, w0, 1.0 / 128, 0.01, free=True, nsteps=4, solve=_direct(N))
    b = _run(1, 4, 4.0 / 128, 0.01)
    assert np.array_equal(bits(a.phi), bits(b.phi)) and np.array_equal(bits(a.f), bits(b.f))
    assert a.cfl == b.cfl


def test_stage_by_hand():
    """(b) One interior point of stage() against the expression of the header; B3 and K3 by their
    words; the frame is W's, a -0.0 and a subnormal included, and W0's frame has no part in it;
    vmax is the Euler pass's."""
    assert bits(np.array([vort_rk_model.K3, vort_rk_model.B3])).tolist() == [0x3FD5555555555555,
                                                                              0x3FE5555555555555]
    assert vort_rk_model.STAGES == {1: (), 2: ((0.5, 0.5),),
                                    3: ((0.75, 0.25), (vort_rk_model.K3, vort_rk_model.B3))}
    rng = np.random.default_rng(4)
    M, h, dt, nu = 5, -0.3, 0.01, 0.2
    P, W, W0 = (rng.standard_normal((M, M)) for _ in range(3))
    W[0, 2], W[3, 0], W[4, 4] = -0.0, 5e-324, -0.0
    W0[0, :] = W0[-1, :] = np.nan
    W0[:, 0] = W0[:, -1] = np.nan
    e, emax = vort_model.step(P, W, h, dt, nu)
    keep = np.ones((M, M), dtype=bool)
    keep[1:-1, 1:-1] = False
    for a, b in ((vort_rk_model.K3, vort_rk_model.B3), (0.75, 0.25), (0.5, 0.5)):
        out, vmax = vort_rk_model.stage(P, W, W0, h, dt, nu, a, b)
        w, ih = 0.5 / h, 1.0 / (h * h)
        y, x = 2, 3
        px, py = (P[y][x + 1] - P[y][x - 1]) * w, (P[y + 1][x] - P[y - 1][x]) * w
        wx, wy = (W[y][x + 1] - W[y][x - 1]) * w, (W[y + 1][x] - W[y - 1][x]) * w
        adv = py * wx - px * wy
        lap = (W[y][x - 1] + W[y][x + 1] + W[y - 1][x] + W[y + 1][x] - 4.0 * W[y][x]) * ih
        ev = W[y][x] + dt * (nu * lap - adv)
        assert ev == e[y, x]
        assert out[y, x] == a * W0[y][x] + b * ev
        assert np.array_equal(bits(out)[keep], bits(W)[keep])
        assert np.isfinite(out).all() and vmax == emax
    # (0, 1): the Euler step's numbers (0 * W0 + 1 * e; only the sign of a zero can differ)
    W0f = np.where(np.isnan(W0), 0.0, W0)
    out = vort_rk_model.stage(P, W, W0f, h, dt, nu, 0.0, 1.0)[0]
    assert np.array_equal(out, e)
    # W0 may be W itself
    out = vort_rk_model.stage(P, W, W, h, dt, nu, 0.5, 0.5)[0]
    assert out[2, 3] == 0.5 * W[2][3] + 0.5 * e[2, 3]


# (c): the error ratios per halving of dt the test allows, by order: +-10 % around 2, 4 and 8 (the
# margin test_vort_cpu.py gives its second-order ratio; measured here: 2.01, 2.00; 4.08, 4.05;
# 8.17, 8.13)
RATIO = {1: (1.8, 2.2), 2: (3.6, 4.4), 3: (7.2, 8.8)}


@pytest.mark.parametrize("order", [1, 2, 3])
def test_temporal_order(order):
    """(c) nu = 0.01, T = 0.25 (the flow moves by 43 % of its amplitude), direct solves: the
    max-norm error of psi against an order-3 run of 1024 steps at n = 32, 64, 128 steps falls by
    2^order per halving of dt."""
    psi0, _ = _flow()
    ref = _run(3, 1024, 0.25, 0.01).phi
    err = [float(np.max(np.abs(_run(order, n, 0.25, 0.01).phi - ref))) for n in (32, 64, 128)]
    ratios = [err[0] / err[1], err[1] / err[2]]
    moved = float(np.max(np.abs(ref - psi0)) / np.max(np.abs(psi0)))
    print(f"order {order}: errors {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}, ratios {ratios[0]:.3f} "
          f"{ratios[1]:.3f}; cfl at n = 32: {_run(order, 32, 0.25, 0.01).cfl:.3f}; moved {moved:.3f}")
    lo, hi = RATIO[order]
    assert all(lo <= r <= hi for r in ratios), (order, ratios)
    assert moved > 0.4


def _enstrophy(w):
    return float(np.sum(w[1:-1, 1:-1] ** 2))


def test_order_3_is_stable_where_euler_and_heun_are_not():
    """(d) nu = 1e-4, dt = 1/128, 1024 steps (T = 8; cfl about 0.8, a cell Reynolds number in the
    thousands): order 3 ends finite with its enstrophy, the sum of w^2 over the interior, within
    10 % of the initial one (measured: 1.011 times it); orders 1 and 2 amplify every advective
    mode and end non-finite."""
    _, w0 = _flow()
    start = _enstrophy(w0)
    with np.errstate(all="ignore"):
        end = {order: _run(order, 1024, 8.0, 1e-4) for order in (1, 2, 3)}
    for order, m in end.items():
        print(f"order {order}: enstrophy ratio {_enstrophy(m.f) / start!r}, cfl {m.cfl!r}, "
              f"diffusion {m.diffusion!r}")
    m = end[3]
    assert np.isfinite(m.phi).all() and np.isfinite(m.f).all()
    assert 0.9 <= _enstrophy(m.f) / start <= 1.1
    assert 0.5 < m.cfl < 1.73
    for order in (1, 2):
        assert not np.isfinite(end[order].phi).all(), order


# (e): max |psi_multigrid - psi_direct| after the 8 steps, measured with this file; the test allows
# ten times as much
MEASURED_MG_VS_DIRECT = 1.4e-12


def test_multigrid_solves_follow_the_direct_ones():
    """(e) Order 3, nu = 0.01, dt = 1/128, 8 steps, eps < 0, every stage's solve to atol = 1e-11
    ||w0||: psi differs from the run with direct solves by what the solves leave (measured:
    MEASURED_MG_VS_DIRECT), far below the time discretisation error of that run."""
    psi0, w0 = _flow()
    di = _run(3, 8, 8.0 / 128, 0.01)
    mg = vort_rk_model.vorticity_step_rk(N, psi0, w0, 1.0 / 128, 0.01, free=True, order=3, nsteps=8,
                                         eps=-1.0, atol=_atol(w0), **RULE)
    d = float(np.max(np.abs(mg.phi - di.phi)))
    fine = _run(3, 64, 8.0 / 128, 0.01)
    disc = float(np.max(np.abs(di.phi - fine.phi)))
    print(f"multigrid vs direct {d:.3e}; time discretisation error of the run {disc:.3e}; "
          f"{mg.cycles} cycles in 24 solves, last reason {mg.last.reason}")
    assert mg.cycles >= 24 and mg.last.reason == 1
    assert d <= 10.0 * MEASURED_MG_VS_DIRECT, (d, MEASURED_MG_VS_DIRECT)
    assert 10.0 * MEASURED_MG_VS_DIRECT < disc, (MEASURED_MG_VS_DIRECT, disc)
    assert mg.cfl == di.cfl or abs(mg.cfl - di.cfl) < 1e-9 * di.cfl
