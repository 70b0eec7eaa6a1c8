"""CPU: the model of the Runge-Kutta buoyancy-driven flow (tests/bouss_rk_model.py; include/pgmg.h
"Runge-Kutta buoyancy-driven flow") against what the scheme must do, with no GPU: (a) order 1 is
the Euler model bit for bit; (b) a stage value, the constants and the frame rule by hand; (c) the
temporal orders 1, 2 and 3 of psi and of T on the coupled system; (d) a stably stratified box, whose
internal gravity waves explicit Euler amplifies whatever the diffusion, stays bounded at orders 2
and 3; (e) the multigrid solves in place of the direct one.

The flow is test_vort_rk_cpu.py's three-mode psi0 under free slip, N = 17, with that file's dense
sine-transform solver.  (c) and (e): T0 = (1 - x) + 0.2 sin(pi x) cos(pi y), buoy = (0, 20), nu =
0.01, kappa = 0.02, adiabatic bottom and top.  (d): T0 = y, psi0 scaled by 0.01, buoy = (0, 400), nu
= kappa = 1e-4, adiabatic left and right walls.
"""
import functools

import numpy as np
import pytest

import bouss_model
import bouss_rk_model
import vort_rk_model
from bouss_model import BOTTOM, LEFT, RIGHT, TOP
from conftest import bits
from test_vort_cpu import RULE, _atol, _direct, _grid, _minus_lap
from test_vort_rk_cpu import _flow

N = 17


@functools.lru_cache(maxsize=None)
def _heated():
    """(c), (e): the fields, the parameters of boussinesq_step_rk"""
    psi0, w0 = _flow()
    x, y = _grid(N)
    T0 = (1.0 - x) + 0.2 * np.sin(np.pi * x) * np.cos(np.pi * y)
    T0[:, 0], T0[:, -1] = 1.0, 0.0
    T0.setflags(write=False)
    return psi0, w0, T0, dict(nu=0.01, kappa=0.02, buoy=(0.0, 20.0), free=True, adiabatic=BOTTOM | TOP)


@functools.lru_cache(maxsize=None)
def _stratified():
    """(d): the fields, the parameters"""
    psi0, _ = _flow()
    psi0 = 0.01 * psi0
    w0 = _minus_lap(psi0, 1.0 / (N - 1))
    x, y = _grid(N)
    T0 = y + 0.0 * x
    for a in (psi0, w0, T0):
        a.setflags(write=False)
    return psi0, w0, T0, dict(nu=1e-4, kappa=1e-4, buoy=(0.0, 400.0), free=True, adiabatic=LEFT | RIGHT)


@functools.lru_cache(maxsize=None)
def _run(order, n, t_end):
    psi0, w0, T0, kw = _heated()
    return bouss_rk_model.boussinesq_step_rk(N, psi0, w0, T0, t_end / n, order=order, nsteps=n,
                                             solve=_direct(N), **kw)


def test_order_1_is_the_euler_model():
    """(a) Order 1 of the model against bouss_model.boussinesq_step, bitwise: the heated cavity with
    no-slip walls from rest with the multigrid solves, and the free-slip flow with the direct one."""
    Nc = 17
    rng = np.random.default_rng(7)
    psi0, w0 = np.zeros((Nc, Nc)), np.zeros((Nc, Nc))
    psi0[0, 3] = -0.0
    x, _ = _grid(Nc)
    T0 = (1.0 - x) + np.zeros((Nc, 1))
    T0[1:-1, 1:-1] += 0.01 * rng.standard_normal((Nc - 2, Nc - 2))
    kw = dict(buoy=(0.0, 710.0), nsteps=3, omega=0.5, eps=-1.0, atol=1e-8, **RULE)
    h = 1.0 / (Nc - 1)
    a = bouss_model.boussinesq_step(Nc, psi0, w0, T0, h * h / 8.0, 0.71, 1.0, **kw)
    b = bouss_rk_model.boussinesq_step_rk(Nc, psi0, w0, T0, h * h / 8.0, 0.71, 1.0, order=1, **kw)
    for name in ("phi", "f", "T"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert (a.cycles, a.sweeps) == (b.cycles, b.sweeps) and a.cycles >= 3
    assert (a.cfl, a.diffusion, a.diffusion_t) == (b.cfl, b.diffusion, b.diffusion_t) and a.cfl > 0.0
    assert np.array_equal(bits(a.last.phi), bits(b.last.phi))
    psi0, w0, T0, kw = _heated()
    a = bouss_model.boussinesq_step(N, psi0, w0, T0, 1.0 / 128, nsteps=4, solve=_direct(N), **kw)
    b = _run(1, 4, 4.0 / 128)
    for name in ("phi", "f", "T"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert a.cfl == b.cfl


def test_stage_by_hand():
    """(b) One interior point of stage() against the expression of the header; B3 and K3 by their
    words; the frames are W's and T's, a -0.0 and a subnormal included, and the frames of W0 and T0
    have no part in it; vmax is the Euler pass's; (0, 1) is the Euler step as numbers; W0 = W and
    T0 = T are allowed."""
    assert bits(np.array([bouss_rk_model.K3, bouss_rk_model.B3])).tolist() == [0x3FD5555555555555,
                                                                                0x3FE5555555555555]
    assert bouss_rk_model.STAGES == {1: (), 2: ((0.5, 0.5),),
                                     3: ((0.75, 0.25), (bouss_rk_model.K3, bouss_rk_model.B3))}
    assert bouss_rk_model.STAGES is vort_rk_model.STAGES
    rng = np.random.default_rng(41)
    M, h, dt, nu, kappa, bx, by = 5, -0.3, 0.01, 0.2, 0.35, -3.5, 2.25
    P, W, T, W0, T0 = (rng.standard_normal((M, M)) for _ in range(5))
    W[0, 2], W[3, 0], W[4, 4] = -0.0, 5e-324, -0.0
    T[4, 1], T[2, 4], T[0, 0] = -0.0, -1e-310, -0.0
    for Z in (W0, T0):
        Z[0, :] = Z[-1, :] = np.nan
        Z[:, 0] = Z[:, -1] = np.nan
    ew, et, emax = bouss_model.step(P, W, T, h, dt, nu, kappa, (bx, by))
    keep = np.ones((M, M), dtype=bool)
    keep[1:-1, 1:-1] = False
    for a, b in ((bouss_rk_model.K3, bouss_rk_model.B3), (0.75, 0.25), (0.5, 0.5)):
        Wout, Tout, vmax = bouss_rk_model.stage(P, W, T, W0, T0, h, dt, nu, kappa, (bx, by), a, b)
        w, ih = 0.5 / h, 1.0 / (h * h)
        for y, x in ((2, 3), (1, 1), (3, 2)):
            px, py = (P[y][x + 1] - P[y][x - 1]) * w, (P[y + 1][x] - P[y - 1][x]) * w
            wx, wy = (W[y][x + 1] - W[y][x - 1]) * w, (W[y + 1][x] - W[y - 1][x]) * w
            tx, ty = (T[y][x + 1] - T[y][x - 1]) * w, (T[y + 1][x] - T[y - 1][x]) * w
            advw, advt = py * wx - px * wy, py * tx - px * ty
            lapw = (W[y][x - 1] + W[y][x + 1] + W[y - 1][x] + W[y + 1][x] - 4.0 * W[y][x]) * ih
            lapt = (T[y][x - 1] + T[y][x + 1] + T[y - 1][x] + T[y + 1][x] - 4.0 * T[y][x]) * ih
            src = by * tx - bx * ty
            evw = W[y][x] + dt * ((nu * lapw - advw) + src)
            evt = T[y][x] + dt * (kappa * lapt - advt)
            assert evw == ew[y, x] and evt == et[y, x]
            assert Wout[y, x] == a * W0[y][x] + b * evw
            assert Tout[y, x] == a * T0[y][x] + b * evt
        assert np.array_equal(bits(Wout)[keep], bits(W)[keep])
        assert np.array_equal(bits(Tout)[keep], bits(T)[keep])
        assert np.isfinite(Wout).all() and np.isfinite(Tout).all() and vmax == emax
    # (0, 1): the Euler step's numbers (0 * W0 + 1 * e; only the sign of a zero can differ)
    W0f, T0f = np.where(np.isnan(W0), 0.0, W0), np.where(np.isnan(T0), 0.0, T0)
    Wout, Tout, _ = bouss_rk_model.stage(P, W, T, W0f, T0f, h, dt, nu, kappa, (bx, by), 0.0, 1.0)
    assert np.array_equal(Wout, ew) and np.array_equal(Tout, et)
    # W0 may be W and T0 may be T
    Wout, Tout, _ = bouss_rk_model.stage(P, W, T, W, T, h, dt, nu, kappa, (bx, by), 0.5, 0.5)
    assert Wout[2, 3] == 0.5 * W[2][3] + 0.5 * ew[2, 3]
    assert Tout[2, 3] == 0.5 * T[2][3] + 0.5 * et[2, 3]


# (c): the error ratios per halving of dt the test allows, by order: +-10 % around 2, 4 and 8
# (measured here: psi 2.61, 2.13; 3.97, 4.00; 8.24, 8.24 and T 2.67, 2.09; 4.02, 4.05; 8.09, 8.00).
# At order 1 only the second ratio is held: n = 32 is not yet asymptotic for Euler
RATIO = {1: (1.8, 2.2), 2: (3.6, 4.4), 3: (7.2, 8.8)}


@pytest.mark.parametrize("order", [1, 2, 3])
def test_temporal_order(order):
    """(c) T_end = 0.25 (psi moves by 48 % of its amplitude, T by 0.76), direct solves: the max-norm
    errors of psi and of T against an order-3 run of 1024 steps at n = 32, 64, 128 steps fall by
    2^order per halving of dt."""
    psi0, _, T0, _ = _heated()
    ref = _run(3, 1024, 0.25)
    runs = [_run(order, n, 0.25) for n in (32, 64, 128)]
    moved = float(np.max(np.abs(ref.phi - psi0)) / np.max(np.abs(psi0)))
    moved_t = float(np.max(np.abs(ref.T - T0)))
    for name, field in (("psi", "phi"), ("T", "T")):
        err = [float(np.max(np.abs(getattr(m, field) - getattr(ref, field)))) for m in runs]
        ratios = [err[0] / err[1], err[1] / err[2]]
        print(f"order {order} {name}: errors {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}, ratios "
              f"{ratios[0]:.3f} {ratios[1]:.3f}; cfl at n = 32: {runs[0].cfl:.3f}; psi moved "
              f"{moved:.3f}, T moved {moved_t:.3f}")
        lo, hi = RATIO[order]
        held = ratios[1:] if order == 1 else ratios
        assert all(lo <= r <= hi for r in held), (order, name, ratios)
    assert moved > 0.4


def test_stratified_box_is_bounded_at_orders_2_and_3_only():
    """(d) T0 = y (stable), buoy = (0, 400), nu = kappa = 1e-4, dt = 1/128, 1024 steps: the
    buoyancy oscillation (frequency at most 20, s = 0.16 per step) is amplified by Euler until it
    leaves the finite numbers; orders 2 and 3 end finite with max |psi| over the run at most 1.05
    times the initial one (measured: 0.994 for both; at the end 0.876 and 0.715 of it) and the final
    T within [-0.05, 1.05]."""
    psi0, w0, T0, kw = _stratified()
    start = float(np.max(np.abs(psi0)))
    solve = _direct(N)
    for order in (1, 2, 3):
        P, W, T = psi0, w0, T0
        top = 0.0
        with np.errstate(all="ignore"):
            for _ in range(1024):   # (calls of one step: nsteps = n gives the bits of n such calls)
                m = bouss_rk_model.boussinesq_step_rk(N, P, W, T, 1.0 / 128, order=order, nsteps=1,
                                                      solve=solve, **kw)
                P, W, T = m.phi, m.f, m.T
                if not np.isfinite(P).all():
                    top = np.inf
                    break
                top = max(top, float(np.max(np.abs(P))))
        end = float(np.max(np.abs(P))) / start if np.isfinite(P).all() else np.inf
        print(f"order {order}: max |psi| over the run {top / start!r}, at the end {end!r}; T in "
              f"[{np.min(T)!r}, {np.max(T)!r}]")
        if order == 1:
            assert not (np.isfinite(P).all() and np.isfinite(T).all())
            continue
        assert np.isfinite(P).all() and np.isfinite(W).all() and np.isfinite(T).all()
        assert top <= 1.05 * start, (order, top / start)
        assert -0.05 <= float(np.min(T)) and float(np.max(T)) <= 1.05


# (e): max |psi_multigrid - psi_direct| after the 8 steps, measured with this file; the test allows
# ten times as much
MEASURED_MG_VS_DIRECT = 8.6e-13


def test_multigrid_solves_follow_the_direct_ones():
    """(e) Order 3, the set-up of (c) at dt = 1/128, 8 steps, eps < 0, every stage's solve to atol =
    1e-11 ||w0||: psi differs from the run with direct solves by what the solves leave (measured:
    MEASURED_MG_VS_DIRECT), far below the time discretisation error of that run."""
    psi0, w0, T0, kw = _heated()
    di = _run(3, 8, 8.0 / 128)
    mg = bouss_rk_model.boussinesq_step_rk(N, psi0, w0, T0, 1.0 / 128, order=3, nsteps=8, eps=-1.0,
                                           atol=_atol(w0), **RULE, **kw)
    d = float(np.max(np.abs(mg.phi - di.phi)))
    dt_ = float(np.max(np.abs(mg.T - di.T)))
    fine = _run(3, 64, 8.0 / 128)
    disc = float(np.max(np.abs(di.phi - fine.phi)))
    print(f"multigrid vs direct: psi {d:.3e}, T {dt_:.3e}; time discretisation error of the run "
          f"{disc:.3e}; {mg.cycles} cycles in 24 solves, last reason {mg.last.reason}")
    assert mg.cycles >= 24 and mg.last.reason == 1
    assert d <= 10.0 * MEASURED_MG_VS_DIRECT, (d, MEASURED_MG_VS_DIRECT)
    assert 10.0 * MEASURED_MG_VS_DIRECT < disc, (MEASURED_MG_VS_DIRECT, disc)
    assert mg.cfl == di.cfl or abs(mg.cfl - di.cfl) < 1e-9 * di.cfl
