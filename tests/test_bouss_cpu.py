"""CPU: the model of the buoyancy-driven flow (tests/bouss_model.py; include/pgmg.h "Buoyancy-driven
flow") against what the scheme must do, with no GPU: (a) the step and the scalar wall pass by hand
at N = 5; (b) the step of T is vort_model's step bit for bit, and with zero buoyancy so is the step
of w; (c) pure conduction between two isothermal walls is a fixed point; (d) de Vahl Davis's
differentially heated cavity at Ra = 10^3 (Int. J. Numer. Meth. Fluids 3, 1983) converges at second
order to the published values; (e) the multigrid model follows the direct one.

The direct solver is the dense sine transform of tests/test_vort_cpu.py, restated: for a zero
frame, psi = S (S w S / (l_i + l_j)) S (2 / (N - 1))^2 on the interior, S[k][j] = sin(pi k j /
(N - 1)) and l_k = 2 (1 - cos(k pi h)) / h^2.
"""
import functools

import numpy as np
import pytest

import bouss_model
import vort_model
from conftest import assert_bitwise, bits

PR, RA = 0.71, 1.0e3
NU, KAPPA, BUOY = PR, 1.0, (0.0, RA * PR)
PUBLISHED = dict(psi_mid=1.174, umax=3.649, vmax=3.697, nu_mid=1.118)


def _direct(N):
    """(W, P) -> psi: the exact solve of -lap_h(psi) = W with a zero frame"""
    h = 1.0 / (N - 1)
    k = np.arange(1, N - 1)
    S = np.sin(np.pi * np.outer(k, k) / (N - 1))
    lam = 2.0 * (1.0 - np.cos(k * np.pi * h)) / (h * h)
    den = lam[:, None] + lam[None, :]
    scale = (2.0 / (N - 1)) ** 2

    def solve(W, P):
        out = np.zeros((N, N))
        out[1:-1, 1:-1] = S @ ((S @ W[1:-1, 1:-1] @ S) / den) @ S * scale
        return out

    return solve


def _conduction(N):
    """T = 1 - x: 1 on x = 0, 0 on x = 1"""
    x = np.arange(N) / (N - 1)
    T = np.repeat((1.0 - x)[None, :], N, axis=0)
    T[:, 0], T[:, -1] = 1.0, 0.0
    return T


def test_step_by_hand():
    """(a) One interior point of step() against the expressions of the header, written out, and the
    frames of both outputs."""
    rng = np.random.default_rng(31)
    N, h, dt, nu, kappa, bx, by = 5, -0.3, 0.01, 0.2, 0.35, -3.5, 2.25
    P, W, T = (rng.standard_normal((N, N)) for _ in range(3))
    W[0, 2], W[3, 0], T[4, 1], T[2, 4] = -0.0, 5e-324, -0.0, -1e-310
    Wout, Tout, vmax = bouss_model.step(P, W, T, h, dt, nu, kappa, (bx, by))
    w, ih = 0.5 / h, 1.0 / (h * h)
    for y, x in ((2, 3), (1, 1), (3, 2)):
        px, py = (P[y][x + 1] - P[y][x - 1]) * w, (P[y + 1][x] - P[y - 1][x]) * w
        wx, wy = (W[y][x + 1] - W[y][x - 1]) * w, (W[y + 1][x] - W[y - 1][x]) * w
        tx, ty = (T[y][x + 1] - T[y][x - 1]) * w, (T[y + 1][x] - T[y - 1][x]) * w
        advw, advt = py * wx - px * wy, py * tx - px * ty
        lapw = (W[y][x - 1] + W[y][x + 1] + W[y - 1][x] + W[y + 1][x] - 4.0 * W[y][x]) * ih
        lapt = (T[y][x - 1] + T[y][x + 1] + T[y - 1][x] + T[y + 1][x] - 4.0 * T[y][x]) * ih
        src = by * tx - bx * ty
        assert Wout[y, x] == W[y][x] + dt * ((nu * lapw - advw) + src)
        assert Tout[y, x] == T[y][x] + dt * (kappa * lapt - advt)
    keep = np.ones((N, N), dtype=bool)
    keep[1:-1, 1:-1] = False
    assert np.array_equal(bits(Wout)[keep], bits(W)[keep])
    assert np.array_equal(bits(Tout)[keep], bits(T)[keep])
    assert vmax == vort_model.step(P, W, h, dt, nu)[1]
    # one value with round numbers: P = 0, so Tout = T + dt kappa lapt, and Wout = W + dt src
    Z = np.zeros((N, N))
    Tq = np.arange(25, dtype=np.float64).reshape(N, N) ** 2      # T[j][i] = (5 j + i)^2
    Wout, Tout, vmax = bouss_model.step(Z, Z, Tq, 0.5, 0.125, 1.0, 2.0, (1.0, 3.0))
    # at (2, 2): T = 144, neighbours 121, 169, 49, 289: lapt = (628 - 576) * 4 = 208
    assert Tout[2, 2] == 144.0 + 0.125 * (2.0 * 208.0)
    # tx = (169 - 121) * 1 = 48, ty = (289 - 49) * 1 = 240: src = 3 * 48 - 1 * 240 = -96
    assert Wout[2, 2] == 0.125 * -96.0 and vmax == 0.0


def test_wall_scalar_by_hand():
    """(a) Every wall against the formula written out, mask 0, the corners, the clear walls."""
    N = 5
    T = np.arange(25, dtype=np.float64).reshape(N, N) ** 2 / 8.0   # T[j][i] = (5 j + i)^2 / 8
    T[0, 0] = -0.0
    k3 = bouss_model.K3
    assert k3 == 1.0 / 3.0 and bits(np.array([k3]))[0] == 0x3FD5555555555555
    assert_bitwise(bouss_model.wall_scalar(T, 0), T, "mask 0")
    for mask in range(16):
        got = bouss_model.wall_scalar(T, mask)
        assert_bitwise(got[1:-1, 1:-1], T[1:-1, 1:-1], "the interior")
        for j, i in ((0, 0), (0, 4), (4, 0), (4, 4)):
            assert bits(got)[j, i] == bits(T)[j, i], "a corner was written"
        for x in (1, 2, 3):
            b = T[1][x] + (T[1][x] - T[2][x]) * k3
            t = T[3][x] + (T[3][x] - T[2][x]) * k3
            assert got[0, x] == (b if mask & 1 else T[0][x])
            assert got[4, x] == (t if mask & 2 else T[4][x])
        for y in (1, 2, 3):
            l = T[y][1] + (T[y][1] - T[y][2]) * k3
            r = T[y][3] + (T[y][3] - T[y][2]) * k3
            assert got[y, 0] == (l if mask & 4 else T[y][0])
            assert got[y, 4] == (r if mask & 8 else T[y][4])
    # one value written out: T[1][1] = 36/8, T[2][1] = 121/8: 4.5 + (4.5 - 15.125) * K3
    assert bouss_model.wall_scalar(T, 1)[0, 1] == 4.5 + -10.625 * k3
    # a constant field is kept exactly, and the formula is dT/dn = 0 to second order: a parabola
    # with its vertex on the wall is reproduced to rounding
    C = np.full((N, N), 0.1)
    assert_bitwise(bouss_model.wall_scalar(C, 15), C, "a constant field")
    y = np.arange(N)[:, None] * 0.25
    Q = np.repeat(2.0 + 3.0 * y * y, N, axis=1)
    assert abs(bouss_model.wall_scalar(Q, 1)[0, 2] - 2.0) < 1e-15
    assert T[0, 0] == 0.0 and np.signbit(T[0, 0]), "T is only read"


@pytest.mark.parametrize("N", [9, 33])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_outputs_against_the_vorticity_model(N, sign):
    """(b) On random fields Tout is bitwise vort_model.step(P, T, h, dt, kappa), whatever the
    buoyancy; with buoy = (0, 0), Wout is np.array_equal to vort_model.step(P, W, h, dt, nu)."""
    rng = np.random.default_rng(100 + N)
    P, W, T = (rng.standard_normal((N, N)) for _ in range(3))
    h, dt, nu, kappa = sign * 1.3 / (N - 1), 1e-3, 0.02, 0.7
    for buoy in ((0.0, 0.0), (0.0, 710.0), (-3.5, 2.25)):
        Wout, Tout, vmax = bouss_model.step(P, W, T, h, dt, nu, kappa, buoy)
        want_t, want_vmax = vort_model.step(P, T, h, dt, kappa)
        assert_bitwise(Tout, want_t, f"Tout N={N} h={h} buoy={buoy}")
        assert vmax == want_vmax
        want_w = vort_model.step(P, W, h, dt, nu)[0]
        if buoy == (0.0, 0.0):
            assert np.array_equal(Wout, want_w)
        else:
            assert not np.array_equal(Wout[1:-1, 1:-1], want_w[1:-1, 1:-1]), "the source is live"


# (c): max |T - (1 - x)| after the 100 steps, measured with this file: exactly 0.0 (at N = 17 the
# values k / 16 and every operation of the step and the wall pass on them are exact); the test
# allows ten times it
MEASURED_CONDUCTION_DRIFT = 0.0


def test_conduction_is_a_fixed_point():
    """(c) psi = 0, w = 0, buoy = (0, 0), T = 1 - x between T = 1 on x = 0 and T = 0 on x = 1, top
    and bottom adiabatic, N = 17, 100 steps, direct solve.  T stays at 1 - x up to the rounding the
    Laplacian of a linear field leaves, the flow stays at rest.  Measured: see
    MEASURED_CONDUCTION_DRIFT; ten times it is allowed, and that stays below 1e-12."""
    N = 17
    h = 1.0 / (N - 1)
    T0 = _conduction(N)
    Z = np.zeros((N, N))
    m = bouss_model.boussinesq_step(N, Z, Z, T0, h * h / 8.0, NU, KAPPA, (0.0, 0.0), nsteps=100,
                                    solve=_direct(N))
    drift = float(np.max(np.abs(m.T - T0)))
    print(f"conduction: max |T - (1 - x)| = {drift:.3e}, max |psi| = {np.max(np.abs(m.phi)):.3e}")
    tol = 10.0 * MEASURED_CONDUCTION_DRIFT
    assert tol < 1e-12
    assert drift <= tol, (drift, tol)
    assert not m.phi.any() and not m.f.any(), "the flow stays at rest"


@functools.lru_cache(maxsize=None)
def _cavity(N):
    """de Vahl Davis, Ra = 10^3: (the final state, max |psi| after nine tenths of the run)"""
    h = 1.0 / (N - 1)
    dt = h * h / 8.0
    nsteps = int(round(0.5 / dt))
    Z = np.zeros((N, N))
    kw = dict(solve=_direct(N))
    a = bouss_model.boussinesq_step(N, Z, Z, _conduction(N), dt, NU, KAPPA, BUOY,
                                    nsteps=nsteps - nsteps // 10, **kw)
    b = bouss_model.boussinesq_step(N, a.phi, a.f, a.T, dt, NU, KAPPA, BUOY, nsteps=nsteps // 10, **kw)
    return b, float(np.max(np.abs(a.phi)))


def _peak(a):
    """the maximum of |a| along a line, from the parabola through the largest sample and its two
    neighbours (the published maxima are those of the profile, not of its samples)"""
    a = np.abs(a)
    k = int(np.argmax(a))
    if k == 0 or k == len(a) - 1:
        return float(a[k])
    d = a[k - 1] - 2.0 * a[k] + a[k + 1]
    return float(a[k] - (a[k + 1] - a[k - 1]) ** 2 / (8.0 * d))


def _quantities(m, N):
    h = 1.0 / (N - 1)
    mid = (N - 1) // 2
    psi, T = m.phi, m.T
    u = np.zeros(N)
    u[1:-1] = (psi[2:, mid] - psi[:-2, mid]) / (2.0 * h)            # u = psi_y on x = 1/2
    v = -(psi[mid, 2:] - psi[mid, :-2]) / (2.0 * h)                 # v = -psi_x on y = 1/2
    tx = (T[:, mid + 1] - T[:, mid - 1]) / (2.0 * h)
    q = u * T[:, mid] - tx                                          # the heat flux through x = 1/2
    nu_mid = h * (q.sum() - 0.5 * (q[0] + q[-1]))                   # the trapezoid rule over y
    return dict(psi_mid=abs(psi[mid, mid]), umax=_peak(u), vmax=_peak(v), nu_mid=float(nu_mid))


# (d): the relative deviations from the published values at N = 33, measured with this file; the
# test allows twice each
MEASURED_DEVIATION = dict(psi_mid=7.946e-3, umax=1.438e-3, vmax=2.007e-3, nu_mid=1.632e-5)
SCHEME_IS_WRONG_ABOVE = dict(psi_mid=0.015, umax=0.005, vmax=0.005, nu_mid=0.005)


def test_de_vahl_davis_cavity():
    """(d) Pr = 0.71, Ra = 10^3: nu = 0.71, kappa = 1, buoy = (0, 710); T = 1 on x = 0, 0 on x = 1,
    top and bottom adiabatic, no-slip walls at rest; from rest and T = 1 - x, dt = h^2 / 8 to
    T_end = 0.5 with the direct solve at N = 17, 33, 65.  |psi| at the centre converges at second
    order (the Richardson ratio in [3.6, 4.4]); at N = 33 the four benchmark quantities lie within
    twice the measured deviation from the published 1.174, 3.649, 3.697, 1.118
    (MEASURED_DEVIATION; more than 1.5 % for psi or 0.5 % for the others would mean the scheme is
    wrong); the last tenth of the run changes max |psi| by less than 1e-4 relative.
    Measured here: |psi_mid| 1.20964, 1.18333, 1.17679, ratio 4.025; at N = 33 |psi_mid| 1.18333
    (0.79 %), max |u| 3.64375 (0.14 %), max |v| 3.68958 (0.20 %), Nu 1.117982 (0.0016 %), the
    maxima from the parabola through the three samples at the peak; the last tenth changes
    max |psi| by 1.0e-6, 1.7e-6 and 1.9e-6 relative at N = 17, 33, 65."""
    q = {N: _quantities(_cavity(N)[0], N) for N in (17, 33, 65)}
    for N in q:
        print(f"N={N}: " + ", ".join(f"{k} {v:.5f}" for k, v in q[N].items()))
    p = [q[N]["psi_mid"] for N in (17, 33, 65)]
    ratio = (p[0] - p[1]) / (p[1] - p[2])
    print(f"Richardson ratio of |psi_mid|: {ratio:.3f}")
    assert 3.6 <= ratio <= 4.4, ratio
    for k, pub in PUBLISHED.items():
        dev = abs(q[33][k] - pub) / pub
        print(f"N=33 {k}: {q[33][k]:.6f} against {pub}: deviation {dev:.4e}")
        assert MEASURED_DEVIATION[k] < SCHEME_IS_WRONG_ABOVE[k], k
        assert dev <= min(2.0 * MEASURED_DEVIATION[k], SCHEME_IS_WRONG_ABOVE[k]), (k, dev)
    for N in (17, 33, 65):
        m, before = _cavity(N)
        change = abs(float(np.max(np.abs(m.phi))) - before) / before
        print(f"N={N}: the last tenth changes max |psi| by {change:.2e} relative")
        assert change < 1e-4, (N, change)
    assert max(_cavity(65)[0].cfl, _cavity(65)[0].diffusion, _cavity(65)[0].diffusion_t) < 1.0


# (e): the max-norm differences (psi, T) between the multigrid and the direct model after the 64
# steps, measured with this file; the test allows ten times each
MEASURED_MG_VS_DIRECT = (7.58e-13, 4.22e-14)


def test_multigrid_model_against_direct():
    """(e) 64 steps of (d) at N = 17: the multigrid model (eps < 0, atol = 1e-11 ||w|| of the final
    state, at most 30 cycles) against the direct one; ten times the measured max-norm differences
    in psi and T are allowed (MEASURED_MG_VS_DIRECT)."""
    N = 17
    h = 1.0 / (N - 1)
    Z = np.zeros((N, N))
    args = (N, Z, Z, _conduction(N), h * h / 8.0, NU, KAPPA, BUOY)
    di = bouss_model.boussinesq_step(*args, nsteps=64, solve=_direct(N))
    atol = 1e-11 * float(np.linalg.norm(di.f[1:-1, 1:-1]))
    mg = bouss_model.boussinesq_step(*args, nsteps=64, eps=-1.0, atol=atol, rtol=0.0, max_cycles=30)
    d_psi = float(np.max(np.abs(mg.phi - di.phi)))
    d_t = float(np.max(np.abs(mg.T - di.T)))
    print(f"multigrid vs direct: psi {d_psi:.3e} (max |psi| {np.max(np.abs(di.phi)):.3e}), T {d_t:.3e}; "
          f"atol {atol:.3e}, {mg.cycles} cycles, last reason {mg.last.reason}")
    assert mg.last.reason == 1 and mg.cycles >= 64
    assert d_psi <= 10.0 * MEASURED_MG_VS_DIRECT[0], d_psi
    assert d_t <= 10.0 * MEASURED_MG_VS_DIRECT[1], d_t
    assert np.max(np.abs(di.phi)) > 1e3 * 10.0 * MEASURED_MG_VS_DIRECT[0], "the flow has started"
