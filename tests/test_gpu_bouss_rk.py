"""GPU: pgmg_boussinesq_step_rk (include/pgmg.h "Runge-Kutta buoyancy-driven flow") through
Solver.boussinesq_step(order=2 and 3) against its model, tests/bouss_rk_model.boussinesq_step_rk:
phi, f with its frame and T bitwise, the statistics equal, the stop decisions the way
tests/test_gpu_bouss.py compares them.

The flow, the rule and the time steps are that file's: the start of de Vahl Davis's cavity at Ra =
10^3 (no-slip walls at rest, bottom and top adiabatic, T = 1 on x = 0 and T = 0 on x = 1, a
perturbed conduction profile), dt = h^2 / 8, omega = 0.5 for the damped solve, eps < 0, rtol = 0,
atol = 1e-8, at most 30 cycles.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bouss_model
import bouss_rk_model
from conftest import assert_bitwise, bits
from test_gpu_bouss import BUOY, KAPPA, NU, RULE, WALLS, _check_solve, _compare, _dt, _start, _t

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(N, order, nsteps):
    psi0, w0, T0 = _start(N)
    m = bouss_rk_model.boussinesq_step_rk(N, psi0, w0, T0, _dt(N), NU, KAPPA, BUOY, WALLS, False, 3,
                                          order, nsteps, omega=0.5, eps=-1.0, **RULE)
    for a in (m.phi, m.f, m.T):
        a.setflags(write=False)
    return m


def _run(pgmg, N, order, nsteps=2, **kw):
    psi0, w0, T0 = _start(N)
    m = _model(N, order, nsteps)
    what = f"heated cavity N={N} order={order} nsteps={nsteps} {kw}"
    with pgmg.Solver(N, eps=-1.0, **kw) as s:
        s.set_problem(None, None)        # an analytic problem and cycles before: all replaced
        s.vcycle(1)
        s.set_problem(psi0, w0)
        T = _t(T0)
        info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, nsteps=nsteps, order=order, **RULE)
        _compare(s, T, info, m, N, nsteps, what)
        assert m.cycles >= order * nsteps
        # the problem is one with a caller's f
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_ERROR, C.byref(pgmg.PgmgMonitorOut())) == pgmg.PGMG_ERR_STATE
        return s.stats_detail()[2] >= 0   # level 0 is cross-fused


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("N", [33, 65])
def test_cavity_against_the_model(pgmg, N, order):
    _run(pgmg, N, order)


@pytest.mark.parametrize("order", [2, 3])
def test_cross_fused_level_0(pgmg, plan, order):
    """N = 129 with tail_n = 17 and cross_min_n = 9: level 0 is cross-fused, its cycles rotate the
    level-0 grids, and every wall and stage pass reads psi where it lies then."""
    plan(cross_min_n=9)
    assert _run(pgmg, 129, order, tail_n=17)


@pytest.mark.parametrize("order", [2, 3])
def test_free_slip_dirichlet_walls(pgmg, order):
    """PGMG_WALL_FREE and mask 0 on random w and T: the frame w came with is replaced by +0.0, in f
    and so in the saved w too; no wall of T is written."""
    import torch
    N = 33
    rng = np.random.default_rng(13)
    psi0 = np.zeros((N, N))
    w0 = np.zeros((N, N))
    w0[1:-1, 1:-1] = rng.standard_normal((N - 2, N - 2))
    w0[0, :] = 5.0                      # a frame the wall pass replaces
    T0 = rng.standard_normal((N, N))
    m = bouss_rk_model.boussinesq_step_rk(N, psi0, w0, T0, 1e-4, NU, KAPPA, (-3.0, 20.0), WALLS, True, 0,
                                          order, 2, omega=0.5, eps=-1.0, **RULE)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        T = _t(T0)
        info = s.boussinesq_step(T, 1e-4, NU, KAPPA, (-3.0, 20.0), WALLS, free=True, adiabatic=0, nsteps=2,
                                 order=order, **RULE)
        torch.cuda.synchronize()
        assert_bitwise(s.solution(), m.phi, "phi")
        f = s.rhs()
        assert_bitwise(f, m.f, "w")
        assert not bits(np.concatenate([f[0], f[-1], f[:, 0], f[:, -1]])).any()
        got = T.cpu().numpy()
        assert_bitwise(got, m.T, "T")
        keep = np.ones((N, N), dtype=bool)
        keep[1:-1, 1:-1] = False
        assert np.array_equal(bits(got)[keep], bits(T0)[keep])
        assert (info.steps, info.cycles, info.sweeps) == (2, m.cycles, m.sweeps)
        assert bits(np.array([info.cfl, info.diffusion_t])).tolist() == bits(np.array([m.cfl, m.diffusion_t])).tolist()


def _call(pgmg, s, T, omega=0.5, dt=1e-4, nu=NU, kappa=KAPPA, buoy=BUOY, mode=0, walls=WALLS, mask=3,
          order=3, nsteps=1, info=True, opts=True, params=True, out=None, **fields):
    o, p = pgmg.PgmgSolveOpts(), pgmg.PgmgBoussParams()
    out = pgmg.PgmgBoussInfo() if out is None else out
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, val in fields.items():
        setattr(o, k, val)
    p.dt, p.nu, p.kappa, p.mode, p.adiabatic = dt, nu, kappa, mode, mask
    p.buoy = (C.c_double * 2)(*buoy)
    p.walls = (C.c_double * 4)(*walls)
    return s.lib.pgmg_boussinesq_step_rk(s.h, C.byref(o) if opts else None, omega,
                                         C.byref(p) if params else None, T, order, nsteps,
                                         C.byref(out) if info else None)


def test_order_1_is_the_euler_entry(pgmg):
    """pgmg_boussinesq_step_rk(order = 1) against pgmg_boussinesq_step from the same start on two
    contexts: phi, f, T and every field of info but the times, bit for bit; and against the Euler
    model."""
    import torch
    N, nsteps = 65, 3
    psi0, w0, T0 = _start(N)
    res = []
    for rk in (False, True):
        with pgmg.Solver(N, eps=-1.0) as s:
            s.set_problem(psi0, w0)
            T = _t(T0)
            if rk:
                out = pgmg.PgmgBoussInfo()
                assert _call(pgmg, s, C.c_void_p(T.data_ptr()), dt=_dt(N), order=1, nsteps=nsteps, out=out,
                             **RULE) == pgmg.PGMG_OK
                info, dift = out.flow, out.diffusion_t
            else:
                info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, nsteps=nsteps, **RULE)
                dift = info.diffusion_t
            fields = [info.steps, info.cycles, info.sweeps, info.worst_reason, info.worst_res, info.cfl,
                      info.diffusion, dift]
            fields += [getattr(info.last, name) for name, _ in pgmg.PgmgSolveInfo._fields_
                       if not name.endswith("_ms")]
            torch.cuda.synchronize()
            res.append((s.solution(), s.rhs(), T.cpu().numpy(), fields, s.stats()))
    (p0, f0, T_0, i0, s0), (p1, f1, T_1, i1, s1) = res
    assert_bitwise(p1, p0, "phi")
    assert_bitwise(f1, f0, "w")
    assert_bitwise(T_1, T_0, "T")
    assert bits(np.array(i1, dtype=np.float64)).tolist() == bits(np.array(i0, dtype=np.float64)).tolist(), (i0, i1)
    assert s1 == s0 and i0[0] == nsteps and i0[1] >= nsteps
    m = bouss_model.boussinesq_step(N, psi0, w0, T0, _dt(N), NU, KAPPA, BUOY, WALLS, False, 3, nsteps,
                                    omega=0.5, eps=-1.0, **RULE)
    assert_bitwise(p1, m.phi, "phi against the Euler model")
    assert_bitwise(f1, m.f, "w against the Euler model")
    assert_bitwise(T_1, m.T, "T against the Euler model")


def test_three_calls_and_what_follows(pgmg, oracle_mod):
    """nsteps = 3 equals three calls of one step, order 3; a gradient and a vcycle afterwards
    continue from (psi, w)."""
    import torch
    import grad_model
    N, order = 33, 3
    h = 1.0 / (N - 1)
    psi0, w0, T0 = _start(N)
    m = _model(N, order, 3)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        T = _t(T0)
        cycles = 0
        for k in range(3):
            info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, order=order, **RULE)
            assert info.steps == 1
            cycles += info.cycles
            mk = _model(N, order, k + 1)
            torch.cuda.synchronize()
            assert_bitwise(s.solution(), mk.phi, f"phi after call {k + 1}")
            assert_bitwise(s.rhs(), mk.f, f"w after call {k + 1}")
            assert_bitwise(T.cpu().numpy(), mk.T, f"T after call {k + 1}")
        assert cycles == m.cycles
        _check_solve(info.last, m.last, N, "third call")
        gx, gy = s.gradient(order=2, scale=1.0)
        torch.cuda.synchronize()
        wx, wy = grad_model.gradient(m.phi, h, 2, 1.0)
        assert_bitwise(gx.cpu().numpy(), wx, "gx after the call")
        assert_bitwise(gy.cpu().numpy(), wy, "gy after the call")
        s.vcycle(1)
        got = s.solution()
        sweeps = s.stats()[0]
    o = oracle_mod.Oracle(eps=-1.0)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(m.f), h)
    assert_bitwise(got, x, "vcycle(1) after the call")
    assert sweeps == m.last.sweeps + o.sweeps
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        T = _t(T0)
        info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, nsteps=3, order=order, **RULE)
        _compare(s, T, info, m, N, 3, "nsteps = 3")


def test_another_order_on_the_same_context(pgmg):
    """Order 1 (no saved grids yet), then order 3 (their first allocation), then order 2 on one
    context, each from the same start, against the model."""
    import torch
    N = 33
    psi0, w0, T0 = _start(N)
    with pgmg.Solver(N, eps=-1.0) as s:
        for order in (1, 3, 2, 3):
            m = _model(N, order, 2)
            s.set_problem(psi0, w0)
            T = _t(T0)
            info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, nsteps=2, order=order, **RULE)
            torch.cuda.synchronize()
            assert_bitwise(s.solution(), m.phi, f"phi, order {order}")
            assert_bitwise(s.rhs(), m.f, f"w, order {order}")
            assert_bitwise(T.cpu().numpy(), m.T, f"T, order {order}")
            assert (info.steps, info.cycles, info.sweeps) == (2, m.cycles, m.sweeps), order


def test_errors_write_nothing(pgmg):
    import torch
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    nan, inf = float("nan"), float("inf")
    keep = np.random.default_rng(6).standard_normal((N, N))
    Tt = _t(keep)
    T = C.c_void_p(Tt.data_ptr())
    host = np.array(keep)

    def untouched(s, before, what):
        assert_bitwise(s.solution(), before[0], what + ": phi")
        assert_bitwise(s.rhs(), before[1], what + ": f")
        assert s.stats() == before[2], what
        torch.cuda.synchronize()
        assert_bitwise(Tt.cpu().numpy(), keep, what + ": T")

    with pgmg.Solver(N) as s:
        assert _call(pgmg, s, T) == STATE                           # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for bad in (0, 4, -1, 17):
            assert _call(pgmg, s, T, order=bad) == ARG, bad
        assert s.lib.pgmg_boussinesq_step_rk(None, None, 0.5, None, None, 3, 1, None) == ARG
        assert _call(pgmg, s, T, info=False) == ARG and _call(pgmg, s, T, opts=False) == ARG
        assert _call(pgmg, s, T, params=False) == ARG and _call(pgmg, s, None) == ARG
        assert _call(pgmg, s, host.ctypes.data_as(C.c_void_p)) == ARG        # a host T
        assert _call(pgmg, s, T, check_every=0) == ARG
        assert _call(pgmg, s, T, monitor=pgmg.PGMG_MON_RESIDUAL | pgmg.PGMG_MON_ERROR) == ARG
        for bad in (0.0, 1.5, -0.5, nan, inf):
            assert _call(pgmg, s, T, omega=bad) == ARG, bad
        for bad in (0.0, -1e-3, nan, inf):
            assert _call(pgmg, s, T, dt=bad) == ARG, bad
        for bad in (-1e-9, nan, inf):
            assert _call(pgmg, s, T, nu=bad) == ARG and _call(pgmg, s, T, kappa=bad) == ARG, bad
        for k in range(2):
            for bad in (nan, inf, -inf):
                b = list(BUOY)
                b[k] = bad
                assert _call(pgmg, s, T, buoy=b) == ARG, (k, bad)
        for bad in (16, 19, 64, 2 ** 31):
            assert _call(pgmg, s, T, mask=bad) == ARG, bad
        for bad in (-1, 2, 5):
            assert _call(pgmg, s, T, mode=bad) == ARG, bad
        for k in range(4):
            for bad in (nan, inf, -inf):
                ws = list(WALLS)
                ws[k] = bad
                assert _call(pgmg, s, T, walls=ws) == ARG and _call(pgmg, s, T, walls=ws, mode=1) == ARG
        for bad in (0, -3):
            assert _call(pgmg, s, T, nsteps=bad) == ARG, bad
        assert np.array_equal(bits(host), bits(keep))
        untouched(s, before, "refused calls")
        with pytest.raises(pgmg.PgmgError):
            s.boussinesq_step(Tt, 1e-4, NU, KAPPA, order=4)
        with pytest.raises(ValueError):
            s.boussinesq_step(Tt.cpu(), 1e-4, NU, KAPPA, order=3)
        untouched(s, before, "order 4 through the Solver")
        for order in (1, 2, 3):
            assert _call(pgmg, s, T, order=order) == pgmg.PGMG_OK   # (and the arguments were good)
        Tt.copy_(_t(keep))
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        before = (s.solution(), s.rhs(), s.stats())
        assert _call(pgmg, s, T) == STATE
        untouched(s, before, "fp32")
    fkeep = np.random.default_rng(5).standard_normal((N, N))
    with pgmg.Solver(N) as s:             # a device-bound problem: f is the caller's
        g, fd = _t(np.zeros((N, N))), _t(fkeep)
        s.set_problem_device(g, fd)
        assert _call(pgmg, s, T) == STATE
        torch.cuda.synchronize()
        assert_bitwise(fd.cpu().numpy(), fkeep, "the caller's f")
        assert not g.cpu().numpy().any()
        assert_bitwise(Tt.cpu().numpy(), keep, "device-bound: T")


def test_boussinesq_rk_time(pgmg):
    import torch
    N = 257
    keep = np.random.default_rng(8).standard_normal((N, N))
    T = _t(keep)
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for which, per_point in ((0, 88.0), (1, 56.0), (0, 88.0), (2, 88.0), (3, 56.0)):
            ms, b = s.boussinesq_rk_time(which, reps=3)
            assert ms > 0.0 and b == per_point * N * N, (which, ms, b)
        assert_bitwise(s.solution(), before[0], "phi after boussinesq_rk_time")
        assert_bitwise(s.rhs(), before[1], "f after boussinesq_rk_time")
        assert s.stats() == before[2]
        torch.cuda.synchronize()
        assert_bitwise(T.cpu().numpy(), keep, "T after boussinesq_rk_time")
        for bad in (-1, 4):
            assert s.lib.pgmg_boussinesq_rk_time(s.h, bad, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_boussinesq_rk_time(s.h, 0, 0, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert s.lib.pgmg_boussinesq_rk_time(s.h, 0, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_STATE
