"""GPU: pgmg_boussinesq_step (include/pgmg.h "Buoyancy-driven flow") through Solver.boussinesq_step
against its model, tests/bouss_model.boussinesq_step: phi, f and T bitwise, the statistics equal,
the stop decisions the way tests/test_gpu_vorticity.py compares them (the device norms differ from
the model's sequential ones in summation order only: solve_rule.norm_tol).

The flow is the start of de Vahl Davis's cavity at Ra = 10^3, Pr = 0.71: nu = 0.71, kappa = 1, buoy
= (0, 710), no-slip walls at rest, top and bottom adiabatic; psi0 = 0 (with a few -0.0 on its
frame), w0 = 0, T0 = 1 - x between T = 1 on x = 0 and T = 0 on x = 1 plus a seeded random
perturbation of the interior (amplitude 0.05), so every term is live in step 1; dt = h^2 / 8
(diffusion 0.355, diffusion_t 0.5); omega = 0.5 for the damped solve, eps < 0, rtol = 0, atol =
1e-8, at most 30 cycles.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import bouss_model
from conftest import assert_bitwise, bits
from solve_rule import close, norm_tol

pytestmark = pytest.mark.gpu

NU, KAPPA, BUOY, WALLS = 0.71, 1.0, (0.0, 710.0), (0.0, 0.0, 0.0, 0.0)
RULE = dict(max_cycles=30, rtol=0.0, atol=1e-8)


def _dt(N):
    return 1.0 / (8.0 * (N - 1) * (N - 1))


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _start(N):
    psi0, w0 = np.zeros((N, N)), np.zeros((N, N))
    psi0[0, 3], psi0[-1, 0], psi0[2, -1] = -0.0, -0.0, -0.0
    x = np.arange(N) / (N - 1)
    T0 = np.repeat((1.0 - x)[None, :], N, axis=0)
    T0[1:-1, 1:-1] += 0.05 * np.random.default_rng(4200 + N).standard_normal((N - 2, N - 2))
    T0[:, 0], T0[:, -1] = 1.0, 0.0
    for a in (psi0, w0, T0):
        a.setflags(write=False)
    return psi0, w0, T0


@functools.lru_cache(maxsize=None)
def _model(N, nsteps, buoy=BUOY):
    psi0, w0, T0 = _start(N)
    m = bouss_model.boussinesq_step(N, psi0, w0, T0, _dt(N), NU, KAPPA, buoy, WALLS, False, 3, nsteps,
                                    omega=0.5, eps=-1.0, **RULE)
    for a in (m.phi, m.f, m.T):
        a.setflags(write=False)
    return m


def _check_solve(info, m, N, what):
    print(f"{what}: {info.cycles} cycles, reason {info.reason}, res {info.res:.3e} "
          f"(model {m.cycles}, {m.reason}, margin {m.margin:.3e})")
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.checks, info.reason) == (m.cycles, m.checks, m.reason), what
    assert close(info.res0, m.history[0][1], N) and close(info.res, m.history[-1][1], N), what


def _compare(s, T, info, m, N, nsteps, what):
    import torch
    psi0 = _start(N)[0]
    assert info.steps == nsteps, what
    _check_solve(info.last, m.last, N, what)
    assert len(info.history) == len(m.last.history), what
    for (k, r, _), (mk, mr, _) in zip(info.history, m.last.history):
        assert k == mk and close(r, mr, N), (what, k, r, mr)
    got = s.solution()
    assert_bitwise(got, m.phi, what + " phi")
    assert_bitwise(s.rhs(), m.f, what + " w")
    torch.cuda.synchronize()
    assert_bitwise(T.cpu().numpy(), m.T, what + " T")
    frame = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
    want = np.concatenate([psi0[0], psi0[-1], psi0[:, 0], psi0[:, -1]])
    assert np.array_equal(bits(frame), bits(want)), "phi's frame changed"
    # the statistics: the context's start over at every step, the info sums them
    assert s.stats()[0] == m.last.sweeps, (what, s.stats(), m.last.sweeps)
    assert (info.cycles, info.sweeps) == (m.cycles, m.sweeps), (what, info.cycles, m.cycles)
    print(f"{what}: cfl {info.cfl!r} (model {m.cfl!r}), diffusion {info.diffusion!r}, "
          f"diffusion_t {info.diffusion_t!r}")
    assert bits(np.array([info.cfl, info.diffusion, info.diffusion_t])).tolist() == \
        bits(np.array([m.cfl, m.diffusion, m.diffusion_t])).tolist()
    assert m.cfl > 0.0 and m.diffusion <= 1.0 and m.diffusion_t <= 1.0
    assert info.worst_res >= info.last.res > 0.0 and info.worst_reason in (1, 2, 3)
    assert info.step_ms > 0.0 and info.solve_ms > 0.0 and info.elapsed_ms >= info.solve_ms


def _run(pgmg, N, nsteps=3, **kw):
    psi0, w0, T0 = _start(N)
    m = _model(N, nsteps)
    what = f"heated cavity N={N} nsteps={nsteps} {kw}"
    with pgmg.Solver(N, eps=-1.0, **kw) as s:
        s.set_problem(None, None)        # an analytic problem and cycles before: all replaced
        s.vcycle(1)
        s.set_problem(psi0, w0)
        T = _t(T0)
        info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, nsteps=nsteps, **RULE)
        _compare(s, T, info, m, N, nsteps, what)
        # the problem is one with a caller's f
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_ERROR, C.byref(pgmg.PgmgMonitorOut())) == pgmg.PGMG_ERR_STATE
        return s.stats_detail()[2] >= 0   # level 0 is cross-fused


@pytest.mark.parametrize("N", [33, 65])
def test_against_the_model(pgmg, N):
    _run(pgmg, N)


def test_cross_fused_level_0(pgmg, plan):
    """N = 129 with tail_n = 17 and cross_min_n = 9: level 0 is cross-fused, its cycles rotate the
    level-0 grids, and every pass reads psi where it lies then."""
    assert not _run(pgmg, 129, tail_n=17)
    plan(cross_min_n=9)
    assert _run(pgmg, 129, tail_n=17)


def test_three_calls_and_what_follows(pgmg, oracle_mod):
    """nsteps = 3 equals three calls of one step (the closing wall passes of a call are the opening
    ones of the next, bit for bit); Solver.rhs() is w; a vcycle afterwards continues from (psi,
    w); PGMG_MON_ERROR is refused afterwards."""
    import torch
    N = 65
    h = 1.0 / (N - 1)
    psi0, w0, T0 = _start(N)
    m = _model(N, 3)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        T = _t(T0)
        cycles = 0
        for k in range(3):
            info = s.boussinesq_step(T, _dt(N), NU, KAPPA, BUOY, WALLS, adiabatic=("bottom", "top"), **RULE)
            assert info.steps == 1
            cycles += info.cycles
            mk = _model(N, k + 1)
            torch.cuda.synchronize()
            assert_bitwise(s.solution(), mk.phi, f"phi after call {k + 1}")
            assert_bitwise(s.rhs(), mk.f, f"w after call {k + 1}")
            assert_bitwise(T.cpu().numpy(), mk.T, f"T after call {k + 1}")
        assert cycles == m.cycles
        _check_solve(info.last, m.last, N, "third call")
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_ERROR, C.byref(pgmg.PgmgMonitorOut())) == pgmg.PGMG_ERR_STATE
        s.vcycle(1)
        got = s.solution()
        sweeps = s.stats()[0]
    o = oracle_mod.Oracle(eps=-1.0)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(m.f), h)
    assert_bitwise(got, x, "vcycle(1) after the call")
    assert sweeps == m.last.sweeps + o.sweeps


def test_zero_buoyancy_is_the_vorticity_step(pgmg):
    """buoy = (0, 0): the flow does not see T, and phi and f equal those of vorticity_step with the
    same arguments as numbers (np.array_equal: the added +0.0 can only change the sign of a
    zero).  A moving lid, so that there is a flow."""
    N, walls, dt = 33, (0.0, 1.0, 0.0, 0.0), 0.004
    psi0, w0, T0 = _start(N)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        a = s.vorticity_step(dt, 0.01, walls, nsteps=3, **RULE)
        phi_v, f_v = s.solution(), s.rhs()
        s.set_problem(psi0, w0)
        T = _t(T0)
        b = s.boussinesq_step(T, dt, 0.01, 0.02, (0.0, 0.0), walls, nsteps=3, **RULE)
        assert np.array_equal(s.solution(), phi_v) and np.array_equal(s.rhs(), f_v)
        assert (a.cycles, a.sweeps, a.cfl, a.diffusion) == (b.cycles, b.sweeps, b.cfl, b.diffusion)
        assert np.abs(phi_v).max() > 0.0 and b.cfl > 0.0
        m = bouss_model.boussinesq_step(N, psi0, w0, T0, dt, 0.01, 0.02, (0.0, 0.0), walls, nsteps=3,
                                        omega=0.5, eps=-1.0, **RULE)
        assert_bitwise(T.cpu().numpy(), m.T, "T is carried by the lid's flow")
        assert not np.array_equal(m.T[1:-1, 1:-1], T0[1:-1, 1:-1])


def _call(pgmg, s, T, omega=0.5, dt=1e-4, nu=NU, kappa=KAPPA, buoy=BUOY, mode=0, walls=WALLS, mask=3,
          nsteps=1, info=True, opts=True, params=True, **fields):
    o, out, p = pgmg.PgmgSolveOpts(), pgmg.PgmgBoussInfo(), pgmg.PgmgBoussParams()
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, val in fields.items():
        setattr(o, k, val)
    p.dt, p.nu, p.kappa, p.mode, p.adiabatic = dt, nu, kappa, mode, mask
    p.buoy = (C.c_double * 2)(*buoy)
    p.walls = (C.c_double * 4)(*walls)
    return s.lib.pgmg_boussinesq_step(s.h, C.byref(o) if opts else None, omega,
                                      C.byref(p) if params else None, T, nsteps,
                                      C.byref(out) if info else None)


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
        assert s.lib.pgmg_boussinesq_step(None, None, 0.5, None, None, 1, None) == ARG
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
        for bad in (Tt[:-1], Tt.to(torch.float32), Tt.t(), Tt.cpu(), host):   # the Python checks
            with pytest.raises(ValueError):
                s.boussinesq_step(bad, 1e-4, NU, KAPPA)
        with pytest.raises(ValueError):
            s.boussinesq_step(Tt, 1e-4, NU, KAPPA, adiabatic=("up",))
        untouched(s, before, "refused calls")
        assert _call(pgmg, s, T) == pgmg.PGMG_OK                    # (and the arguments were good)
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


def test_refuses_row_strips(pgmg):
    import torch
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world
    keep = np.random.default_rng(7).standard_normal((N, N))
    Ts = [_t(keep) for _ in range(world)]
    torch.cuda.synchronize()

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                rc[r] = (_call(pgmg, s, C.c_void_p(Ts[r].data_ptr())), s.stats()[0])
        except Exception as e:  # surfaced below
            err[r] = e

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    hub.close()
    for e in err:
        if e is not None:
            raise e
    assert rc == [(pgmg.PGMG_ERR_STATE, 0)] * world, rc
    torch.cuda.synchronize()
    for T in Ts:
        assert_bitwise(T.cpu().numpy(), keep, "T after the refused call")


def test_boussinesq_time(pgmg):
    import torch
    N = 257
    keep = np.random.default_rng(8).standard_normal((N, N))
    T = _t(keep)
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for which, per_point in ((0, 72.0), (1, 40.0), (0, 72.0)):
            ms, b = s.boussinesq_time(which, reps=3)
            assert ms > 0.0 and b == per_point * N * N, (which, ms, b)
        assert_bitwise(s.solution(), before[0], "phi after boussinesq_time")
        assert_bitwise(s.rhs(), before[1], "f after boussinesq_time")
        assert s.stats() == before[2]
        torch.cuda.synchronize()
        assert_bitwise(T.cpu().numpy(), keep, "T after boussinesq_time")
        assert s.lib.pgmg_boussinesq_time(s.h, 2, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_boussinesq_time(s.h, 0, 0, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert s.lib.pgmg_boussinesq_time(s.h, 0, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_STATE
