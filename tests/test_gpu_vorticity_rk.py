"""GPU: pgmg_vorticity_step_rk (include/pgmg.h "Runge-Kutta vorticity transport") through
Solver.vorticity_step(order=2 and 3) against its model, tests/vort_rk_model.vorticity_step_rk: phi,
f with its frame and the statistics bitwise or equal, the stop decisions the way
tests/test_gpu_vorticity.py compares them.

The flow, the rule and the time steps are that file's: the lid-driven cavity at Re = 100 from rest,
walls = (0, 1, 0, 0), nu = 0.01, dt = 0.01, 0.004, 0.001 at N = 33, 65, 129; omega = 0.5 for the
damped solve, eps < 0, rtol = 0, atol = 1e-8, at most 30 cycles.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import vort_model
import vort_rk_model
from conftest import assert_bitwise, bits
from solve_rule import close, norm_tol

pytestmark = pytest.mark.gpu

NU, WALLS = 0.01, (0.0, 1.0, 0.0, 0.0)
RULE = dict(max_cycles=30, rtol=0.0, atol=1e-8)
DT = {33: 0.01, 65: 0.004, 129: 0.001}


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _start(N):
    psi0, w0 = np.zeros((N, N)), np.zeros((N, N))
    psi0[0, 3], psi0[-1, 0], psi0[2, -1] = -0.0, -0.0, -0.0
    for a in (psi0, w0):
        a.setflags(write=False)
    return psi0, w0


@functools.lru_cache(maxsize=None)
def _model(N, order, nsteps):
    psi0, w0 = _start(N)
    m = vort_rk_model.vorticity_step_rk(N, psi0, w0, DT[N], NU, WALLS, False, order, nsteps, omega=0.5,
                                        eps=-1.0, **RULE)
    m.phi.setflags(write=False)
    m.f.setflags(write=False)
    return m


def _check_solve(info, m, N, what):
    print(f"{what}: {info.cycles} cycles, reason {info.reason}, res {info.res:.3e} "
          f"(model {m.cycles}, {m.reason}, margin {m.margin:.3e})")
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.checks, info.reason) == (m.cycles, m.checks, m.reason), what
    assert close(info.res0, m.history[0][1], N) and close(info.res, m.history[-1][1], N), what


def _compare(s, info, m, N, nsteps, what):
    psi0, _ = _start(N)
    assert info.steps == nsteps, what
    _check_solve(info.last, m.last, N, what)
    got = s.solution()
    assert_bitwise(got, m.phi, what + " phi")
    assert_bitwise(s.rhs(), m.f, what + " omega")
    frame = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
    want = np.concatenate([psi0[0], psi0[-1], psi0[:, 0], psi0[:, -1]])
    assert np.array_equal(bits(frame), bits(want)), "phi's frame changed"
    # the statistics: the context's start over at every stage, the info sums them
    assert s.stats()[0] == m.last.sweeps, (what, s.stats(), m.last.sweeps)
    assert (info.cycles, info.sweeps) == (m.cycles, m.sweeps), (what, info.cycles, m.cycles)
    print(f"{what}: cfl {info.cfl!r} (model {m.cfl!r}), diffusion {info.diffusion!r}")
    assert bits(np.array([info.cfl, info.diffusion])).tolist() == bits(np.array([m.cfl, m.diffusion])).tolist()
    assert info.worst_res >= info.last.res > 0.0 and info.worst_reason in (1, 2, 3)
    assert info.step_ms > 0.0 and info.solve_ms > 0.0 and info.elapsed_ms >= info.solve_ms


def _run(pgmg, N, order, nsteps=2, **kw):
    psi0, w0 = _start(N)
    m = _model(N, order, nsteps)
    what = f"cavity N={N} order={order} nsteps={nsteps} {kw}"
    with pgmg.Solver(N, eps=-1.0, **kw) as s:
        s.set_problem(None, None)        # an analytic problem and cycles before: all replaced
        s.vcycle(1)
        s.set_problem(psi0, w0)
        info = s.vorticity_step(DT[N], NU, WALLS, nsteps=nsteps, order=order, **RULE)
        _compare(s, info, m, N, nsteps, what)
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
def test_free_slip(pgmg, order):
    """PGMG_WALL_FREE on a random vorticity: the frame omega came with is replaced by +0.0, in f
    and so in the saved omega too."""
    N = 33
    rng = np.random.default_rng(11)
    psi0 = np.zeros((N, N))
    w0 = np.zeros((N, N))
    w0[1:-1, 1:-1] = rng.standard_normal((N - 2, N - 2))
    w0[0, :] = 5.0                      # a frame the wall pass replaces
    m = vort_rk_model.vorticity_step_rk(N, psi0, w0, 1e-3, NU, WALLS, True, order, 2, omega=0.5,
                                        eps=-1.0, **RULE)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        info = s.vorticity_step(1e-3, NU, WALLS, free=True, nsteps=2, order=order, **RULE)
        assert_bitwise(s.solution(), m.phi, "phi")
        f = s.rhs()
        assert_bitwise(f, m.f, "omega")
        assert not bits(np.concatenate([f[0], f[-1], f[:, 0], f[:, -1]])).any()
        assert (info.steps, info.cycles, info.sweeps) == (2, m.cycles, m.sweeps)
        assert bits(np.array([info.cfl])).tolist() == bits(np.array([m.cfl])).tolist()


def _call(pgmg, s, omega=0.5, dt=1e-3, nu=NU, mode=0, walls=WALLS, order=3, nsteps=1, info=True,
          opts=True, out=None, **fields):
    o, out = pgmg.PgmgSolveOpts(), pgmg.PgmgVortInfo() if out is None else out
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, val in fields.items():
        setattr(o, k, val)
    w = None if walls is None else (C.c_double * 4)(*walls)
    return s.lib.pgmg_vorticity_step_rk(s.h, C.byref(o) if opts else None, omega, dt, nu, mode, w,
                                        order, nsteps, C.byref(out) if info else None)


def test_order_1_is_the_euler_entry(pgmg):
    """pgmg_vorticity_step_rk(order = 1) against pgmg_vorticity_step from the same start on two
    contexts: phi, f and every field of info but the times, bit for bit; and against the Euler
    model."""
    N, nsteps = 65, 3
    psi0, w0 = _start(N)
    res = []
    for rk in (False, True):
        with pgmg.Solver(N, eps=-1.0) as s:
            s.set_problem(psi0, w0)
            if rk:
                info = pgmg.PgmgVortInfo()
                assert _call(pgmg, s, dt=DT[N], order=1, nsteps=nsteps, out=info, **RULE) == pgmg.PGMG_OK
            else:
                info = s.vorticity_step(DT[N], NU, WALLS, nsteps=nsteps, **RULE)
            fields = [info.steps, info.cycles, info.sweeps, info.worst_reason, info.worst_res, info.cfl,
                      info.diffusion]
            fields += [getattr(info.last, name) for name, _ in pgmg.PgmgSolveInfo._fields_
                       if not name.endswith("_ms")]
            res.append((s.solution(), s.rhs(), fields, s.stats()))
    (p0, f0, i0, s0), (p1, f1, i1, s1) = res
    assert_bitwise(p1, p0, "phi")
    assert_bitwise(f1, f0, "omega")
    assert bits(np.array(i1, dtype=np.float64)).tolist() == bits(np.array(i0, dtype=np.float64)).tolist(), (i0, i1)
    assert s1 == s0 and i0[0] == nsteps and i0[1] >= nsteps
    m = vort_model.vorticity_step(N, psi0, w0, DT[N], NU, WALLS, False, nsteps, omega=0.5, eps=-1.0, **RULE)
    assert_bitwise(p1, m.phi, "phi against the Euler model")
    assert_bitwise(f1, m.f, "omega against the Euler model")


def test_three_calls_and_what_follows(pgmg, oracle_mod):
    """nsteps = 3 equals three calls of one step, order 3; a gradient and a vcycle afterwards
    continue from (psi, omega)."""
    import torch
    import grad_model
    N, order = 33, 3
    h = 1.0 / (N - 1)
    psi0, w0 = _start(N)
    m = _model(N, order, 3)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        cycles = 0
        for k in range(3):
            info = s.vorticity_step(DT[N], NU, WALLS, order=order, **RULE)
            assert info.steps == 1
            cycles += info.cycles
            mk = _model(N, order, k + 1)
            assert_bitwise(s.solution(), mk.phi, f"phi after call {k + 1}")
            assert_bitwise(s.rhs(), mk.f, f"omega after call {k + 1}")
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
        info = s.vorticity_step(DT[N], NU, WALLS, nsteps=3, order=order, **RULE)
        _compare(s, info, m, N, 3, "nsteps = 3")


def test_errors_write_nothing(pgmg):
    import torch
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    nan, inf = float("nan"), float("inf")

    def untouched(s, before, what):
        assert_bitwise(s.solution(), before[0], what + ": phi")
        assert_bitwise(s.rhs(), before[1], what + ": f")
        assert s.stats() == before[2], what

    with pgmg.Solver(N) as s:
        assert _call(pgmg, s) == STATE                              # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for bad in (0, 4, -1, 17):
            assert _call(pgmg, s, order=bad) == ARG, bad
        assert s.lib.pgmg_vorticity_step_rk(None, None, 0.5, 1e-3, NU, 0, None, 3, 1, None) == ARG
        assert _call(pgmg, s, info=False) == ARG and _call(pgmg, s, opts=False) == ARG
        assert _call(pgmg, s, walls=None) == ARG
        assert _call(pgmg, s, check_every=0) == ARG
        assert _call(pgmg, s, monitor=pgmg.PGMG_MON_RESIDUAL | pgmg.PGMG_MON_ERROR) == ARG
        for bad in (0.0, 1.5, -0.5, nan, inf):
            assert _call(pgmg, s, omega=bad) == ARG, bad
        for bad in (0.0, -1e-3, nan, inf):
            assert _call(pgmg, s, dt=bad) == ARG, bad
        for bad in (-1e-9, nan, inf):
            assert _call(pgmg, s, nu=bad) == ARG, bad
        for bad in (-1, 2, 5):
            assert _call(pgmg, s, mode=bad) == ARG, bad
        for k in range(4):
            for bad in (nan, inf, -inf):
                ws = list(WALLS)
                ws[k] = bad
                assert _call(pgmg, s, walls=ws) == ARG and _call(pgmg, s, walls=ws, mode=1) == ARG
        for bad in (0, -3):
            assert _call(pgmg, s, nsteps=bad) == ARG, bad
        untouched(s, before, "refused calls")
        with pytest.raises(pgmg.PgmgError):
            s.vorticity_step(1e-3, NU, WALLS, order=4)
        untouched(s, before, "order 4 through the Solver")
        for order in (1, 2, 3):
            assert _call(pgmg, s, order=order) == pgmg.PGMG_OK      # (and the arguments were good)
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        before = (s.solution(), s.rhs(), s.stats())
        assert _call(pgmg, s) == STATE
        untouched(s, before, "fp32")
    keep = np.random.default_rng(5).standard_normal((N, N))
    with pgmg.Solver(N) as s:             # a device-bound problem: f is the caller's
        g, fd = _t(np.zeros((N, N))), _t(keep)
        s.set_problem_device(g, fd)
        assert _call(pgmg, s) == STATE
        torch.cuda.synchronize()
        assert_bitwise(fd.cpu().numpy(), keep, "the caller's f")
        assert not g.cpu().numpy().any()


def test_refuses_row_strips(pgmg):
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                rc[r] = (_call(pgmg, s), s.stats()[0])
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


def test_vorticity_rk_time(pgmg):
    N = 257
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for which, per_point in ((0, 48.0), (1, 32.0), (0, 48.0)):
            ms, b = s.vorticity_rk_time(which, reps=3)
            assert ms > 0.0 and b == per_point * N * N, (which, ms, b)
        assert_bitwise(s.solution(), before[0], "phi after vorticity_rk_time")
        assert_bitwise(s.rhs(), before[1], "f after vorticity_rk_time")
        assert s.stats() == before[2]
        assert s.lib.pgmg_vorticity_rk_time(s.h, 2, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_vorticity_rk_time(s.h, 0, 0, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert s.lib.pgmg_vorticity_rk_time(s.h, 0, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_STATE
