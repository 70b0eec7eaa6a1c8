"""GPU: pgmg_vorticity_step (include/pgmg.h "Vorticity transport") through Solver.vorticity_step
against its model, tests/vort_model.vorticity_step: phi, f with its frame and the statistics
bitwise or equal, the stop decisions the way tests/test_gpu_project.py compares them (the device
norms differ from the model's sequential ones in summation order only: solve_rule.norm_tol).

The flow is the lid-driven cavity at Re = 100 from rest: walls = (0, 1, 0, 0), nu = 0.01, psi0 = 0
(with a -0.0 on its frame), omega0 = 0; dt = 0.01, 0.004, 0.001 at N = 33, 65, 129 (diffusion
numbers 0.41, 0.66, 0.66); omega = 0.5 for the damped solve, eps < 0, rtol = 0, atol = 1e-8, at
most 30 cycles.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import grad_model
import vort_model
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
def _model(N, nsteps, free=False):
    psi0, w0 = _start(N)
    m = vort_model.vorticity_step(N, psi0, w0, DT[N], NU, WALLS, free, nsteps, omega=0.5, eps=-1.0,
                                  **RULE)
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
    h = 1.0 / (N - 1)
    assert info.steps == nsteps, what
    _check_solve(info.last, m.last, N, what)
    assert len(info.history) == len(m.last.history), what
    for (k, r, _), (mk, mr, _) in zip(info.history, m.last.history):
        assert k == mk and close(r, mr, N), (what, k, r, mr)
    got = s.solution()
    assert_bitwise(got, m.phi, what + " phi")
    assert_bitwise(s.rhs(), m.f, what + " omega")
    frame = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
    want = np.concatenate([psi0[0], psi0[-1], psi0[:, 0], psi0[:, -1]])
    assert np.array_equal(bits(frame), bits(want)), "phi's frame changed"
    # the statistics: the context's start over at every step, the info sums them
    assert s.stats()[0] == m.last.sweeps, (what, s.stats(), m.last.sweeps)
    assert (info.cycles, info.sweeps) == (m.cycles, m.sweeps), (what, info.cycles, m.cycles)
    print(f"{what}: cfl {info.cfl!r} (model {m.cfl!r}), diffusion {info.diffusion!r}")
    assert bits(np.array([info.cfl, info.diffusion])).tolist() == bits(np.array([m.cfl, m.diffusion])).tolist()
    assert info.worst_res >= info.last.res > 0.0 and info.worst_reason in (1, 2, 3)
    assert info.step_ms > 0.0 and info.solve_ms > 0.0 and info.elapsed_ms >= info.solve_ms
    assert m.f[-1, 1:-1].min() < -2.0 / h * 0.5, "the lid's vorticity is there"


def _run(pgmg, N, nsteps=3, **kw):
    psi0, w0 = _start(N)
    m = _model(N, nsteps)
    what = f"cavity N={N} nsteps={nsteps} {kw}"
    with pgmg.Solver(N, eps=-1.0, **kw) as s:
        s.set_problem(None, None)        # an analytic problem and cycles before: all replaced
        s.vcycle(1)
        s.set_problem(psi0, w0)
        info = s.vorticity_step(DT[N], NU, WALLS, nsteps=nsteps, **RULE)
        _compare(s, info, m, N, nsteps, what)
        # the problem is one with a caller's f
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_ERROR, C.byref(pgmg.PgmgMonitorOut())) == pgmg.PGMG_ERR_STATE
        return s.stats_detail()[2] >= 0   # level 0 is cross-fused


@pytest.mark.parametrize("N", [33, 65])
def test_cavity_against_the_model(pgmg, N):
    _run(pgmg, N)


def test_cross_fused_level_0(pgmg, plan):
    """N = 129 with tail_n = 17 and cross_min_n = 9: level 0 is cross-fused, its cycles rotate the
    level-0 grids, and every wall and step pass reads psi where it lies then."""
    assert not _run(pgmg, 129, tail_n=17)
    plan(cross_min_n=9)
    assert _run(pgmg, 129, tail_n=17)


def test_three_calls_and_what_follows(pgmg, oracle_mod):
    """nsteps = 3 equals three calls of one step (the closing wall pass of a call is the opening
    one of the next, bit for bit); Solver.rhs() is omega; velocity() is two gradient calls; a
    vcycle afterwards continues from (psi, omega)."""
    import torch
    N = 65
    h = 1.0 / (N - 1)
    psi0, w0 = _start(N)
    m = _model(N, 3)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        cycles = 0
        for k in range(3):
            info = s.vorticity_step(DT[N], NU, WALLS, **RULE)
            assert info.steps == 1
            cycles += info.cycles
            mk = _model(N, k + 1)
            assert_bitwise(s.solution(), mk.phi, f"phi after call {k + 1}")
            assert_bitwise(s.rhs(), mk.f, f"omega after call {k + 1}")
        assert cycles == m.cycles
        _check_solve(info.last, m.last, N, "third call")
        u, v = s.velocity()
        gy = s.gradient(order=2, scale=1.0)[1]
        gx = s.gradient(order=2, scale=-1.0)[0]
        torch.cuda.synchronize()
        assert_bitwise(u.cpu().numpy(), gy.cpu().numpy(), "u = psi_y")
        assert_bitwise(v.cpu().numpy(), gx.cpu().numpy(), "v = -psi_x")
        wx, wy = grad_model.gradient(m.phi, h, 2, 1.0)
        assert_bitwise(u.cpu().numpy(), wy, "u against the model")
        assert_bitwise(v.cpu().numpy(), grad_model.gradient(m.phi, h, 2, -1.0)[0], "v against the model")
        with pytest.raises(ValueError):
            s.velocity(u.to(torch.float32), v)
        s.vcycle(1)
        got = s.solution()
        sweeps = s.stats()[0]
    o = oracle_mod.Oracle(eps=-1.0)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(m.f), h)
    assert_bitwise(got, x, "vcycle(1) after the call")
    assert sweeps == m.last.sweeps + o.sweeps


def test_free_slip(pgmg):
    """PGMG_WALL_FREE on a random vorticity: the frame omega came with is replaced by +0.0."""
    N = 33
    rng = np.random.default_rng(11)
    psi0 = np.zeros((N, N))
    w0 = np.zeros((N, N))
    w0[1:-1, 1:-1] = rng.standard_normal((N - 2, N - 2))
    w0[0, :] = 5.0                      # a frame the wall pass replaces
    m = vort_model.vorticity_step(N, psi0, w0, 1e-3, NU, WALLS, True, 2, omega=0.5, eps=-1.0, **RULE)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(psi0, w0)
        info = s.vorticity_step(1e-3, NU, WALLS, free=True, nsteps=2, **RULE)
        assert_bitwise(s.solution(), m.phi, "phi")
        f = s.rhs()
        assert_bitwise(f, m.f, "omega")
        assert not bits(np.concatenate([f[0], f[-1], f[:, 0], f[:, -1]])).any()
        assert (info.cycles, info.sweeps) == (m.cycles, m.sweeps)


def _call(pgmg, s, omega=0.5, dt=1e-3, nu=NU, mode=0, walls=WALLS, nsteps=1, info=True, opts=True,
          **fields):
    o, out = pgmg.PgmgSolveOpts(), pgmg.PgmgVortInfo()
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, val in fields.items():
        setattr(o, k, val)
    w = None if walls is None else (C.c_double * 4)(*walls)
    return s.lib.pgmg_vorticity_step(s.h, C.byref(o) if opts else None, omega, dt, nu, mode, w, nsteps,
                                     C.byref(out) if info else None)


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
        assert s.lib.pgmg_vorticity_step(None, None, 0.5, 1e-3, NU, 0, None, 1, None) == ARG
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
        assert _call(pgmg, s) == pgmg.PGMG_OK                       # (and the arguments were good)
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


def test_vorticity_time(pgmg):
    N = 257
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for which, per_point in ((0, 40.0), (1, 24.0), (0, 40.0)):
            ms, b = s.vorticity_time(which, reps=3)
            assert ms > 0.0 and b == per_point * N * N, (which, ms, b)
        assert_bitwise(s.solution(), before[0], "phi after vorticity_time")
        assert_bitwise(s.rhs(), before[1], "f after vorticity_time")
        assert s.stats() == before[2]
        assert s.lib.pgmg_vorticity_time(s.h, 2, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_vorticity_time(s.h, 0, 0, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert s.lib.pgmg_vorticity_time(s.h, 0, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_STATE
