"""GPU: pgmg_solve_mixed (include/pgmg.h "Mixed-precision refinement") through Solver.solve_mixed
against its model, tests/mixed_model.solve_mixed.

Three problems: oracle.rhs_mt64 with a zero frame (a caller's f), the analytic one (f regenerated
in-kernel by the parent's monitor, read as stored by the defect pass) and p = q = 0.5 with the
exact solution as the frame.  rtol = 0, atol = N^2 2^-52 ||f||_2 over the interior, 8 steps at
most, omega = 0.5.  phi is compared bitwise; the stop decisions the way tests/test_gpu_extrap.py
compares them: the device norm differs from the model's sequential one in summation order only
(solve_rule.norm_tol), and the model's smallest margin of any comparison the rule made must be
100 times that for the decisions to be comparable at all.  The scale s_i is a function of the
previous norm's exponent: every case first asserts that the model's rho_i / (N - 2) stays 1e-6
relative away from a power of two, so that the device picks the same s_i.
"""
import ctypes as C
import functools
import math
import threading

import numpy as np
import pytest

import fmg_bc_model
import mixed_model
from conftest import assert_bitwise, bits
from solve_rule import MAX_CYCLES, NONFINITE, close, norm_tol

pytestmark = pytest.mark.gpu

MAX_STEPS = 8


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _problem(kind, N):
    """(f, phi0, atol, Solver / oracle fields)"""
    import oracle
    kw = {}
    if kind == "mt":
        f, phi0 = np.array(oracle.rhs_mt64(N)), np.zeros((N, N))
    elif kind == "analytic":
        f, phi0 = oracle.Oracle().rhs(N), np.zeros((N, N))
    else:
        kw = dict(p=0.5, q=0.5)
        o = oracle.Oracle(**kw)
        f, phi0 = o.rhs(N), fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    atol = N * N * 2.0 ** -52 * float(np.linalg.norm(f[1:-1, 1:-1]))
    return _ro(f, phi0) + (atol, kw)


@functools.lru_cache(maxsize=None)
def _model(kind, N, nu):
    f, phi0, atol, kw = _problem(kind, N)
    m = mixed_model.solve_mixed(N, f, phi0, nu, 0.5, atol=atol, max_steps=MAX_STEPS, **kw)
    _ro(m.phi)
    return m


def _frame(a):
    return np.concatenate([a[0, :], a[-1, :], a[:, 0], a[:, -1]])


def _compare(info, got, m, N, what):
    print(f"{what}: {info.cycles} steps, reason {info.reason}, res {info.res:.3e} (model {m.steps}, "
          f"{m.reason}, margin {m.margin:.3e}, distance from a power of two {m.pow2_dist:.3e})")
    assert m.pow2_dist > 1e-6, (what, m.pow2_dist)
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.checks, info.reason) == (m.steps, m.checks, m.reason), what
    assert close(info.res0, m.history[0][1], N) and close(info.res, m.history[-1][1], N), what
    assert len(info.history) == len(m.history)
    for (k, r, e), (mk, mr) in zip(info.history, m.history):
        assert k == mk and close(r, mr, N) and math.isnan(e), (what, k, r, mr)
    assert_bitwise(got, m.phi, what)
    assert info.inner_sweeps == m.inner_sweeps, (what, info.inner_sweeps, m.inner_sweeps)
    if m.steps > 0:
        assert info.defect_ms > 0.0 and info.inner_ms > 0.0 and info.correct_ms > 0.0
    assert info.total_ms > 0.0


CASES = [(33, False), (65, False), (129, False), (65, True), (129, True)]


@pytest.mark.parametrize("nu,eps", [(2, 1e-7), (2, -1.0), (3, -1.0)])
@pytest.mark.parametrize("N,cross", CASES)
@pytest.mark.parametrize("kind", ["mt", "analytic", "half"])
def test_context_owned(pgmg, plan, kind, N, cross, nu, eps):
    """cross: both contexts cross-fused (cross_min_n = 9), as every N >= 2049 is by default: the
    child's cycles rotate its level-0 grids, so its phi lies in another grid after a solve.  The
    parent's eps must not matter: it runs no cycle."""
    if cross:
        plan(cross_min_n=9)
    f, phi0, atol, kw = _problem(kind, N)
    m = _model(kind, N, nu)
    with pgmg.Solver(N, eps=eps, **kw) as s:
        s.set_problem(phi0, None if kind != "mt" else f)
        before = (s.stats(), s.stats_detail())
        info = s.solve_mixed(atol=atol, max_steps=MAX_STEPS, nu=nu)
        got = s.solution()
        assert (s.stats(), s.stats_detail()) == before, "the parent's statistics moved"
        assert_bitwise(s.rhs(), f, "f")
        assert s.monitor().res_norm == info.res, "phi is not the iterate the last norm was taken on"
    _compare(info, got, m, N, f"{kind} N={N} cross={cross} nu={nu} eps={eps}")
    assert np.array_equal(bits(_frame(got)), bits(_frame(phi0))), "the frame changed"


@pytest.mark.parametrize("N,inplace", [(33, False), (65, False), (129, False), (129, True)])
@pytest.mark.parametrize("kind", ["mt", "analytic", "half"])
def test_device_bound(pgmg, plan, kind, N, inplace):
    """The caller's arrays of pgmg_set_problem_device, staged (torch tensors) and in place
    (pgmg_alloc_grid on a cross-fused context): phi and f are read where they lie, the result
    lands in the caller's phi, f comes back bitwise."""
    import torch
    if inplace:
        plan(cross_min_n=9)
    f, phi0, atol, kw = _problem(kind, N)
    m = _model(kind, N, 2)
    bound_f = kind == "mt"
    with pgmg.Solver(N, eps=-1.0, **kw) as s:
        if inplace:
            g = pgmg.DeviceGrid(N, np.array(phi0))
            fd = pgmg.DeviceGrid(N, np.array(f)) if bound_f else None
            get, getf = g.download, (fd.download if bound_f else None)
        else:
            g = torch.tensor(np.array(phi0), dtype=torch.float64, device="cuda")
            fd = torch.tensor(np.array(f), dtype=torch.float64, device="cuda") if bound_f else None
            torch.cuda.synchronize()
            get, getf = (lambda: g.cpu().numpy()), ((lambda: fd.cpu().numpy()) if bound_f else None)
        s.set_problem_device(g, fd)
        assert s.device_info() == (True, inplace)
        before = s.stats()
        info = s.solve_mixed(atol=atol, max_steps=MAX_STEPS)
        got = get()
        assert s.stats() == before
        assert_bitwise(s.solution(), got, "pgmg_get_solution reads the caller's phi")
        if bound_f:
            assert_bitwise(getf(), f, "the caller's f")
        if inplace:
            g.close()
            if fd is not None:
                fd.close()
    _compare(info, got, m, N, f"device-bound {kind} N={N} inplace={inplace}")
    assert np.array_equal(bits(_frame(got)), bits(_frame(phi0))), "the frame changed"


def test_stop_at_check_0_writes_nothing(pgmg):
    N = 33
    f, phi0, atol, kw = _problem("half", N)
    with pgmg.Solver(N, **kw) as s:
        s.set_problem(phi0, f)
        r0 = s.monitor().res_norm
        info = s.solve_mixed(atol=atol, max_steps=0)
        assert (info.cycles, info.checks, info.reason) == (0, 1, MAX_CYCLES)
        assert info.res == r0 and info.res0 == r0 and info.inner_sweeps == 0
        assert len(info.history) == 1 and info.history[0][:2] == (0, r0)
        assert_bitwise(s.solution(), phi0, "phi after max_steps = 0")
        for bad in (float("nan"), float("inf")):
            fb = np.array(f)
            fb[7, 11] = bad
            s.set_problem(phi0, fb)
            info = s.solve_mixed(atol=atol)
            assert (info.cycles, info.checks, info.reason) == (0, 1, NONFINITE), bad
            assert not math.isfinite(info.res) and info.inner_sweeps == 0
            assert_bitwise(s.solution(), phi0, f"phi after a stop on f = {bad}")
        # the context still solves afterwards
        s.set_problem(phi0, f)
        info = s.solve_mixed(atol=atol)
        m = _model("half", N, 2)
        _compare(info, s.solution(), m, N, "after the refused problems")


@pytest.mark.parametrize("cross", [False, True])
def test_second_call_same_bits_and_later_cycles(pgmg, plan, oracle_mod, cross):
    """A second call from the same start reuses the fp32 context and gives the same bits; a call
    on the converged phi stops at check 0; vcycle(1) afterwards is one oracle V-cycle of the
    model's result, started without a carry."""
    if cross:
        plan(cross_min_n=9)
    N, kind, eps = 129, "mt", 1e-7
    f, phi0, atol, kw = _problem(kind, N)
    m = _model(kind, N, 2)
    with pgmg.Solver(N, eps=eps) as s:
        outs = []
        for _ in range(2):
            s.set_problem(phi0, f)
            info = s.solve_mixed(atol=atol, max_steps=MAX_STEPS)
            outs.append((s.solution(), info.cycles, info.reason, info.inner_sweeps, info.res))
        assert_bitwise(outs[0][0], outs[1][0], "second call")
        assert outs[0][1:] == outs[1][1:]
        assert_bitwise(outs[1][0], m.phi, "against the model")
        again = s.solve_mixed(atol=atol, max_steps=MAX_STEPS)
        assert (again.cycles, again.checks, again.inner_sweeps) == (0, 1, 0) and again.res == info.res
        assert_bitwise(s.solution(), m.phi, "a call on the converged phi")
        sweeps0, taken0 = s.stats()[0], s.carry_info()[0]
        s.vcycle(1)
        got = s.solution()
        assert s.carry_info()[0] == taken0, "the V-cycle after solve_mixed started from a carry"
        sweeps = s.stats()[0] - sweeps0
    o = oracle_mod.Oracle(eps=eps)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(f))
    assert_bitwise(got, x, "vcycle(1) after solve_mixed")
    assert sweeps == o.sweeps


def test_drops_a_carry(pgmg, plan, oracle_mod):
    """v(1) makes a carry; solve_mixed in between must drop it (phi changed): v(1), one step,
    v(1) is the oracle's cycle of the model's step."""
    plan(cross_min_n=9)
    N = 257
    f, phi0, _, kw = _problem("analytic", N)
    o = oracle_mod.Oracle()
    x = np.array(phi0)
    o.v_cycle(x, np.array(f))
    m = mixed_model.solve_mixed(N, f, x, 2, 0.5, max_steps=1)
    assert m.pow2_dist > 1e-6, m.pow2_dist
    y = np.array(m.phi)
    o.v_cycle(y, np.array(f))
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        taken0, made0, _ = s.carry_info()
        info = s.solve_mixed(max_steps=1)
        assert (info.cycles, info.checks, info.reason) == (1, 2, MAX_CYCLES)
        assert_bitwise(s.solution(), m.phi, "V, one step")
        s.vcycle(1)
        taken1 = s.carry_info()[0]
        assert_bitwise(s.solution(), y, "V, one step, V")
        assert s.stats()[0] == o.sweeps
    assert made0 >= 1, "the V call before solve_mixed made no carry: the test shows nothing"
    assert taken1 == taken0, "the V-cycle after solve_mixed started from a carried pre-smooth"


def test_mixed_time(pgmg):
    N = 129
    with pgmg.Solver(N) as s:
        s.set_problem()
        for which in (0, 1):
            ms, b = s.mixed_time(which, reps=3)
            assert ms > 0.0 and b == 20.0 * N * N
        with pytest.raises(pgmg.PgmgError):
            s.mixed_time(2)


def _call(pgmg, s, nu=2, omega=0.5, **opts):
    o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgMixedInfo()
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    return s.lib.pgmg_solve_mixed(s.h, C.byref(o), nu, omega, C.byref(info))


def test_errors_enqueue_nothing(pgmg):
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    with pgmg.Solver(N) as s:
        assert _call(pgmg, s) == STATE                      # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats(), s.history())
        for bad in (0.0, 1.5, -0.5, float("nan"), float("inf")):
            assert _call(pgmg, s, omega=bad) == ARG, bad
        assert _call(pgmg, s, nu=0) == ARG
        assert _call(pgmg, s, check_every=0) == ARG
        assert _call(pgmg, s, check_every=2) == ARG
        assert _call(pgmg, s, cycle=pgmg.PGMG_CYCLE_W) == ARG
        assert _call(pgmg, s, cycle=pgmg.PGMG_CYCLE_F) == ARG
        assert _call(pgmg, s, max_cycles=-1) == ARG
        assert _call(pgmg, s, atol=-1.0) == ARG
        assert _call(pgmg, s, monitor=pgmg.PGMG_MON_RESIDUAL | pgmg.PGMG_MON_ERROR) == ARG
        o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgMixedInfo()
        s.lib.pgmg_solve_opts_default(C.byref(o))
        assert s.lib.pgmg_solve_mixed(None, C.byref(o), 2, 0.5, C.byref(info)) == ARG
        assert s.lib.pgmg_solve_mixed(s.h, None, 2, 0.5, C.byref(info)) == ARG
        assert s.lib.pgmg_solve_mixed(s.h, C.byref(o), 2, 0.5, None) == ARG
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert (s.stats(), s.history()) == before[1:]
    for n, kw in ((9, dict(n_coarse=3)), (17, dict(n_coarse=4))):
        with pgmg.Solver(n, **kw) as s:                     # a coarsest level of 3 points
            s.set_problem()
            assert _call(pgmg, s) == ARG, (n, kw)
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert _call(pgmg, s) == STATE
        assert "fp64 contexts only" in s.lib.pgmg_last_error().decode()
        ms, b = C.c_double(), C.c_double()
        assert s.lib.pgmg_mixed_time(s.h, 0, 3, C.byref(ms), C.byref(b)) == STATE


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
