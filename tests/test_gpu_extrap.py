"""GPU: pgmg_solve_extrap (include/pgmg.h "Fourth-order solves by Richardson extrapolation")
through Solver.solve(order=4) against its model, tests/extrap_model.solve_extrap.

Two problems: the analytic one with p = q = 0.5 and the exact solution as the frame (f
regenerated in-kernel on the parent, stored and injected for the child) and oracle.rhs_mt64 with a
zero frame (a caller's f).  rtol = 0 and atol = 1e-10 ||f||_2 over the interior (what the header
recommends), 40 cycles at most, nu = 2, omega = 0.5.  phi is compared bitwise; the stop decisions
the way tests/test_damp_gpu.py compares them: the device norm differs from the model's sequential
one in summation order only (solve_rule.norm_tol), and the model's smallest margin of any
comparison the rule made must be 100 times that for the decisions to be comparable at all.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import extrap_model
import fmg_bc_model
from conftest import assert_bitwise, bits
from solve_rule import close, norm_tol

pytestmark = pytest.mark.gpu

PQ = 0.5
RULE = dict(max_cycles=40, rtol=0.0)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _problem(kind, N):
    """(f, phi0, atol)"""
    import oracle
    if kind == "analytic":
        o = oracle.Oracle(p=PQ, q=PQ)
        f = o.rhs(N)
        phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    else:
        f = np.array(oracle.rhs_mt64(N))
        phi0 = np.zeros((N, N))
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    return _ro(f, phi0) + (atol,)


@functools.lru_cache(maxsize=None)
def _model(kind, N, eps):
    f, phi0, atol = _problem(kind, N)
    m = extrap_model.solve_extrap(N, f, phi0, 2, 0.5, eps=eps, atol=atol, **RULE)
    _ro(m.phi, m.phi2)
    return m


def _solver(pgmg, kind, N, eps, **kw):
    if kind == "analytic":
        kw.update(p=PQ, q=PQ)
    return pgmg.Solver(N, eps=eps, **kw)


def _check_solve(info, m, N, what):
    """cycles, checks, reason and the norms of one of the two solves against the model's"""
    print(f"{what}: {info.cycles} cycles, reason {info.reason}, res {info.res:.3e} "
          f"(model {m.cycles}, {m.reason}, margin {m.margin:.3e})")
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.checks, info.reason) == (m.cycles, m.checks, m.reason), what
    assert close(info.res0, m.history[0][1], N) and close(info.res, m.history[-1][1], N), what


def _compare(info, got, fine_sweeps, m, N, what):
    Nc = (N + 1) // 2
    _check_solve(info, m.fine, N, what + " fine")
    _check_solve(info.coarse, m.coarse, Nc, what + " coarse")
    assert len(info.history) == len(m.fine.history)
    for (k, r, _), (mk, mr, _) in zip(info.history, m.fine.history):
        assert k == mk and close(r, mr, N), (what, k, r, mr)
    assert_bitwise(got, m.phi, what)
    assert fine_sweeps == m.fine.sweeps, (what, fine_sweeps, m.fine.sweeps)
    assert info.coarse_sweeps == m.coarse.sweeps, (what, info.coarse_sweeps, m.coarse.sweeps)
    assert info.extrap_ms > 0.0 and info.total_ms >= info.elapsed_ms > 0.0


@pytest.mark.parametrize("eps", [-1.0, 1e-7])
@pytest.mark.parametrize("N,cross", [(33, False), (65, False), (129, False), (65, True), (129, True)])
@pytest.mark.parametrize("kind", ["analytic", "mt"])
def test_context_owned(pgmg, plan, kind, N, cross, eps):
    """cross: both contexts cross-fused (cross_min_n = 9), as every N >= 2049 is by default: their
    cycles rotate the level-0 grids, so phi lies in another grid after the solves than before."""
    if cross:
        plan(cross_min_n=9)
    f, phi0, atol = _problem(kind, N)
    m = _model(kind, N, eps)
    with _solver(pgmg, kind, N, eps) as s:
        s.set_problem(phi0, None if kind == "analytic" else f)
        info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
        got = s.solution()
        sweeps = s.stats()[0]
    _compare(info, got, sweeps, m, N, f"{kind} N={N} eps={eps}")
    frame = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
    want = np.concatenate([phi0[0], phi0[-1], phi0[:, 0], phi0[:, -1]])
    assert np.array_equal(bits(frame), bits(want)), "the frame changed"


@pytest.mark.parametrize("eps", [-1.0, 1e-7])
@pytest.mark.parametrize("N,inplace", [(33, False), (65, False), (129, False), (129, True)])
@pytest.mark.parametrize("kind", ["analytic", "mt"])
def test_device_bound(pgmg, plan, kind, N, inplace, eps):
    """The caller's arrays of pgmg_set_problem_device, staged (torch tensors) and in place
    (pgmg_alloc_grid on a cross-fused context; the child is cross-fused too): the result lands
    in the caller's phi, f comes back bitwise."""
    import torch
    if inplace:
        plan(cross_min_n=9)
    f, phi0, atol = _problem(kind, N)
    m = _model(kind, N, eps)
    bound_f = kind != "analytic"
    with _solver(pgmg, kind, N, eps) as s:
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
        info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
        got = get()
        sweeps = s.stats()[0]
        assert_bitwise(s.solution(), got, "pgmg_get_solution reads the caller's phi")
        if bound_f:
            assert_bitwise(getf(), f, "the caller's f")
        if inplace:
            g.close()
            if fd is not None:
                fd.close()
    _compare(info, got, sweeps, m, N, f"device-bound {kind} N={N} inplace={inplace} eps={eps}")


def test_fourth_order_on_the_device(pgmg, oracle_mod):
    """rel_error of the extrapolated phi at N = 129 and 257 (p = q = 0.5): the model's within 1e-6
    relative (the same phi; the monitor sums in another order), and the ratio at least 14."""
    errs = []
    for N in (129, 257):
        f, phi0, atol = _problem("analytic", N)
        m = _model("analytic", N, -1.0)
        want = oracle_mod.Oracle(p=PQ, q=PQ).rel_error(m.phi)
        with _solver(pgmg, "analytic", N, -1.0) as s:
            s.set_problem(phi0, None)
            info = s.solve(order=4, damp=0.5, atol=atol, error=True, **RULE)
            got = s.monitor(error=True).rel_error
        print(f"N={N}: rel_error {got:.6e} (model {want:.6e}), second order {info.rel_error:.6e}")
        assert abs(got - want) <= 1e-6 * want, (N, got, want)
        assert got < info.rel_error / 1000.0   # (info.rel_error: the fine solve's last check)
        errs.append(got)
    assert errs[0] / errs[1] >= 14.0, errs


@pytest.mark.parametrize("cross", [False, True])
def test_second_call_same_bits_and_later_cycles(pgmg, plan, oracle_mod, cross):
    """A second call from the same start reuses the half-resolution context and gives the same
    bits and statistics; vcycle(1) afterwards is one oracle V-cycle of the model's result."""
    if cross:
        plan(cross_min_n=9)
    N, kind, eps = 65, "mt", 1e-7
    f, phi0, atol = _problem(kind, N)
    m = _model(kind, N, eps)
    with _solver(pgmg, kind, N, eps) as s:
        outs = []
        for _ in range(2):
            s.set_problem(phi0, f)
            info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
            outs.append((s.solution(), s.stats(), info.coarse_sweeps, info.coarse_exits,
                         info.cycles, info.coarse.cycles))
        assert_bitwise(outs[0][0], outs[1][0], "second call")
        assert outs[0][1:] == outs[1][1:]
        assert_bitwise(outs[1][0], m.phi, "against the model")
        s.vcycle(1)
        got = s.solution()
        sweeps = s.stats()[0]
    o = oracle_mod.Oracle(eps=eps)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(f))
    assert_bitwise(got, x, "vcycle(1) after the extrapolation")
    assert sweeps == m.fine.sweeps + o.sweeps


def test_set_eps_reaches_the_child(pgmg):
    N, kind = 65, "mt"
    f, phi0, atol = _problem(kind, N)
    m7, m3 = _model(kind, N, 1e-7), _model(kind, N, 1e-3)
    assert m7.coarse.sweeps != m3.coarse.sweeps, "the two eps give the same child: nothing shown"
    with _solver(pgmg, kind, N, 1e-7) as s:
        s.set_problem(phi0, f)
        info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
        assert info.coarse_sweeps == m7.coarse.sweeps
        s.set_eps(1e-3)
        s.set_problem(phi0, f)
        info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
        got = s.solution()
        sweeps = s.stats()[0]
    _compare(info, got, sweeps, m3, N, "after set_eps(1e-3)")


def _call(pgmg, s, nu=2, omega=0.5, **opts):
    o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgExtrapInfo()
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    return s.lib.pgmg_solve_extrap(s.h, C.byref(o), nu, omega, C.byref(info))


def test_errors_enqueue_nothing(pgmg):
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    with pgmg.Solver(N) as s:
        assert _call(pgmg, s) == STATE                      # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats())
        for bad in (0.0, 1.5, -0.5, float("nan"), float("inf")):
            assert _call(pgmg, s, omega=bad) == ARG, bad
        assert _call(pgmg, s, nu=0) == ARG
        assert _call(pgmg, s, check_every=0) == ARG
        o = pgmg.PgmgSolveOpts()
        s.lib.pgmg_solve_opts_default(C.byref(o))
        info = pgmg.PgmgExtrapInfo()
        assert s.lib.pgmg_solve_extrap(None, C.byref(o), 2, 0.5, C.byref(info)) == ARG
        assert s.lib.pgmg_solve_extrap(s.h, None, 2, 0.5, C.byref(info)) == ARG
        assert s.lib.pgmg_solve_extrap(s.h, C.byref(o), 2, 0.5, None) == ARG
        with pytest.raises(ValueError):
            s.solve(order=4)                                # damp = 0
        with pytest.raises(ValueError):
            s.solve(order=3, damp=0.5)
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
    for n, kw in ((5, {}), (9, dict(n_coarse=3)), (17, dict(n_coarse=4))):
        with pgmg.Solver(n, **kw) as s:                     # N < 9; a coarsest level of 3 points
            s.set_problem()
            assert _call(pgmg, s) == ARG, (n, kw)
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert _call(pgmg, s) == STATE
        assert "rounding floor" in s.lib.pgmg_last_error().decode()
    with pgmg.Solver(N) as s:                               # the error norm of a caller's f
        s.set_problem(None, np.zeros((N, N)))
        assert _call(pgmg, s, monitor=pgmg.PGMG_MON_RESIDUAL | pgmg.PGMG_MON_ERROR) == STATE


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
