"""GPU: pgmg_project (include/pgmg.h "Projection") through Solver.project against its model,
tests/proj_model.project: phi, u, v and the stored f bitwise, the statistics equal, the stop
decisions the way tests/test_gpu_extrap.py compares them (the device norms differ from the model's
sequential ones in summation order only: solve_rule.norm_tol).  div_before and div_after are sums
in the pass's own order: they are compared bit for bit with ops.divergence's norm of the same
arrays (the same kernel on the same decomposition, itself bitwise against the model's values in
tests/test_gpu_divergence_grid.py) and with the model's sequential sum within N^2 2^-52.

nu = 2, omega = 0.5, eps < 0, rtol = 0, atol = 1e-10 ||f||_2 over the interior, at most 40 cycles.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import grad_model
import proj_model
from conftest import assert_bitwise, bits
from solve_rule import close, norm_tol

pytestmark = pytest.mark.gpu

RULE = dict(max_cycles=40, rtol=0.0)
KINDS = ["pq11", "pq0515", "random", "h0"]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _h0(kind, N):
    return 0.7 / (N - 1) if kind == "h0" else None


@functools.lru_cache(maxsize=None)
def _problem(kind, N):
    """(u*, v*, phi0): the table's fields with a zero frame (pq11) or psi's (pq0515, h0), or a
    random field and a random frame with a -0.0 in it"""
    if kind == "random":
        rng = np.random.default_rng(9000 + N)
        u, v = rng.standard_normal((N, N)), rng.standard_normal((N, N))
        phi0 = rng.standard_normal((N, N))     # (the interior is ignored)
        phi0[0, 3], phi0[-1, 0], phi0[2, -1] = -0.0, -0.0, 0.0
    else:
        p, q = (1.0, 1.0) if kind == "pq11" else (0.5, 1.5)
        u, v, _, _, phi0 = proj_model.table_fields(p, q, N)
        if kind == "pq11":
            phi0 = np.zeros((N, N))
    return _ro(u, v, phi0)


@functools.lru_cache(maxsize=None)
def _model(kind, N, order, eps=-1.0):
    u, v, phi0 = _problem(kind, N)
    h0 = _h0(kind, N)
    f = proj_model.divergence(u, v, h0 or 1.0 / (N - 1), order, -1.0)
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    m = proj_model.project(N, u, v, phi0, order, 2, 0.5, eps=eps, h0=h0, atol=atol, **RULE)
    m.atol = atol
    _ro(m.phi, m.u, m.v, m.f)
    return m


def _solver(pgmg, kind, N, eps=-1.0, **kw):
    if _h0(kind, N):
        kw["h0"] = _h0(kind, N)
    return pgmg.Solver(N, eps=eps, **kw)


def _same_bits(a, b):
    return bits(np.array([a]))[0] == bits(np.array([b]))[0]


def _check_solve(info, m, N, what):
    print(f"{what}: {info.cycles} cycles, reason {info.reason}, res {info.res:.3e} "
          f"(model {m.cycles}, {m.reason}, margin {m.margin:.3e})")
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.checks, info.reason) == (m.cycles, m.checks, m.reason), what
    assert close(info.res0, m.history[0][1], N) and close(info.res, m.history[-1][1], N), what


def _compare(pgmg, s, info, u, v, ut, vt, m, N, order, what, h):
    """everything the call on (u, v), now (ut, vt), leaves against the model m"""
    import torch
    torch.cuda.synchronize()
    _check_solve(info.solve.fine, m.fine, N, what + " fine")
    if order == 4:
        _check_solve(info.solve.coarse, m.coarse, (N + 1) // 2, what + " coarse")
        assert info.solve.coarse_sweeps == m.coarse.sweeps, what
        assert info.solve.extrap_ms > 0.0
    else:
        assert bytes(info.solve.coarse) == bytes(pgmg.PgmgSolveInfo()), what + ": coarse is not zero"
        assert (info.solve.coarse_sweeps, info.solve.coarse_exits, info.solve.extrap_ms) == (0, 0, 0.0)
    assert len(info.history) == len(m.fine.history), what
    for (k, r, _), (mk, mr, _) in zip(info.history, m.fine.history):
        assert k == mk and close(r, mr, N), (what, k, r, mr)
    assert_bitwise(s.solution(), m.phi, what + " phi")
    assert_bitwise(s.rhs(), m.f, what + " f")
    assert_bitwise(ut.cpu().numpy(), m.u, what + " u")
    assert_bitwise(vt.cpu().numpy(), m.v, what + " v")
    assert s.stats() == (m.fine.sweeps, m.fine.exits), (what, s.stats(), m.fine.sweeps, m.fine.exits)
    # the two norms: the pass's own sums
    n_before = pgmg.ops.divergence(_t(u), _t(v), h, order=order, scale=-1.0, norm=True)[1]
    n_after = pgmg.ops.divergence(ut, vt, h, order=order, scale=-1.0, norm=True)[1]
    print(f"{what}: div_before {info.div_before!r} (model {m.div_before!r}), div_after "
          f"{info.div_after!r} (model {m.div_after!r})")
    assert _same_bits(info.div_before, n_before) and _same_bits(info.div_after, n_after), what
    assert abs(info.div_before - m.div_before) <= N * N * 2.0 ** -52 * m.div_before, what
    assert abs(info.div_after - m.div_after) <= N * N * 2.0 ** -52 * m.div_after, what
    assert info.div_ms > 0.0 and info.update_ms > 0.0
    assert info.elapsed_ms >= info.solve.fine.elapsed_ms > 0.0


def _run(pgmg, kind, N, order, **kw):
    u, v, phi0 = _problem(kind, N)
    m = _model(kind, N, order)
    what = f"{kind} N={N} order={order} {kw}"
    h = _h0(kind, N) or 1.0 / (N - 1)
    with _solver(pgmg, kind, N, **kw) as s:
        s.set_problem(phi0, None)       # an analytic problem before the call: f is replaced
        s.vcycle(1)                     # (and phi's interior is ignored: it may hold anything)
        ut, vt = _t(u), _t(v)
        info = s.project(ut, vt, order=order, atol=m.atol, measure_after=True, **RULE)
        _compare(pgmg, s, info, u, v, ut, vt, m, N, order, what, h)
        got = s.solution()
        frame = np.concatenate([got[0], got[-1], got[:, 0], got[:, -1]])
        want = np.concatenate([phi0[0], phi0[-1], phi0[:, 0], phi0[:, -1]])
        assert np.array_equal(bits(frame), bits(want)), "the frame changed"
        # the problem is one with a caller's f now
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_ERROR, C.byref(pgmg.PgmgMonitorOut())) == pgmg.PGMG_ERR_STATE
    pgmg.ops.release()


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("N", [9, 17, 33, 129])
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_model(pgmg, kind, N, order):
    _run(pgmg, kind, N, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("kind", ["pq0515", "random"])
def test_bulk_levels_and_cross_fused(pgmg, plan, kind, order):
    """N = 129 with tail_n = 17: bulk levels exist (in the child too); then cross-fused contexts
    (cross_min_n = 9), whose cycles rotate the level-0 grids: phi lies in another grid after the
    solve than before, and the update reads it there."""
    _run(pgmg, kind, 129, order, tail_n=17)
    plan(cross_min_n=9)
    _run(pgmg, kind, 129, order, tail_n=17)
    _run(pgmg, kind, 33, order)


@pytest.mark.parametrize("order", [2, 4])
def test_second_call_and_what_follows(pgmg, oracle_mod, order):
    """A second call on the same context (the half-resolution child, the events and the partials
    are reused) gives the same bits and statistics; measure_after=False leaves div_after NaN; a
    vcycle and a Solver.gradient afterwards continue from the potential and the divergence."""
    import torch
    kind, N = "pq0515", 65
    u, v, phi0 = _problem(kind, N)
    m = _model(kind, N, order)
    h = 1.0 / (N - 1)
    with _solver(pgmg, kind, N) as s:
        s.set_problem(phi0, None)
        outs = []
        for k in range(2):
            ut, vt = _t(u), _t(v)
            info = s.project(ut, vt, order=order, atol=m.atol, measure_after=bool(k), **RULE)
            torch.cuda.synchronize()
            assert np.isnan(info.div_after) == (k == 0)
            outs.append((s.solution(), ut.cpu().numpy(), vt.cpu().numpy(), s.rhs(), s.stats(),
                         info.div_before, info.solve.fine.cycles, info.solve.coarse_sweeps))
        for a, b in zip(outs[0][:4], outs[1][:4]):
            assert_bitwise(a, b, "second call")
        assert outs[0][4:] == outs[1][4:]
        assert_bitwise(outs[1][0], m.phi, "phi against the model")
        assert_bitwise(outs[1][1], m.u, "u against the model")
        gx, gy = s.gradient(order=order, scale=-1.0)
        torch.cuda.synchronize()
        wx, wy = grad_model.gradient(m.phi, h, order, -1.0)
        assert_bitwise(gx.cpu().numpy(), wx, "gradient after the call")
        assert_bitwise(gy.cpu().numpy(), wy, "gradient after the call")
        s.vcycle(1)
        got = s.solution()
        sweeps = s.stats()[0]
    o = oracle_mod.Oracle(eps=-1.0)
    x = np.array(m.phi)
    o.v_cycle(x, np.array(m.f), h)
    assert_bitwise(got, x, "vcycle(1) after the call")
    assert sweeps == m.fine.sweeps + o.sweeps
    pgmg.ops.release()


def test_a_stored_f_after_analytic_cycles(pgmg, oracle_mod):
    """What both routes rely on: a context that ran cycles on the analytic problem (their graph is
    captured with the tables that regenerate f) and is then given a stored f -- by set_problem, or
    by project's divergence -- cycles on the stored f."""
    N = 129
    f, phi0 = np.array(oracle_mod.rhs_mt64(N)), np.zeros((N, N))
    with pgmg.Solver(N) as s:
        s.set_problem(phi0, f)
        s.vcycle(2)
        want = (s.solution(), s.stats())
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        s.set_problem(phi0, f)
        s.vcycle(2)
        assert_bitwise(s.solution(), want[0], "a stored f after analytic cycles")
        assert s.stats() == want[1]
        s.set_problem()                 # ... and back
        s.vcycle(2)
        back = s.solution()
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(2)
        assert_bitwise(back, s.solution(), "the analytic f after a stored one")


def test_by_hand_route_at_1025(pgmg):
    """N = 1025, order 4, no CPU solve: the same bits come from the public entries one by one --
    ops.divergence, a download, set_problem(phi_now, f), solve(order=4), Solver.gradient, u + gx."""
    import torch
    N, order = 1025, 4
    h = 1.0 / (N - 1)
    u, v, _, _, phi0 = proj_model.table_fields(0.5, 1.5, N)
    kw = dict(atol=1e-10 * float(np.linalg.norm(proj_model.divergence(u, v, h, order, -1.0)[1:-1, 1:-1])),
              **RULE)
    with pgmg.Solver(N, eps=-1.0) as s:
        s.set_problem(phi0, None)
        ut, vt = _t(u), _t(v)
        info = s.project(ut, vt, order=order, measure_after=True, **kw)
        torch.cuda.synchronize()
        got = (s.solution(), ut.cpu().numpy(), vt.cpu().numpy(), s.rhs(), s.stats())
        hist = info.history
    with pgmg.Solver(N, eps=-1.0) as s:
        ut, vt = _t(u), _t(v)
        f, n = pgmg.ops.divergence(ut, vt, h, torch.empty_like(ut), order=order, scale=-1.0, norm=True)
        s.set_problem(phi0, f.cpu().numpy())
        hand = s.solve(order=4, damp=0.5, nu=2, **kw)
        gx, gy = s.gradient(order=order, scale=-1.0)
        ut.add_(gx)
        vt.add_(gy)
        torch.cuda.synchronize()
        want = (s.solution(), ut.cpu().numpy(), vt.cpu().numpy(), s.rhs(), s.stats())
        n_after = pgmg.ops.divergence(ut, vt, h, order=order, scale=-1.0, norm=True)[1]
    for a, b, name in zip(got[:4], want[:4], ("phi", "u", "v", "f")):
        assert_bitwise(a, b, name + " by hand")
    assert got[4] == want[4]
    assert [(k, r) for k, r, _ in hist] == [(k, r) for k, r, _ in hand.history]
    assert (info.solve.fine.cycles, info.solve.coarse.cycles, info.solve.coarse_sweeps) == \
        (hand.cycles, hand.coarse.cycles, hand.coarse_sweeps)
    assert info.solve.fine.reason == info.solve.coarse.reason == pgmg.PGMG_STOP_CONVERGED
    assert _same_bits(info.div_before, n) and _same_bits(info.div_after, n_after)
    print(f"N={N}: div_before {info.div_before:.6e} div_after {info.div_after:.6e}, "
          f"{info.solve.fine.cycles} + {info.solve.coarse.cycles} cycles")
    assert info.div_after < 1e-6 * info.div_before
    pgmg.ops.release()


def _call(pgmg, s, u, v, order=4, nu=2, omega=0.5, info=True, opts=True, **fields):
    o, out = pgmg.PgmgSolveOpts(), pgmg.PgmgProjectInfo()
    s.lib.pgmg_solve_opts_default(C.byref(o))
    for k, val in fields.items():
        setattr(o, k, val)
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return s.lib.pgmg_project(s.h, C.byref(o) if opts else None, order, nu, omega, ptr(u), ptr(v), 1,
                              C.byref(out) if info else None)


def test_errors_write_nothing(pgmg):
    import torch
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    rng = np.random.default_rng(5)
    ku, kv = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    ut, vt = _t(ku), _t(kv)
    torch.cuda.synchronize()

    def untouched(s, before, what):
        torch.cuda.synchronize()
        assert_bitwise(ut.cpu().numpy(), ku, what + ": u")
        assert_bitwise(vt.cpu().numpy(), kv, what + ": v")
        if before is not None:
            assert_bitwise(s.solution(), before[0], what + ": phi")
            assert_bitwise(s.rhs(), before[1], what + ": f")
            assert s.stats() == before[2], what

    with pgmg.Solver(N) as s:
        assert _call(pgmg, s, ut, vt) == STATE                     # before set_problem
        untouched(s, None, "before set_problem")
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        assert s.lib.pgmg_project(None, None, 4, 2, 0.5, None, None, 0, None) == ARG
        assert _call(pgmg, s, None, vt) == ARG and _call(pgmg, s, ut, None) == ARG
        assert _call(pgmg, s, ut, vt, info=False) == ARG and _call(pgmg, s, ut, vt, opts=False) == ARG
        assert _call(pgmg, s, ut, vt, check_every=0) == ARG
        for bad in (0, 1, 3, 6):
            assert _call(pgmg, s, ut, vt, order=bad) == ARG, bad
        assert _call(pgmg, s, ut, vt, nu=0) == ARG
        for bad in (0.0, 1.5, -0.5, float("nan"), float("inf")):
            assert _call(pgmg, s, ut, vt, omega=bad) == ARG, bad
        host = np.zeros((N, N))
        assert _call(pgmg, s, host.ctypes.data, vt) == ARG and _call(pgmg, s, ut, host.ctypes.data) == ARG
        assert not host.any()
        assert _call(pgmg, s, ut, ut) == ARG                       # the same array twice
        assert _call(pgmg, s, ut, ut.data_ptr() + 8 * (N * N - 1)) == ARG
        p, pitch, n, es = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        assert s.lib.pgmg_phi_device(s.h, C.byref(p), C.byref(pitch), C.byref(n), C.byref(es)) == 0
        assert _call(pgmg, s, p.value, vt) == ARG                  # a grid of the context
        assert _call(pgmg, s, ut, vt, monitor=pgmg.PGMG_MON_RESIDUAL | pgmg.PGMG_MON_ERROR) == STATE
        untouched(s, before, "refused calls")
        with pytest.raises(ValueError):
            s.project(ut, vt.to(torch.float32))
        with pytest.raises(ValueError):
            s.project(ut[:-1], vt)
        assert _call(pgmg, s, ut, vt) == pgmg.PGMG_OK               # (and the arguments were good)
    ut.copy_(_t(ku))
    vt.copy_(_t(kv))
    for n, kw, order in ((5, {}, 4), (9, dict(n_coarse=3), 2), (17, dict(n_coarse=4), 4), (9, dict(n_coarse=4), 2)):
        a, b = _t(ku[:n, :n]), _t(kv[:n, :n])
        with pgmg.Solver(n, **kw) as s:   # N < 9 at order 4; a coarsest level of 3 points
            s.set_problem()
            before = (s.solution(), s.rhs(), s.stats())
            assert _call(pgmg, s, a, b, order=order) == ARG, (n, kw)
            assert_bitwise(s.rhs(), before[1], "f after a refused call")
            assert_bitwise(a.cpu().numpy(), ku[:n, :n], "u after a refused call")
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        before = (s.solution(), s.rhs(), s.stats())
        assert _call(pgmg, s, ut, vt) == STATE
        untouched(s, before, "fp32")
    with pgmg.Solver(N) as s:             # a device-bound problem: f is the caller's
        g, fd = _t(np.zeros((N, N))), _t(ku)
        s.set_problem_device(g, fd)
        assert _call(pgmg, s, ut, vt) == STATE
        torch.cuda.synchronize()
        assert_bitwise(fd.cpu().numpy(), ku, "the caller's f")
        assert not g.cpu().numpy().any()
        untouched(s, None, "device-bound")


def test_refuses_row_strips(pgmg):
    import torch
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world
    ut, vt = _t(np.ones((N, N))), _t(np.ones((N, N)))
    torch.cuda.synchronize()

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                rc[r] = (_call(pgmg, s, ut, vt), s.stats()[0])
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
    assert np.all(ut.cpu().numpy() == 1.0) and np.all(vt.cpu().numpy() == 1.0)


@pytest.mark.parametrize("order", [2, 4])
def test_project_time(pgmg, order):
    N = 257
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.rhs(), s.stats())
        for which, per_point in ((0, 24.0), (1, 40.0), (0, 24.0)):
            ms, b = s.project_time(which, order=order, reps=3)
            assert ms > 0.0 and b == per_point * N * N, (which, ms, b)
        assert_bitwise(s.solution(), before[0], "phi after project_time")
        assert_bitwise(s.rhs(), before[1], "f after project_time")
        assert s.stats() == before[2]
        assert s.lib.pgmg_project_time(s.h, 2, order, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_project_time(s.h, 0, 3, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_ARG
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem()
        assert s.lib.pgmg_project_time(s.h, 0, order, 3, C.byref(C.c_double()), None) == pgmg.PGMG_ERR_STATE
