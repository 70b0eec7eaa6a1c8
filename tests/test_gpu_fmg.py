"""GPU: pgmg_fmg (full multigrid for the problem's own right-hand side) against its model.

The model is tests/fmg_model.py: numpy over the CPU oracle (restricted f chain, the coarsest
level from zero, cubic interpolation and nu oracle V-cycles per level).  Every case is bitwise
(assert_bitwise), the sweep count equals the model's, and the early exits are compared the way
tests/test_gpu_fp32.py compares them (the GPU's count is at most the oracle's).
"""
import functools
import threading

import numpy as np
import pytest

import fmg_model
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model_analytic(N, nu=2, eps=1e-7, dtype="f64"):
    u, o = fmg_model.fmg_analytic(N, nu=nu, eps=eps, dtype=dtype)
    u = u.astype(np.float64)
    u.setflags(write=False)
    return u, o.sweeps, o.early_exits


def _model_f(oracle_mod, f, nu=2, eps=1e-7, dtype="f64"):
    o = oracle_mod.Oracle(eps=eps, dtype=dtype)
    u = fmg_model.fmg(o, np.ascontiguousarray(f, dtype=o.dt), nu)
    return u.astype(np.float64), o


def _check_analytic(pgmg, N, nu=2, dtype="f64", **cfg):
    want, sweeps, exits = _model_analytic(N, nu, cfg.get("eps", 1e-7), dtype)
    with pgmg.Solver(N, dtype=dtype, **cfg) as s:
        s.set_problem()
        s.fmg(nu)
        got = s.solution()
        d = s.stats_detail()
    assert_bitwise(got, want, f"fmg N={N} nu={nu} {dtype} {cfg}")
    assert d[0] == sweeps and d[1] <= exits, (N, cfg, d, sweeps, exits)


@pytest.mark.parametrize("N,tail_n,cross", [(5, None, False), (9, 65, False), (33, 9, False),
                                            (129, 17, False), (129, 65, False), (257, None, True),
                                            (513, None, False), (1025, None, False),
                                            (2049, None, False)])
def test_fmg_analytic_bitwise(pgmg, plan, N, tail_n, cross):
    """No climb (5), the tail only (9), two bulk levels (33 / 9), tile levels (513), several
    column blocks of the cubic pass (1025: 513 coarse columns), the default plan (2049)."""
    if cross:
        plan(cross_min_n=9)
    cfg = {} if tail_n is None else {"tail_n": tail_n}
    _check_analytic(pgmg, N, **cfg)


def test_fmg_no_ctile(pgmg):
    _check_analytic(pgmg, 1025, flags=pgmg.PGMG_FLAG_NO_CTILE)


@pytest.mark.parametrize("nu", [1, 3])
def test_fmg_nu(pgmg, nu):
    _check_analytic(pgmg, 129, nu=nu)


@pytest.mark.parametrize("flag", ["PGMG_FLAG_STORED_RHS", "PGMG_FLAG_NO_GRAPH", "PGMG_FLAG_UNFUSED",
                                  "PGMG_FLAG_NO_RECOMPUTE"])
def test_fmg_flags(pgmg, flag):
    _check_analytic(pgmg, 129, flags=getattr(pgmg, flag), tail_n=17)


@pytest.mark.parametrize("N", [33, 129, 1025])
def test_fmg_fp32_bitwise_vs_fp32_model(pgmg, N):
    _check_analytic(pgmg, N, dtype="f32")


@pytest.mark.parametrize("N", [129, 513])
def test_fmg_stored_f_and_a_second_f(pgmg, oracle_mod, N):
    """The caller's f (not the analytic chain pgmg_fcycle swaps in); a second, different f on
    the same context: the restricted chain is rebuilt, not cached stale."""
    f1 = oracle_mod.rhs_mt64(N)
    f2 = oracle_mod.rhs_mt64(N, seed=777)
    assert not np.array_equal(f1, f2)
    with pgmg.Solver(N) as s:
        for f in (f1, f2):
            want, o = _model_f(oracle_mod, f)
            s.set_problem(None, f)
            s.fmg(2)
            assert_bitwise(s.solution(), want, f"stored f N={N}")
            d = s.stats_detail()
            assert d[0] == o.sweeps and d[1] <= o.early_exits, (d, o.sweeps, o.early_exits)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fmg_early_exits_fire(pgmg, oracle_mod, plan, dtype):
    """The random problem of test_fp32_early_exit_rare_paths_bitwise, eps walked down from 1:
    the smoother's early exits fire on the tail levels and the bulk levels' rare paths run,
    still bitwise the model."""
    plan(cross_min_n=9)
    rng = np.random.default_rng(7)
    N = 129
    phi0 = rng.uniform(-1, 1, (N, N))
    f = rng.uniform(-1, 1, (N, N)) * 1e-3
    for a in (phi0, f):
        a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = 0.0
    phi0 = phi0.astype(np.float32).astype(np.float64)   # representable in fp32
    f = f.astype(np.float32).astype(np.float64)
    exits = model_exits = 0
    for k in range(0, -44, -4):
        eps = 10 ** (k / 8.0)
        want, o = _model_f(oracle_mod, f, eps=eps, dtype=dtype)
        with pgmg.Solver(N, dtype=dtype, eps=eps, tail_n=17) as s:
            s.set_problem(phi0, f)   # phi0 is ignored by fmg
            s.fmg(2)
            assert_bitwise(s.solution(), want, f"eps={eps} {dtype}")
            d = s.stats_detail()
        assert d[0] == o.sweeps and d[1] <= o.early_exits, (eps, d, o.sweeps, o.early_exits)
        exits += d[1]
        model_exits += o.early_exits
    assert model_exits > 0 and exits > 0, (exits, model_exits)


def test_fmg_then_vcycles_through_a_graph(pgmg, oracle_mod):
    """fmg(2) then vcycle(3) = the model followed by three oracle V-cycles (N = 513: the
    V-cycles are an eager cycle and a captured graph, captured before and replayed after)."""
    N = 513
    f = oracle_mod.rhs_mt64(N, seed=5)
    o = oracle_mod.Oracle()
    warm = np.zeros((N, N))
    for _ in range(3):
        o.v_cycle(warm, f)
    want = fmg_model.fmg(o, f, 2)
    for _ in range(3):
        o.v_cycle(want, f)
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        s.vcycle(3)          # captures the graph
        s.fmg(2)
        s.vcycle(3)          # replays it from u_0
        assert_bitwise(s.solution(), want, "fmg + 3 V")
        assert s.stats()[0] == o.sweeps


def test_vcycles_fmg_vcycle_drops_the_carry(pgmg, oracle_mod, plan):
    plan(cross_min_n=9)
    N = 257
    o = oracle_mod.Oracle()
    f = o.rhs(N)
    phi = np.zeros((N, N))
    for _ in range(2):
        o.v_cycle(phi, f)
    want = fmg_model.fmg(o, f, 2)
    o.v_cycle(want, f)
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(2)
        taken0, made0, _ = s.carry_info()
        s.fmg(2)
        s.vcycle(1)
        taken1, _, _ = s.carry_info()
        assert_bitwise(s.solution(), want, "V V fmg V")
        assert s.stats()[0] == o.sweeps
    assert made0 >= 1, "the V call before fmg made no carry: the test shows nothing"
    assert taken1 == taken0, "the V-cycle after fmg started from a carried pre-smooth"


def test_fmg_then_solve_history(pgmg):
    """solve after fmg continues from u_0: the history of a plain solve from that phi."""
    N = 257
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.fmg(2)
        u0 = s.solution()
        a = s.solve(rtol=1e-6)
        ha = [h[:2] for h in a.history]   # (cycle, res); rel_error is NaN (not monitored)
    with pgmg.Solver(N) as s:
        s.set_problem(u0, None)
        b = s.solve(rtol=1e-6)
        hb = [h[:2] for h in b.history]
    assert ha == hb and len(ha) >= 2, (ha, hb)
    assert (a.cycles, a.reason) == (b.cycles, b.reason)


@pytest.mark.parametrize("stored", [False, True])
def test_fmg_device_bound(pgmg, oracle_mod, plan, stored):
    plan(cross_min_n=9)
    N = 257
    f = oracle_mod.rhs_mt64(N, seed=99) if stored else None
    if stored:
        want, o = _model_f(oracle_mod, f)
        sweeps = o.sweeps
    else:
        want, sweeps, _ = _model_analytic(N)
    rng = np.random.default_rng(1)
    with pgmg.DeviceGrid(N, rng.standard_normal((N, N))) as phi, pgmg.Solver(N) as s:
        fd = pgmg.DeviceGrid(N, f) if stored else None
        s.set_problem_device(phi, fd)
        s.fmg(2)
        assert_bitwise(phi.download(), want, f"device-bound stored={stored}")
        assert s.stats()[0] == sweeps
        # ... and the bound problem goes on from the caller's array
        o2 = oracle_mod.Oracle()
        nxt = np.array(want)
        o2.v_cycle(nxt, o2.rhs(N) if f is None else f)
        s.vcycle(1)
        assert_bitwise(phi.download(), nxt, "V after a device-bound fmg")
        if fd is not None:
            fd.close()


def test_fmg_errors_enqueue_nothing(pgmg):
    N = 33
    with pgmg.Solver(N) as s:
        assert s.lib.pgmg_fmg(s.h, 2) == pgmg.PGMG_ERR_STATE        # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats())
        assert s.lib.pgmg_fmg(s.h, 0) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_fmg(s.h, -1) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_fmg(None, 2) == pgmg.PGMG_ERR_ARG
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
    with pgmg.Solver(N, n_coarse=3) as s:
        s.set_problem()
        assert s.lib.pgmg_fmg(s.h, 2) == pgmg.PGMG_ERR_ARG
        assert s.stats()[0] == 0
        with pytest.raises(pgmg.PgmgError):
            s.fmg()


@pytest.mark.parametrize("dtype,es", [("f64", 8), ("f32", 4)])
def test_fmg_interp_time(pgmg, dtype, es):
    """The measurement entry: its byte model, and the context still computes the model's fmg
    after it (it overwrites phi only)."""
    N = 129
    want, sweeps, _ = _model_analytic(N, 2, 1e-7, dtype)
    with pgmg.Solver(N, dtype=dtype, tail_n=17) as s:
        s.set_problem()
        ms, nbytes = s.fmg_interp_time(reps=3)
        assert ms > 0.0 and nbytes == es * (129 * 129 + 65 * 65), (ms, nbytes)
        s.set_problem()
        s.fmg(2)
        assert_bitwise(s.solution(), want, f"fmg after fmg_interp_time {dtype}")
        assert s.stats()[0] == sweeps
    with pgmg.Solver(5) as s:       # no level 1 of 5 points per side
        s.set_problem()
        with pytest.raises(pgmg.PgmgError):
            s.fmg_interp_time()


def test_fmg_refuses_row_strips(pgmg):
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                rc[r] = (s.lib.pgmg_fmg(s.h, 2), s.stats()[0])
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


def test_fmg_leaves_f_untouched(pgmg, oracle_mod):
    """After fmg on a stored f the context's residual is ||f - A phi|| of the downloaded phi
    with the caller's f (every lv[l].F is back in place, level 0's was never written)."""
    N = 129
    f = oracle_mod.rhs_mt64(N)
    with pgmg.Solver(N, tail_n=17) as s:
        s.set_problem(None, f)
        s.fmg(2)
        got = s.residual_norm()
        phi = s.solution()
    r = oracle_mod.residual(phi, f, 1.0 / (N - 1))
    r[0, :] = r[-1, :] = r[:, 0] = r[:, -1] = 0.0
    want = float(np.sqrt(np.sum(r * r)))
    assert abs(got - want) <= 1e-12 * max(want, 1e-300), (got, want)
