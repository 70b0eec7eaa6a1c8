"""GPU: pgmg_fmg_damped (full multigrid with a damping pass after every V-cycle of the climb)
against its model, tests/fmg_damped_model.py: numpy over the CPU oracle (fmg_model's restricted f
chain and cubic interpolation, the oracle's V-cycles, damp_model's damp with each level's h).

It mirrors tests/test_gpu_fmg.py: every case is bitwise (assert_bitwise), the sweep count equals
the model's -- the damps add nothing to it -- and the early exits are at most the oracle's.  The
damping pass runs on every level of the climb, so the sizes cover levels of 9 .. 65 points that
otherwise live in the one-workgroup tail, the bulk levels of every plan, and level 0 of a
cross-fused context (where the grids rotate between the cycles).
"""
import functools
import math
import threading

import numpy as np
import pytest

import damp_model
import fmg_damped_model
import fmg_model
from conftest import assert_bitwise
from solve_rule import CONVERGED, close, norm_tol

pytestmark = pytest.mark.gpu

OMEGA = 0.5


@functools.lru_cache(maxsize=None)
def _model_analytic(N, nu=2, dtype="f64", omega=OMEGA):
    u, o = fmg_damped_model.fmg_damped_analytic(N, nu=nu, omega=omega, dtype=dtype)
    u = u.astype(np.float64)
    u.setflags(write=False)
    return u, o.sweeps, o.early_exits


@functools.lru_cache(maxsize=None)
def _model_mt(N, seed=None, nu=2, omega=OMEGA):
    """(f, u_0, sweeps, early exits) of the damped FMG on oracle.rhs_mt64."""
    import oracle
    f = np.array(oracle.rhs_mt64(N) if seed is None else oracle.rhs_mt64(N, seed=seed))
    o = oracle.Oracle()
    u = fmg_damped_model.fmg_damped(o, f, nu, omega)
    for a in (f, u):
        a.setflags(write=False)
    return f, u, o.sweeps, o.early_exits


def _check_analytic(pgmg, N, nu=2, dtype="f64", **cfg):
    want, sweeps, exits = _model_analytic(N, nu, dtype)
    with pgmg.Solver(N, dtype=dtype, **cfg) as s:
        s.set_problem()
        s.fmg(nu, damp=OMEGA)
        got = s.solution()
        d = s.stats_detail()
    assert_bitwise(got, want, f"fmg_damped N={N} nu={nu} {dtype} {cfg}")
    assert d[0] == sweeps and d[1] <= exits, (N, cfg, d, sweeps, exits)


@pytest.mark.parametrize("N,tail_n,cross", [(5, None, False), (9, 65, False), (33, 9, False),
                                            (129, 17, False), (129, 65, False), (257, None, True),
                                            (513, None, False), (1025, None, False)])
def test_fmg_damped_analytic_bitwise(pgmg, plan, N, tail_n, cross):
    """No climb (5: nothing is damped), the tail only (9), bulk levels of 17 .. 65 points
    (33 / 9, 129 / 17), a cross-fused level 0 (257), tile levels (513), two column tiles of the
    damping pass (1025)."""
    if cross:
        plan(cross_min_n=9)
    cfg = {} if tail_n is None else {"tail_n": tail_n}
    _check_analytic(pgmg, N, **cfg)


@pytest.mark.parametrize("nu", [1, 3])
def test_fmg_damped_nu(pgmg, nu):
    _check_analytic(pgmg, 129, nu=nu)


@pytest.mark.parametrize("N", [33, 129, 1025])
def test_fmg_damped_fp32_bitwise_vs_fp32_model(pgmg, N):
    _check_analytic(pgmg, N, dtype="f32")


@pytest.mark.parametrize("flag", ["PGMG_FLAG_STORED_RHS", "PGMG_FLAG_NO_GRAPH", "PGMG_FLAG_UNFUSED",
                                  "PGMG_FLAG_NO_CTILE"])
def test_fmg_damped_flags(pgmg, flag):
    _check_analytic(pgmg, 129, flags=getattr(pgmg, flag), tail_n=17)


@pytest.mark.parametrize("N", [129, 513])
def test_fmg_damped_stored_f(pgmg, oracle_mod, N):
    """The caller's f: bitwise the model, and the GPU result's ||r|| / ||f|| is where the feature
    promises it (2e-3; plain FMG stops at 1e-1)."""
    f, want, sweeps, exits = _model_mt(N)
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        s.fmg(2, damp=OMEGA)
        got = s.solution()
        d = s.stats_detail()
    assert_bitwise(got, want, f"stored f N={N}")
    assert d[0] == sweeps and d[1] <= exits, (d, sweeps, exits)
    rel = fmg_damped_model.rel_residual(got, f, 1.0 / (N - 1))
    print(f"N={N}: ||r|| / ||f|| = {rel:.3e}")
    assert rel <= 2e-3, (N, rel)


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("stored", [False, True])
def test_fmg_damped_device_bound(pgmg, oracle_mod, plan, stored, inplace):
    """pgmg_set_problem_device, in place (pgmg_alloc_grid, cross-fused) and staged (a plain
    device allocation): the climb and its damps run on the context's grids, the result lands in
    the caller's phi, and the bound problem goes on from there."""
    import torch
    plan(cross_min_n=9)
    N = 257
    if stored:
        f, want, sweeps, _ = _model_mt(N, seed=99)
    else:
        f = None
        want, sweeps, _ = _model_analytic(N)
    rng = np.random.default_rng(1)
    phi0 = rng.standard_normal((N, N))
    with pgmg.Solver(N) as s:
        if inplace:
            phi = pgmg.DeviceGrid(N, phi0)
            fd = pgmg.DeviceGrid(N, f) if stored else None
            get = phi.download
        else:
            phi = torch.tensor(phi0, dtype=torch.float64, device="cuda")
            fd = torch.tensor(np.array(f), dtype=torch.float64, device="cuda") if stored else None
            torch.cuda.synchronize()
            get = lambda: phi.cpu().numpy()   # noqa: E731
        s.set_problem_device(phi, fd)
        assert s.device_info() == (True, inplace)
        s.fmg(2, damp=OMEGA)
        assert_bitwise(get(), want, f"device-bound stored={stored} inplace={inplace}")
        assert s.stats()[0] == sweeps
        if stored:
            fgot = fd.download() if inplace else fd.cpu().numpy()
            assert_bitwise(fgot, f, "the caller's f")
        o2 = oracle_mod.Oracle()
        nxt = np.array(want)
        o2.v_cycle(nxt, o2.rhs(N) if f is None else f)
        s.vcycle(1)
        assert_bitwise(get(), nxt, "V after a device-bound damped fmg")
        if inplace:
            phi.close()
            if fd is not None:
                fd.close()


def test_solve_from_damped_fmg_against_the_model(pgmg, oracle_mod):
    """solve(damp, start="fmg"): the FMG model, then damp_model's loop from that iterate.  The
    cycle count, reason, check count, the history's cycle numbers, phi and the sweeps are the
    model's exactly.  The norms are the monitor's sums, which add the oracle's terms in another
    order: they are compared with the model's within solve_rule.close (N^2 2^-52, the bound every
    solve test uses) and, bit for bit, with the library's own damped solve started from the
    model's FMG iterate."""
    N = 129
    f, u0, fmg_sweeps, _ = _model_mt(N)
    m = damp_model.solve_damped(N, f=f, phi0=u0, kind="V", omega=OMEGA, rtol=1e-6, max_cycles=30)
    print(f"model: {m.cycles} cycles after FMG, reason {m.reason}, margin {m.margin:.3e}, "
          f"history {m.history}")
    assert m.reason == CONVERGED and m.margin > 100 * norm_tol(N), (m.reason, m.margin)
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        info = s.solve(rtol=1e-6, max_cycles=30, damp=OMEGA, start="fmg", nu=2)
        got = s.solution()
        sweeps = s.stats()[0]
    assert (info.cycles, info.reason, info.checks) == (m.cycles, CONVERGED, m.checks)
    assert [h[0] for h in info.history] == [h[0] for h in m.history]
    for (k, r, _), (_, mr, _) in zip(info.history, m.history):
        assert close(r, mr, N), (k, r, mr)
    assert_bitwise(got, m.phi, "solve from the damped FMG iterate")
    assert sweeps == fmg_sweeps + m.sweeps, (sweeps, fmg_sweeps, m.sweeps)
    with pgmg.Solver(N) as s:
        s.set_problem(u0, f)
        b = s.solve(rtol=1e-6, max_cycles=30, damp=OMEGA)
    assert [h[:2] for h in info.history] == [h[:2] for h in b.history]
    # To ONE absolute target, 1e-6 x the residual of phi = 0 (with start="fmg" rtol is relative
    # to the FMG iterate, whose residual is already ~1e-3 of that): the model's counts are 12
    # cycles from zero and 5 after the damped FMG.
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        zero = s.solve(rtol=1e-6, max_cycles=30, damp=OMEGA)
        s.set_problem(None, f)
        after = s.solve(rtol=0.0, atol=1e-6 * zero.res0, max_cycles=30, damp=OMEGA, start="fmg")
    mz = damp_model.solve_damped(N, f=f, kind="V", omega=OMEGA, rtol=1e-6, max_cycles=30)
    ma = damp_model.solve_damped(N, f=f, phi0=u0, kind="V", omega=OMEGA, rtol=0.0,
                                 atol=1e-6 * mz.history[0][1], max_cycles=30)
    print(f"to 1e-6 ||r(0)||: {zero.cycles} damped cycles from zero, {after.cycles} after the "
          f"damped FMG (model {mz.cycles}, {ma.cycles})")
    assert min(mz.margin, ma.margin) > 100 * norm_tol(N)
    assert (zero.cycles, zero.reason) == (mz.cycles, CONVERGED)
    assert (after.cycles, after.reason) == (ma.cycles, CONVERGED)
    assert after.cycles < zero.cycles


@pytest.mark.parametrize("N,cfg", [(129, {"tail_n": 17}), (513, {})])
def test_plain_fmg_is_what_it_was(pgmg, N, cfg):
    """pgmg_fmg after the change: bitwise fmg_model, before and after a damped call on the same
    context (the side buffer, the one-cycle calls and the grid rotation leave nothing behind)."""
    u, o = fmg_model.fmg_analytic(N, nu=2)
    want_d, sweeps_d, _ = _model_analytic(N)
    with pgmg.Solver(N, **cfg) as s:
        s.set_problem()
        s.fmg(2)
        assert_bitwise(s.solution(), u, f"plain fmg N={N}")
        assert s.stats()[0] == o.sweeps
        s.fmg(2, damp=OMEGA)
        assert_bitwise(s.solution(), want_d, f"damped fmg after plain N={N}")
        s.fmg(2)
        assert_bitwise(s.solution(), u, f"plain fmg after damped N={N}")
        assert s.stats()[0] == 2 * o.sweeps + sweeps_d


def test_fmg_damped_errors_enqueue_nothing(pgmg):
    N = 33
    with pgmg.Solver(N) as s:
        assert s.lib.pgmg_fmg_damped(s.h, 2, OMEGA) == pgmg.PGMG_ERR_STATE   # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats())
        for bad in (0.0, -0.5, 1.5, math.nan, math.inf):
            assert s.lib.pgmg_fmg_damped(s.h, 2, bad) == pgmg.PGMG_ERR_ARG, bad
            with pytest.raises(pgmg.PgmgError):
                s.fmg(2, damp=bad)
        assert s.lib.pgmg_fmg_damped(s.h, 0, OMEGA) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_fmg_damped(s.h, -1, OMEGA) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_fmg_damped(None, 2, OMEGA) == pgmg.PGMG_ERR_ARG
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
        with pytest.raises(ValueError):
            s.solve(start="zero")
    with pgmg.Solver(N, n_coarse=3) as s:
        s.set_problem()
        assert s.lib.pgmg_fmg_damped(s.h, 2, OMEGA) == pgmg.PGMG_ERR_ARG
        assert s.stats()[0] == 0
        with pytest.raises(pgmg.PgmgError):
            s.fmg(damp=OMEGA)


def test_fmg_damped_refuses_row_strips(pgmg):
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                rc[r] = (s.lib.pgmg_fmg_damped(s.h, 2, OMEGA), s.stats()[0])
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


def test_fmg_damped_leaves_f_untouched(pgmg, oracle_mod):
    """After the call the context's residual is ||f - A phi|| of the downloaded phi with the
    caller's f: every lv[l].F is back in place and level 0's was never written."""
    N = 129
    f = oracle_mod.rhs_mt64(N)
    with pgmg.Solver(N, tail_n=17) as s:
        s.set_problem(None, f)
        s.fmg(2, damp=OMEGA)
        got = s.residual_norm()
        phi = s.solution()
    r = oracle_mod.residual(phi, f, 1.0 / (N - 1))
    r[0, :] = r[-1, :] = r[:, 0] = r[:, -1] = 0.0
    want = float(np.sqrt(np.sum(r * r)))
    assert abs(got - want) <= 1e-12 * max(want, 1e-300), (got, want)


def test_vcycles_fmg_damped_vcycle_drops_the_carry(pgmg, oracle_mod, plan):
    plan(cross_min_n=9)
    N = 257
    o = oracle_mod.Oracle()
    f = o.rhs(N)
    phi = np.zeros((N, N))
    for _ in range(2):
        o.v_cycle(phi, f)
    want = fmg_damped_model.fmg_damped(o, f, 2, OMEGA)
    o.v_cycle(want, f)
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(2)
        taken0, made0, _ = s.carry_info()
        s.fmg(2, damp=OMEGA)
        s.vcycle(1)
        taken1, _, _ = s.carry_info()
        assert_bitwise(s.solution(), want, "V V fmg_damped V")
        assert s.stats()[0] == o.sweeps
    assert made0 >= 1, "the V call before fmg made no carry: the test shows nothing"
    assert taken1 == taken0, "the V-cycle after the damped fmg started from a carried pre-smooth"
