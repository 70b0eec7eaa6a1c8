"""GPU: pgmg_damp / pgmg_solve_damped (include/pgmg.h "Damping pass and damped solve") against
their model, tests/damp_model.py (numpy over the CPU oracle).

The pass writes phi in place while its workgroups still read each other's halo rows and edge
columns; the sizes are the smallest that exercise each seam of that scheme: N = 5 (one interior
row pair), 17, 129 (three bands, one tile), 1025 (two column tiles x 17 bands), 2049 (four
tiles).  Every comparison of phi is bitwise, boundary included.
"""
import ctypes as C
import functools
import math
import threading

import numpy as np
import pytest

import damp_model
import solve_rule
from conftest import assert_bitwise, bits
from solve_rule import CONVERGED, MAX_CYCLES, close, norm_tol

pytestmark = pytest.mark.gpu

OMEGAS = (0.5, 1.0, 0.3)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _mt(N, dtype="f64"):
    """(f, phi1): the robustness right-hand side and the oracle's iterate after one V-cycle."""
    import oracle
    o = oracle.Oracle(dtype=dtype)
    f = np.ascontiguousarray(oracle.rhs_mt64(N), dtype=o.dt)
    phi = np.zeros((N, N), dtype=o.dt)
    o.v_cycle(phi, f)
    return _ro(f), _ro(phi)


@functools.lru_cache(maxsize=None)
def _analytic(N, dtype="f64"):
    import oracle
    o = oracle.Oracle(dtype=dtype)
    f = o.rhs(N)
    phi = np.zeros((N, N), dtype=o.dt)
    o.v_cycle(phi, f)
    return _ro(f), _ro(phi)


def _h(N):
    return 1.0 / (N - 1)


def _damp_and_check(s, oracle_mod, phi, f, dtype, what, get=None):
    """From the state phi (already set on s): for each omega, damp on the GPU and in the model,
    compare phi bitwise and the norm with the monitor's (bits) and the oracle's (norm_tol)."""
    N = phi.shape[0]
    get = get or s.solution
    cur = np.array(phi)
    for omega in OMEGAS:
        before = s.monitor().res_norm
        got_norm = s.damp(omega)
        want, want_norm = damp_model.damp(cur, f, _h(N), omega, dtype)
        got = get()
        print(f"{what} omega={omega}: norm {got_norm!r} (oracle {want_norm!r})")
        assert_bitwise(got, want, f"{what} omega={omega}")
        assert got_norm == before, (what, omega, got_norm, before)
        assert close(got_norm, want_norm, N), (what, omega, got_norm, want_norm)
        cur = want
    return cur


@pytest.mark.parametrize("N,dtype", [(5, "f64"), (17, "f64"), (129, "f64"), (1025, "f64"),
                                     (2049, "f64"), (17, "f32"), (129, "f32"), (1025, "f32")])
def test_damp_bitwise_stored_f(pgmg, oracle_mod, N, dtype):
    f, phi1 = _mt(N, dtype)
    with pgmg.Solver(N, dtype=dtype) as s:
        s.set_problem(phi1, f)
        _damp_and_check(s, oracle_mod, phi1, f, dtype, f"mt64 N={N} {dtype}")


@pytest.mark.parametrize("N,flags", [(129, 0), (1025, 0), (1025, "PGMG_FLAG_STORED_RHS")])
def test_damp_bitwise_analytic(pgmg, oracle_mod, N, flags):
    """The regenerated analytic f (kMonGen) and the context's stored copy of it."""
    f, phi1 = _analytic(N)
    with pgmg.Solver(N, flags=getattr(pgmg, flags) if flags else 0) as s:
        s.set_problem(phi1, None)
        _damp_and_check(s, oracle_mod, phi1, f, "f64", f"analytic N={N} {flags}")


def test_damp_nonzero_boundary(pgmg, oracle_mod):
    N = 129
    f, _ = _mt(N)
    rng = np.random.default_rng(11)
    phi0 = rng.standard_normal((N, N))
    with pgmg.Solver(N) as s:
        s.set_problem(phi0, f)
        out = _damp_and_check(s, oracle_mod, phi0, f, "f64", "nonzero boundary")
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert np.array_equal(bits(out[edge]), bits(phi0[edge]))


@pytest.mark.parametrize("N", [129, 1025])
def test_damp_same_state_same_bits(pgmg, N):
    f, phi1 = _mt(N)
    outs = []
    for _ in range(2):
        with pgmg.Solver(N) as s:
            s.set_problem(phi1, f)
            r = s.damp(0.5)
            outs.append((r, s.solution()))
    assert outs[0][0] == outs[1][0]
    assert_bitwise(outs[0][1], outs[1][1], f"two runs N={N}")


@pytest.mark.parametrize("N", [129, 1025])
@pytest.mark.parametrize("inplace", [True, False])
def test_damp_device_bound(pgmg, oracle_mod, plan, N, inplace):
    """The caller's arrays of pgmg_set_problem_device: in place (pgmg_alloc_grid, cross-fused)
    and staged (a plain device allocation); stored f and the analytic one."""
    import torch
    plan(cross_min_n=9)
    f, phi1 = _mt(N)
    fa, phia = _analytic(N)
    for ff, p1, what in ((f, phi1, "mt64"), (None, phia, "analytic")):
        with pgmg.Solver(N) as s:
            if inplace:
                g = pgmg.DeviceGrid(N, np.array(p1))
                fd = pgmg.DeviceGrid(N, np.array(ff)) if ff is not None else None
                get = g.download
            else:
                g = torch.tensor(np.array(p1), dtype=torch.float64, device="cuda")
                fd = (torch.tensor(np.array(ff), dtype=torch.float64, device="cuda")
                      if ff is not None else None)
                torch.cuda.synchronize()
                get = lambda: g.cpu().numpy()
            s.set_problem_device(g, fd)
            assert s.device_info() == (True, inplace)
            _damp_and_check(s, oracle_mod, p1, fa if ff is None else ff, "f64",
                            f"device-bound {what} N={N} inplace={inplace}", get=get)
            if inplace:
                g.close()
                if fd is not None:
                    fd.close()


@pytest.mark.parametrize("N", [129, 1025])
@pytest.mark.parametrize("exact", [False, True])
def test_cycles_after_a_damp_continue_exactly(pgmg, oracle_mod, plan, N, exact):
    """damp, 2 V, damp, 1 W: phi bitwise the oracle's cycles on the model's damped iterates, the
    sweeps equal, and no call after a damp starts from a carry."""
    plan(cross_min_n=9)
    f, phi1 = _mt(N)
    o = oracle_mod.Oracle()
    x, _ = damp_model.damp(phi1, f, _h(N), 0.5)
    for _ in range(2):
        o.v_cycle(x, f)
    x, _ = damp_model.damp(x, f, _h(N), 0.5)
    o.w_cycle(x, f)
    with pgmg.Solver(N, flags=pgmg.PGMG_FLAG_EXACT_DIST if exact else 0) as s:
        s.set_problem(phi1, f)
        s.damp(0.5)
        taken0 = s.carry_info()[0]
        s.vcycle(2)
        assert s.carry_info()[0] == taken0, "the V call after a damp started from a carry"
        s.damp(0.5)
        taken1 = s.carry_info()[0]
        s.wcycle(1)
        assert s.carry_info()[0] == taken1
        assert_bitwise(s.solution(), x, f"damp V V damp W N={N} exact={exact}")
        assert s.stats()[0] == o.sweeps, (s.stats(), o.sweeps)


def test_vcycle_damp_vcycle_drops_the_carry(pgmg, oracle_mod, plan):
    """v(1) makes a carry; the damp in between must drop it (phi changed)."""
    plan(cross_min_n=9)
    N = 257
    o = oracle_mod.Oracle()
    f = o.rhs(N)
    x = np.zeros((N, N))
    o.v_cycle(x, f)
    x, _ = damp_model.damp(x, f, _h(N), 0.5)
    o.v_cycle(x, f)
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(1)
        taken0, made0, _ = s.carry_info()
        s.damp(0.5)
        s.vcycle(1)
        taken1 = s.carry_info()[0]
        assert_bitwise(s.solution(), x, "V damp V")
        assert s.stats()[0] == o.sweeps
    assert made0 >= 1, "the V call before the damp made no carry: the test shows nothing"
    assert taken1 == taken0, "the V-cycle after a damp started from a carried pre-smooth"


SOLVES = [
    ("mt V", dict(N=257, kind="V", mt=True), dict(rtol=1e-6)),
    ("mt W", dict(N=257, kind="W", mt=True), dict(rtol=1e-6)),
    ("mt V every 2", dict(N=257, kind="V", mt=True), dict(rtol=1e-6, check_every=2)),
    ("analytic error", dict(N=129, kind="V", mt=False), dict(rtol=1e-3)),
]


@functools.lru_cache(maxsize=None)
def _solve_model(idx):
    import oracle
    _, p, rule = SOLVES[idx]
    f = oracle.rhs_mt64(p["N"]) if p["mt"] else None
    return damp_model.solve_damped(p["N"], f=f, kind=p["kind"], omega=0.5, error=not p["mt"],
                                   max_cycles=30, **rule)


@pytest.mark.parametrize("idx", range(len(SOLVES)))
def test_solve_damped_against_the_model(pgmg, idx):
    name, p, rule = SOLVES[idx]
    N = p["N"]
    m = _solve_model(idx)
    print(f"{name}: model {m.cycles} cycles, reason {m.reason}, margin {m.margin:.3e}")
    assert m.margin > 100 * norm_tol(N), (name, m.margin)
    with pgmg.Solver(N) as s:
        s.set_problem(None, m.f if p["mt"] else None)
        info = s.solve(cycle=p["kind"], max_cycles=30, damp=0.5, error=not p["mt"], **rule)
        got = s.solution()
        sweeps = s.stats()[0]
    assert (info.cycles, info.reason, info.checks) == (m.cycles, m.reason, m.checks)
    assert len(info.history) == len(m.history)
    for (k, r, e), (mk, mr, me) in zip(info.history, m.history):
        assert k == mk and close(r, mr, N), (name, k, r, mr)
        assert close(e, me, N), (name, k, e, me)
    assert info.res == info.history[-1][1]
    assert_bitwise(got, m.phi, name)
    assert sweeps == m.sweeps


def test_the_point_of_the_feature(pgmg, oracle_mod):
    """mt64 at N = 257, rtol 1e-6, 30 cycles: the plain solve runs out of cycles, the damped one
    converges in the model's count, and the phi it leaves is no worse than it reported."""
    N = 257
    f = oracle_mod.rhs_mt64(N)
    m = _solve_model(0)
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        plain = s.solve(rtol=1e-6, max_cycles=30)
        assert (plain.cycles, plain.reason) == (30, MAX_CYCLES)
        s.set_problem(None, f)
        info = s.solve(rtol=1e-6, max_cycles=30, damp=0.5)
        after = s.monitor().res_norm
    print(f"plain r/r0 {plain.res / plain.res0:.3e}; damped {info.cycles} cycles, "
          f"res {info.res:.6e}, phi left at {after:.6e}")
    assert (info.cycles, info.reason) == (m.cycles, CONVERGED)
    assert after <= info.res * (1 + 1e-9)


def test_errors_enqueue_nothing(pgmg):
    N = 33
    with pgmg.Solver(N) as s:
        o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgSolveInfo()
        s.lib.pgmg_solve_opts_default(C.byref(o))
        assert s.lib.pgmg_damp(s.h, 0.5, None) == pgmg.PGMG_ERR_STATE      # before set_problem
        assert s.lib.pgmg_solve_damped(s.h, C.byref(o), 0.5, C.byref(info)) == pgmg.PGMG_ERR_STATE
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats())
        for bad in (0.0, -0.5, 1.5, math.nan, math.inf):
            assert s.lib.pgmg_damp(s.h, bad, None) == pgmg.PGMG_ERR_ARG, bad
            assert s.lib.pgmg_solve_damped(s.h, C.byref(o), bad, C.byref(info)) == pgmg.PGMG_ERR_ARG, bad
            with pytest.raises(pgmg.PgmgError):
                s.damp_time(bad, reps=1)
        o.check_every = 0
        assert s.lib.pgmg_solve_damped(s.h, C.byref(o), 0.5, C.byref(info)) == pgmg.PGMG_ERR_ARG
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
    f = np.zeros((N, N))
    with pgmg.Solver(N) as s:        # the error norm of a caller's f is not known
        s.set_problem(None, f)
        with pytest.raises(pgmg.PgmgError):
            s.solve(damp=0.5, error=True)


def test_damp_refuses_row_strips(pgmg):
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgSolveInfo()
                s.lib.pgmg_solve_opts_default(C.byref(o))
                rc[r] = (s.lib.pgmg_damp(s.h, 0.5, None),
                         s.lib.pgmg_solve_damped(s.h, C.byref(o), 0.5, C.byref(info)), s.stats()[0])
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
    assert rc == [(pgmg.PGMG_ERR_STATE, pgmg.PGMG_ERR_STATE, 0)] * world, rc


@pytest.mark.parametrize("dtype,es", [("f64", 8), ("f32", 4)])
def test_damp_time_byte_model(pgmg, dtype, es):
    N = 129
    with pgmg.Solver(N, dtype=dtype, flags=pgmg.PGMG_FLAG_STORED_RHS) as s:
        s.set_problem()
        ms, nbytes = s.damp_time(0.5, reps=3)
        _, mon = s.monitor_time(reps=1)
    assert ms > 0.0 and nbytes == mon + es * (N - 2) ** 2, (ms, nbytes, mon)
    assert mon == es * (N * N + (N - 2) ** 2)


def test_solve_without_damp_is_pgmg_solve(pgmg, oracle_mod):
    """damp=0.0 is pgmg_solve: info.cycles plain cycles, bit for bit."""
    N = 129
    h = solve_rule.oracle_history(oracle_mod, "V", N)
    with pgmg.Solver(N) as s:
        s.set_problem()
        info = s.solve(rtol=1e-3, damp=0.0)
        got = s.solution()
        sweeps = s.stats()[0]
    assert info.reason == CONVERGED
    h(0, info.cycles)
    assert_bitwise(got, h.phi(info.cycles), "solve(damp=0.0)")
    assert sweeps == h.sweeps(info.cycles)
