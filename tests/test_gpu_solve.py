"""GPU: pgmg_solve, cycle until the residual meets a tolerance (include/pgmg.h
"Convergence monitor and solve-to-tolerance").

The reference's driver runs a fixed number of cycles and prints the norm after each
(MultigridTestRunner::run_cycle, 2_part_MG/MultiGridTestRunner.hpp:190-244); pgmg_solve turns
that history into a stop rule.  Every test computes the expected stop cycle, reason and history
from the oracle with the Python restatement of the rule (tests/solve_rule.py, pinned to the C
header by tests/test_solve_cpu.py), requires that every comparison the rule made has a relative
margin >= 1e-6 (so the N^2 2^-52 difference between two summation orders cannot change a
decision), and then requires of pgmg_solve: the same stop, every record within N^2 2^-52 of the
oracle's norm, and phi and the statistics bit for bit those of info.cycles plain cycles on a
fresh context (the monitor adds no sweep and writes nothing a cycle reads).
"""
import math
import threading

import numpy as np
import pytest

from conftest import assert_bitwise
import solve_rule
from solve_rule import CONVERGED, MAX_CYCLES, STALLED, NONFINITE, close

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-6


def _plain(pgmg, N, kind, cycles, f=None, dtype="f64", **cfg):
    """a fresh context running `cycles` plain cycles, one call"""
    with pgmg.Solver(N, dtype=dtype, **cfg) as s:
        s.set_problem(None, f)
        if cycles:
            {"V": s.vcycle, "W": s.wcycle, "F": s.fcycle}[kind](cycles)
        return s.solution(), s.stats()


def _solve_case(pgmg, oracle_mod, N, kind, opts, f=None, dtype="f64", error=False, **cfg):
    h = solve_rule.oracle_history(oracle_mod, kind, N, f=f, dtype=dtype)
    cycles, reason, recs, margin = solve_rule.simulate(h, **opts)
    print(f"oracle: N={N} {kind} {opts}: {cycles} cycles, {solve_rule.REASON[reason]}, "
          f"margin {margin:.3e}, history {[r for _, r in recs]}")
    assert margin >= MIN_MARGIN, margin      # a condition on the case, not a measurement
    fa = None if f is None else np.asarray(f, dtype=np.float64)
    with pgmg.Solver(N, dtype=dtype, **cfg) as s:
        s.set_problem(None, fa)
        info = s.solve(cycle=kind, error=error, **opts)
        phi, stats = s.solution(), s.stats()
        carry = s.carry_info()
    print(f"solve: {info.cycles} cycles, reason {info.reason}, {info.checks} checks, "
          f"history {info.history}")
    assert (info.cycles, info.reason) == (cycles, reason)
    assert info.checks == len(recs) == len(info.history)
    assert [k for k, _, _ in info.history] == [k for k, _ in recs]
    for (k, got, rel), (_, want) in zip(info.history, recs):
        assert close(got, want, N), (k, got, want)
        if error:
            assert close(rel, h.oracle.rel_error(h.phi(k)), N), (k, rel)
        else:
            assert math.isnan(rel)
    assert info.res0 == info.history[0][1] and info.res == info.history[-1][1]
    assert info.elapsed_ms > 0
    # the invariant: phi and the statistics are those of info.cycles plain cycles
    want_phi, want_stats = _plain(pgmg, N, kind, info.cycles, fa, dtype, **cfg)
    assert_bitwise(phi, want_phi, f"solve vs {info.cycles} plain {kind}")
    assert stats == want_stats, (stats, want_stats)
    return info, h, phi, stats, carry


@pytest.mark.parametrize("cross", [False, True])
def test_solve_v129_converges_in_8(pgmg, oracle_mod, golden_cycles, cross):
    N = 129
    cfg = dict(cross_min_n=9) if cross else {}
    info, h, phi, stats, _ = _solve_case(pgmg, oracle_mod, N, "V", dict(rtol=1e-2), error=True,
                                         **cfg)
    assert (info.cycles, info.reason, len(info.history)) == (8, CONVERGED, 9)
    assert_bitwise(phi, h.phi(8), "solve vs oracle")
    assert stats[0] == h.sweeps(8)
    hit = 0
    for c in golden_cycles:
        if c["kind"] == "V" and c["N"] == N and c["eps"] == 1e-7 and len(c["cycles"]) >= 8:
            assert oracle_mod.fnv_hash(phi) == c["cycles"][7]["hash"]
            assert stats[0] == c["cycles"][7]["sweeps"]
            hit += 1
    print("golden fixtures matched:", hit)


@pytest.mark.parametrize("cross", [False, True])
def test_solve_check_every_3(pgmg, oracle_mod, cross):
    cfg = dict(cross_min_n=9) if cross else {}
    info, *_ = _solve_case(pgmg, oracle_mod, 129, "V",
                           dict(rtol=1e-2, check_every=3, max_cycles=10), **cfg)
    assert (info.cycles, info.reason) == (9, CONVERGED)
    info, *_ = _solve_case(pgmg, oracle_mod, 129, "V",
                           dict(rtol=1e-6, check_every=3, max_cycles=4), **cfg)
    assert (info.cycles, info.reason) == (4, MAX_CYCLES)
    assert [k for k, _, _ in info.history] == [0, 3, 4]        # chunks 3 + 1


def test_solve_w513(pgmg, oracle_mod):
    info, *_ = _solve_case(pgmg, oracle_mod, 513, "W", dict(rtol=1e-2))
    assert (info.cycles, info.reason) == (5, CONVERGED)


def test_solve_f129_stalls(pgmg, oracle_mod):
    info, *_ = _solve_case(pgmg, oracle_mod, 129, "F",
                           dict(rtol=1e-3, stall_ratio=0.99, stall_checks=2))
    assert (info.cycles, info.reason) == (3, STALLED)


def test_solve_mt64_stalls(pgmg, oracle_mod):
    f = oracle_mod.rhs_mt64(129)
    info, *_ = _solve_case(pgmg, oracle_mod, 129, "V",
                           dict(rtol=1e-3, stall_ratio=0.9, stall_checks=2, max_cycles=14), f=f)
    assert (info.cycles, info.reason) == (7, STALLED)


def test_solve_zero_rhs_and_nan_rhs(pgmg, oracle_mod):
    N = 129
    f = np.zeros((N, N))
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        info = s.solve()
        assert (info.cycles, info.reason, info.checks) == (0, CONVERGED, 1)
        assert info.res0 == 0.0 and info.history == [(0, 0.0, info.history[0][2])]
        assert s.stats() == (0, 0)
        f[40, 50] = np.nan
        s.set_problem(None, f)
        info = s.solve()
        assert (info.cycles, info.reason, info.checks) == (0, NONFINITE, 1)
        assert math.isnan(info.res) and math.isnan(info.res0)
        assert s.stats() == (0, 0)


def test_solve_fp32(pgmg, oracle_mod):
    info, h, phi, *_ = _solve_case(pgmg, oracle_mod, 257, "V", dict(rtol=1e-2), dtype="f32",
                                   error=True)
    assert info.reason == CONVERGED
    assert_bitwise(phi, h.phi(info.cycles).astype(np.float64), "fp32 solve vs fp32 oracle")


def test_solve_device_bound_in_place(pgmg, oracle_mod, plan):
    """The caller's array after a solve on it is bitwise the context-owned solve's phi and the
    histories are bitwise equal (the monitor reads the bound array where it lies)."""
    N = 513
    plan(cross_min_n=9)
    opts = dict(rtol=1e-2)
    info, h, phi, stats, _ = _solve_case(pgmg, oracle_mod, N, "V", opts, error=True)
    with pgmg.DeviceGrid(N) as g, pgmg.Solver(N) as s:
        s.set_problem_device(g)
        assert s.device_info() == (True, True)
        got = s.solve(cycle="V", error=True, **opts)
        assert (got.cycles, got.reason) == (info.cycles, info.reason)
        assert_bitwise(g.download(), phi, "bound in place vs context-owned")
        assert s.stats() == stats
        a = np.array(got.history, dtype=np.float64)
        b = np.array(info.history, dtype=np.float64)
        assert (a.view(np.uint64) == b.view(np.uint64)).all(), (got.history, info.history)


def test_solve_check_every_1_runs_on_the_carry(pgmg, oracle_mod, plan):
    plan(cross_min_n=9)
    info, _, _, _, (took, made, dropped) = _solve_case(pgmg, oracle_mod, 513, "V", dict(rtol=1e-2))
    print("carry_info", took, made, dropped, "cycles", info.cycles)
    assert took + dropped == info.cycles - 1 and took >= 1, (took, made, dropped)


def test_solve_invalid_options(pgmg):
    import ctypes as C
    with pgmg.Solver(129) as s:
        s.set_problem()
        for bad in (dict(max_cycles=-1), dict(check_every=0), dict(stall_checks=0),
                    dict(rtol=-1e-3), dict(atol=float("nan")), dict(rtol=float("inf")),
                    dict(cycle=7)):
            with pytest.raises(pgmg.PgmgError):
                s.solve(**bad)
        o, info = pgmg.PgmgSolveOpts(), pgmg.PgmgSolveInfo()
        s.lib.pgmg_solve_opts_default(C.byref(o))
        o.monitor = 8
        assert s.lib.pgmg_solve(s.h, C.byref(o), C.byref(info)) == -1      # PGMG_ERR_ARG
        assert s.stats() == (0, 0)                                         # nothing ran
        s.set_problem(None, np.ones((129, 129)))
        o.monitor = pgmg.PGMG_MON_ERROR
        assert s.lib.pgmg_solve(s.h, C.byref(o), C.byref(info)) == -5      # PGMG_ERR_STATE
        with pytest.raises(pgmg.PgmgError):
            s.solve(error=True)


@pytest.mark.parametrize("world,gather_n", [(2, 65), (3, 129)])
def test_solve_on_loopback_strips(pgmg, oracle_mod, world, gather_n):
    """Row strips: one halo exchange and one rank-ordered allreduce per check give every rank
    identical norms, so every rank stops at the same check; phi is bitwise the one-GPU solve."""
    N = 1025
    opts = dict(rtol=1e-1)
    h = solve_rule.oracle_history(oracle_mod, "V", N)
    cycles, reason, recs, margin = solve_rule.simulate(h, **opts)
    print(f"oracle: {cycles} cycles, margin {margin:.3e}, {[r for _, r in recs]}")
    assert margin >= MIN_MARGIN
    assert (cycles, reason) == (8, CONVERGED)
    with pgmg.Solver(N) as s:
        s.set_problem()
        one = s.solve(cycle="V", error=True, **opts)
        one_phi, one_stats = s.solution(), s.stats()
    assert (one.cycles, one.reason) == (cycles, reason)
    hub = pgmg.LoopbackHub(world)
    out, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=gather_n) as s:
                s.set_problem()
                info = s.solve(cycle="V", error=True, **opts)
                out[r] = (info, s.solution(), s.stats())
        except Exception as e:  # surfaced below
            err[r] = e

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    hub.close()
    for e in err:
        if e is not None:
            raise e
    first = np.array(out[0][0].history, dtype=np.float64).view(np.uint64)
    for r, (info, phi, stats) in enumerate(out):
        assert (info.cycles, info.reason, info.checks) == (cycles, reason, len(recs)), r
        mine = np.array(info.history, dtype=np.float64).view(np.uint64)
        assert (mine == first).all(), f"rank {r}: another history than rank 0"
        for (k, got, rel), (_, want), (_, _, rel1) in zip(info.history, recs, one.history):
            assert close(got, want, N), (r, k, got, want)
            assert close(rel, rel1, N), (r, k, rel, rel1)
        assert_bitwise(phi, one_phi, f"rank {r} of {world} vs one GPU")
    assert out[0][2][0] == one_stats[0]
