"""GPU: pgmg_fmg_bc (full multigrid that keeps phi's Dirichlet frame) against its model,
tests/fmg_bc_model.py: fmg_model's restricted f chain and cubic interpolation, the oracle's
V-cycles, damp_model's damp, and the frame of phi0 injected into every level.

It mirrors tests/test_gpu_fmg.py and tests/test_gpu_fmg_damped.py: every comparison of phi is
bitwise (assert_bitwise), the sweep count equals the model's and the early exits are at most the
oracle's.  The path cases start from a phi0 that is random on the interior AND on the frame: the
interior must not matter, every bit of the frame must come back, and a bulk level l >= 1 runs as
the top of a cycle with a non-zero frame, which no other entry does.
"""
import functools
import math
import threading

import numpy as np
import pytest

import fmg_bc_model
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

OMEGA = 0.5


def _phi0(N, seed, dtype="f64"):
    phi0 = np.random.default_rng(seed).uniform(-1, 1, (N, N))
    if dtype == "f32":
        phi0 = phi0.astype(np.float32).astype(np.float64)   # representable in fp32
    return phi0


@functools.lru_cache(maxsize=None)
def _case(N, fkind, nu=2, omega=0.0, dtype="f64", seed=None):
    """(phi0, f for set_problem or None, u_0, sweeps, early exits) of the model; fkind "a": the
    analytic f, "m": oracle.rhs_mt64."""
    import oracle
    o = oracle.Oracle(dtype=dtype)
    phi0 = _phi0(N, 100 + N if seed is None else seed, dtype)
    f = o.rhs(N) if fkind == "a" else oracle.rhs_mt64(N, dtype=dtype)
    u = fmg_bc_model.fmg_bc(o, phi0, f, nu, omega).astype(np.float64)
    fset = None if fkind == "a" else f.astype(np.float64)
    for a in (phi0, u, fset):
        if a is not None:
            a.setflags(write=False)
    return phi0, fset, u, o.sweeps, o.early_exits


def _frame_bits(got, phi0, what):
    for name, sl in (("top", np.s_[0, :]), ("bottom", np.s_[-1, :]), ("left", np.s_[:, 0]),
                     ("right", np.s_[:, -1])):
        assert_bitwise(got[sl], phi0[sl], f"{what}: {name} line of the frame")


def _check(pgmg, N, fkind, nu=2, omega=0.0, dtype="f64", **cfg):
    phi0, f, want, sweeps, exits = _case(N, fkind, nu, omega, dtype)
    with pgmg.Solver(N, dtype=dtype, **cfg) as s:
        s.set_problem(phi0, f)
        s.fmg(nu, damp=omega or None, boundary="keep")
        got = s.solution()
        d = s.stats_detail()
    what = f"fmg_bc N={N} f={fkind} nu={nu} omega={omega} {dtype} {cfg}"
    _frame_bits(got, phi0, what)
    assert_bitwise(got, want, what)
    assert d[0] == sweeps and d[1] <= exits, (what, d, sweeps, exits)


PATHS = [(5, None, False, "a"), (9, 65, False, "m"), (33, 9, False, "a"), (129, 17, False, "m"),
         (129, 65, False, "a"), (257, None, True, "m"), (513, None, False, "a"),
         (1025, None, False, "m"), (2049, None, False, "a")]


@pytest.mark.parametrize("N,tail_n,cross,fkind", PATHS)
def test_fmg_bc_paths_bitwise(pgmg, plan, N, tail_n, cross, fkind):
    """No climb (5: the coarsest smoother call from a grid with a non-zero frame), the tail only
    (9), two bulk levels (33 / 9), bulk levels of 33 and 65 points (129), a cross-fused level 0
    whose grids rotate (257), tile levels below the top (513), several column blocks, row-marching
    and tile passes (1025), the default plan (2049)."""
    if cross:
        plan(cross_min_n=9)
    cfg = {} if tail_n is None else {"tail_n": tail_n}
    _check(pgmg, N, fkind, **cfg)


def test_fmg_bc_no_ctile(pgmg):
    _check(pgmg, 1025, "a", flags=pgmg.PGMG_FLAG_NO_CTILE)


@pytest.mark.parametrize("N,tail_n,cross,fkind", [(129, 17, False, "a"), (129, 65, False, "m"),
                                                  (257, None, True, "a"), (1025, None, False, "m")])
def test_fmg_bc_damped_bitwise(pgmg, plan, N, tail_n, cross, fkind):
    if cross:
        plan(cross_min_n=9)
    cfg = {} if tail_n is None else {"tail_n": tail_n}
    _check(pgmg, N, fkind, omega=OMEGA, **cfg)


@pytest.mark.parametrize("nu", [1, 3])
def test_fmg_bc_nu(pgmg, nu):
    _check(pgmg, 129, "a", nu=nu)


@pytest.mark.parametrize("flag", ["PGMG_FLAG_STORED_RHS", "PGMG_FLAG_NO_GRAPH", "PGMG_FLAG_UNFUSED",
                                  "PGMG_FLAG_NO_RECOMPUTE"])
def test_fmg_bc_flags(pgmg, flag):
    _check(pgmg, 129, "a", flags=getattr(pgmg, flag), tail_n=17)


@pytest.mark.parametrize("N,fkind", [(33, "a"), (129, "m"), (1025, "a")])
def test_fmg_bc_fp32_bitwise_vs_fp32_model(pgmg, N, fkind):
    _check(pgmg, N, fkind, dtype="f32")


@pytest.mark.parametrize("omega", [0.0, OMEGA])
def test_zero_frame_is_fmg_on_the_same_context(pgmg, oracle_mod, omega):
    """A frame of +0.0: phi and the statistics are those of pgmg_fmg / pgmg_fmg_damped, before
    and after one another on one context."""
    N = 129
    f = oracle_mod.rhs_mt64(N)
    phi0 = np.array(_phi0(N, 5))
    phi0[0, :] = phi0[-1, :] = phi0[:, 0] = phi0[:, -1] = 0.0
    damp = omega or None
    with pgmg.Solver(N, tail_n=17) as s:
        s.set_problem(phi0, f)
        s.fmg(2, damp=damp)
        want, d0 = s.solution(), s.stats_detail()
        s.set_problem(phi0, f)
        s.fmg(2, damp=damp, boundary="keep")
        got, d1 = s.solution(), s.stats_detail()
        assert_bitwise(got, want, f"zero frame, omega={omega}")
        s.fmg(2, damp=damp)
        assert_bitwise(s.solution(), want, "the zero-boundary entry after the new one")
    assert tuple(d1)[:2] == tuple(d0)[:2], (d0, d1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fmg_bc_early_exits_fire(pgmg, oracle_mod, plan, dtype):
    """The eps walk of test_fmg_early_exits_fire with phi0's frame left in place: the smoother's
    early exits fire on the tail levels and the bulk levels' rare paths run, still bitwise."""
    plan(cross_min_n=9)
    rng = np.random.default_rng(7)
    N = 129
    phi0 = rng.uniform(-1, 1, (N, N))
    f = rng.uniform(-1, 1, (N, N)) * 1e-3
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 0.0
    phi0 = phi0.astype(np.float32).astype(np.float64)   # representable in fp32
    f = f.astype(np.float32).astype(np.float64)
    assert np.abs(phi0[0]).min() > 0 and np.abs(phi0[:, -1]).min() > 0
    exits = model_exits = 0
    for k in range(0, -44, -4):
        eps = 10 ** (k / 8.0)
        o = oracle_mod.Oracle(eps=eps, dtype=dtype)
        want = fmg_bc_model.fmg_bc(o, phi0, f, 2).astype(np.float64)
        with pgmg.Solver(N, dtype=dtype, eps=eps, tail_n=17) as s:
            s.set_problem(phi0, f)
            s.fmg(2, boundary="keep")
            got = s.solution()
            d = s.stats_detail()
        _frame_bits(got, phi0, f"eps={eps} {dtype}")
        assert_bitwise(got, want, f"eps={eps} {dtype}")
        assert d[0] == o.sweeps and d[1] <= o.early_exits, (eps, d, o.sweeps, o.early_exits)
        exits += d[1]
        model_exits += o.early_exits
    assert model_exits > 0 and exits > 0, (exits, model_exits)


def test_fmg_bc_then_vcycles_through_a_graph(pgmg, oracle_mod):
    """vcycle(3) captures the graph, fmg(boundary="keep"), then vcycle(3) replays it from u_0:
    the model followed by three oracle V-cycles (a frame missing from a grid the replayed cycle
    reads would show here)."""
    N = 513
    phi0 = _phi0(N, 21)
    f = oracle_mod.rhs_mt64(N, seed=5)
    o = oracle_mod.Oracle()
    warm = np.array(phi0)
    for _ in range(3):
        o.v_cycle(warm, f)
    want = fmg_bc_model.fmg_bc(o, phi0, f, 2)
    for _ in range(3):
        o.v_cycle(want, f)
    with pgmg.Solver(N) as s:
        s.set_problem(phi0, f)
        s.vcycle(3)
        s.fmg(2, boundary="keep")
        s.vcycle(3)
        got = s.solution()
        assert s.stats()[0] == o.sweeps
    _frame_bits(got, phi0, "fmg_bc + 3 V")
    assert_bitwise(got, want, "fmg_bc + 3 V")


def _exact_frame(o, N):
    return fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))


def test_vcycles_fmg_bc_vcycle_drops_the_carry(pgmg, oracle_mod, plan):
    """Cross-fused level 0 (the grids rotate through A, B and S): V V fmg_bc V on the problem
    with boundary data; the V call before makes a carry, the one after must not take it."""
    plan(cross_min_n=9)
    N = 257
    o = oracle_mod.Oracle(p=0.5, q=0.5)
    f = o.rhs(N)
    phi0 = _exact_frame(o, N)
    phi = np.array(phi0)
    for _ in range(2):
        o.v_cycle(phi, f)
    want = fmg_bc_model.fmg_bc(o, phi, f, 2)
    o.v_cycle(want, f)
    with pgmg.Solver(N, p=0.5, q=0.5) as s:
        s.set_problem(phi0)
        s.vcycle(2)
        taken0, made0, _ = s.carry_info()
        s.fmg(2, boundary="keep")
        s.vcycle(1)
        taken1, _, _ = s.carry_info()
        got = s.solution()
        assert s.stats()[0] == o.sweeps
    _frame_bits(got, phi0, "V V fmg_bc V")
    assert_bitwise(got, want, "V V fmg_bc V")
    assert made0 >= 1, "the V call before fmg_bc made no carry: the test shows nothing"
    assert taken1 == taken0, "the V-cycle after fmg_bc started from a carried pre-smooth"


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("stored", [False, True])
def test_fmg_bc_device_bound(pgmg, oracle_mod, plan, stored, inplace):
    """pgmg_set_problem_device, in place (pgmg_alloc_grid, cross-fused) and staged (a plain device
    allocation): g is the frame of the caller's array, the result lands there with that frame,
    and the bound problem goes on from it."""
    import torch
    plan(cross_min_n=9)
    N = 257
    phi0, f, want, sweeps, _ = _case(N, "m" if stored else "a", seed=31)
    with pgmg.Solver(N) as s:
        if inplace:
            phi = pgmg.DeviceGrid(N, phi0)
            fd = pgmg.DeviceGrid(N, f) if stored else None
            get = phi.download
        else:
            phi = torch.tensor(np.array(phi0), dtype=torch.float64, device="cuda")
            fd = torch.tensor(np.array(f), dtype=torch.float64, device="cuda") if stored else None
            torch.cuda.synchronize()
            get = lambda: phi.cpu().numpy()   # noqa: E731
        s.set_problem_device(phi, fd)
        assert s.device_info() == (True, inplace)
        s.fmg(2, boundary="keep")
        got = get()
        what = f"device-bound stored={stored} inplace={inplace}"
        _frame_bits(got, phi0, what)
        assert_bitwise(got, want, what)
        assert s.stats()[0] == sweeps
        if stored:
            assert_bitwise(fd.download() if inplace else fd.cpu().numpy(), f, "the caller's f")
        o2 = oracle_mod.Oracle()
        nxt = np.array(want)
        o2.v_cycle(nxt, o2.rhs(N) if f is None else f)
        s.vcycle(1)
        assert_bitwise(get(), nxt, "V after a device-bound fmg_bc")
        if inplace:
            phi.close()
            if fd is not None:
                fd.close()


@functools.lru_cache(maxsize=None)
def _disc(N, p, q):
    """The discretisation error: 40 oracle V-cycles from the zero interior with the exact frame."""
    import oracle
    o = oracle.Oracle(p=p, q=q)
    f = o.rhs(N)
    phi = _exact_frame(o, N)
    for _ in range(40):
        o.v_cycle(phi, f)
    return o.rel_error(phi)


def test_fmg_bc_accuracy_on_the_device(pgmg, oracle_mod):
    """p = q = 0.5: the exact solution is not zero on the far boundary.  With its frame in phi0
    the device's FMG iterate is at the discretisation error, by the device's own monitor."""
    N, p, q = 257, 0.5, 0.5
    o = oracle_mod.Oracle(p=p, q=q)
    phi0 = _exact_frame(o, N)
    want = fmg_bc_model.fmg_bc(o, phi0, o.rhs(N), 2)
    want_rel = o.rel_error(want)
    disc = _disc(N, p, q)
    with pgmg.Solver(N, p=p, q=q) as s:
        s.set_problem(phi0)
        s.fmg(2, boundary="keep")
        rel = s.monitor(error=True).rel_error
        got = s.solution()
    print(f"N={N} p={p} q={q}: rel_error {rel!r}, model {want_rel!r}, disc {disc!r}, "
          f"ratio {rel / disc:.4f}")
    assert_bitwise(got, want, "fmg_bc on the p = q = 0.5 problem")
    assert abs(rel - want_rel) <= N * N * 2.0 ** -52 * want_rel, (rel, want_rel)
    assert rel <= disc, (rel, disc)


def test_solve_from_fmg_bc_history(pgmg, oracle_mod):
    """solve(damp, start="fmg", boundary="keep") = fmg(boundary="keep", damp) and then a damped
    solve, on a second context, from the downloaded u_0."""
    N, p, q = 257, 0.5, 0.5
    phi0 = _exact_frame(oracle_mod.Oracle(p=p, q=q), N)
    with pgmg.Solver(N, p=p, q=q) as s:
        s.set_problem(phi0)
        s.fmg(2, damp=OMEGA, boundary="keep")
        u0 = s.solution()
        atol = 1e-2 * s.monitor().res_norm
    _frame_bits(u0, phi0, "u_0")
    with pgmg.Solver(N, p=p, q=q) as s:
        s.set_problem(u0)
        b = s.solve(rtol=0.0, atol=atol, damp=OMEGA)
        hb = [h[:2] for h in b.history]
    with pgmg.Solver(N, p=p, q=q) as s:
        s.set_problem(phi0)
        a = s.solve(rtol=0.0, atol=atol, damp=OMEGA, start="fmg", boundary="keep")
        ha = [h[:2] for h in a.history]
        _frame_bits(s.solution(), phi0, "phi after the solve")
    assert ha == hb and len(ha) >= 2, (ha, hb)
    assert (a.cycles, a.reason) == (b.cycles, b.reason)


def test_fmg_bc_errors_enqueue_nothing(pgmg):
    N = 33
    phi0 = _phi0(N, 3)
    with pgmg.Solver(N) as s:
        assert s.lib.pgmg_fmg_bc(s.h, 2, 0.0) == pgmg.PGMG_ERR_STATE   # before set_problem
        s.set_problem(phi0)
        s.vcycle(1)
        before = (s.solution(), s.stats())
        assert s.lib.pgmg_fmg_bc(s.h, 0, 0.0) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_fmg_bc(s.h, 0, OMEGA) == pgmg.PGMG_ERR_ARG
        for bad in (-0.1, 1.5, math.nan):
            assert s.lib.pgmg_fmg_bc(s.h, 2, bad) == pgmg.PGMG_ERR_ARG, bad
        assert s.lib.pgmg_fmg_bc(None, 2, 0.0) == pgmg.PGMG_ERR_ARG
        with pytest.raises(ValueError):
            s.fmg(boundary="x")
        with pytest.raises(ValueError):
            s.solve(start="fmg", boundary="x")
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
    with pgmg.Solver(N, n_coarse=3) as s:
        s.set_problem(phi0)
        assert s.lib.pgmg_fmg_bc(s.h, 2, 0.0) == pgmg.PGMG_ERR_ARG
        assert s.stats()[0] == 0
        assert_bitwise(s.solution(), phi0, "phi after a refused call (n_coarse = 3)")
        with pytest.raises(pgmg.PgmgError):
            s.fmg(boundary="keep")


def test_fmg_bc_refuses_row_strips(pgmg):
    """Two loopback ranks: PGMG_ERR_STATE on both, nothing run, and the contexts go on cycling."""
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                code, s0 = s.lib.pgmg_fmg_bc(s.h, 2, 0.0), s.stats()[0]
                s.vcycle(1)
                rc[r] = (code, s0, s.stats()[0] > 0)
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
    assert rc == [(pgmg.PGMG_ERR_STATE, 0, True)] * world, rc
