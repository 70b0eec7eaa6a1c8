"""GPU: pgmg_gradient (include/pgmg.h "Gradient of the solution") through Solver.gradient, bitwise
against tests/grad_model.gradient on the phi the context holds (pgmg_get_solution), at the
context's own mesh width.

phi is read where it lies: a level-0 grid that cross-fused cycles have rotated, the grids after
fmg(boundary="keep") and solve(order=4), the caller's bound array, staged and in place.  fp32
contexts compute in fp32 (the model in float32) and store the values widened.  The call only reads:
phi, the statistics, the carry and the speculation state are the same before and after.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import fmg_bc_model
import grad_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

CASES = [(2, 1.0), (4, 1.0), (4, -1.0), (2, 0.37)]


def _h(s):
    return s.cfg.h0 if s.cfg.h0 != 0.0 else s.cfg.a / (s.N - 1)


def _check(pgmg, s, dtype, what, cases=CASES):
    """Solver.gradient against the model on the downloaded phi, every case; the norm against the
    model's and, on an fp64 context, bit for bit against ops.gradient's on the same phi"""
    import torch
    phi = s.solution()
    h, N = _h(s), s.N
    npdt = np.float32 if dtype == "f32" else np.float64
    for order, scale in cases:
        wx, wy = grad_model.gradient(phi, h, order, scale, npdt)
        gx, gy, n = s.gradient(order=order, scale=scale, norm=True)
        w = f"{what} order={order} scale={scale}"
        assert_bitwise(gx.cpu().numpy(), wx, "gx " + w)
        assert_bitwise(gy.cpu().numpy(), wy, "gy " + w)
        wn = grad_model.norm(wx, wy)
        assert abs(n - wn) <= N * N * 2.0 ** -52 * wn, (w, n, wn)
        if dtype == "f64":
            pt = torch.tensor(phi, dtype=torch.float64, device="cuda:0")
            n_op = pgmg.ops.gradient(pt, h, order=order, scale=scale, norm=True)[2]
            assert bits(np.array([n]))[0] == bits(np.array([n_op]))[0], (w, n, n_op)
    assert_bitwise(s.solution(), phi, "phi after the gradients " + what)
    pgmg.ops.release()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [17, 129, 257])
def test_after_cross_fused_cycles(pgmg, plan, N, dtype):
    """Level 0 cross-fused (cross_min_n = 9): three V-cycles rotate the level-0 grids, so phi
    lies in another buffer than the one set_problem filled."""
    plan(cross_min_n=9)
    rng = np.random.default_rng(N)
    with pgmg.Solver(N, dtype=dtype) as s:
        s.set_problem(rng.standard_normal((N, N)), None)
        _check(pgmg, s, dtype, f"fresh N={N} {dtype}", CASES[:2])
        s.vcycle(3)
        _check(pgmg, s, dtype, f"N={N} {dtype}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_after_fmg_keep(pgmg, oracle_mod, dtype):
    N, pq = 129, 0.5
    o = oracle_mod.Oracle(p=pq, q=pq)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    with pgmg.Solver(N, dtype=dtype, p=pq, q=pq) as s:
        s.set_problem(phi0, None)
        s.fmg(nu=2, damp=0.5, boundary="keep")
        _check(pgmg, s, dtype, f"after fmg keep {dtype}")


@pytest.mark.parametrize("cross", [False, True])
def test_after_solve_order_4(pgmg, plan, oracle_mod, cross):
    """The pair the entry exists for: the fourth-order field of the fourth-order solve, bitwise
    the model's on that phi and far closer to the exact field than the second-order pair."""
    if cross:
        plan(cross_min_n=9)
    N, pq = 129, 0.5
    o = oracle_mod.Oracle(p=pq, q=pq)
    f = o.rhs(N)
    phi0 = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N))
    atol = 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))
    t = np.arange(N) / (N - 1)
    ux = pq * np.pi * np.outer(np.sin(pq * np.pi * t), np.cos(pq * np.pi * t))
    uy = pq * np.pi * np.outer(np.cos(pq * np.pi * t), np.sin(pq * np.pi * t))

    def err(gx, gy):
        gx, gy = gx.cpu().numpy(), gy.cpu().numpy()
        return float(np.sqrt(np.sum((gx - ux) ** 2 + (gy - uy) ** 2) / np.sum(ux ** 2 + uy ** 2)))

    with pgmg.Solver(N, eps=-1.0, p=pq, q=pq) as s:
        s.set_problem(phi0, None)
        s.solve(order=2, start="fmg", boundary="keep", damp=0.5, rtol=0.0, atol=atol, max_cycles=40)
        e22 = err(*s.gradient(order=2))
        s.set_problem(phi0, None)
        s.solve(order=4, damp=0.5, rtol=0.0, atol=atol, max_cycles=40)
        _check(pgmg, s, "f64", f"after solve(order=4) cross={cross}")
        e44 = err(*s.gradient(order=4))
    # tests/test_grad_cpu.py's table at N = 129, p = q = 0.5: 2.438e-5 and 2.286e-9
    print(f"field error: second-order pair {e22:.3e}, fourth-order pair {e44:.3e}")
    assert abs(e22 - 2.438e-5) <= 1e-3 * 2.438e-5 and abs(e44 - 2.286e-9) <= 1e-3 * 2.286e-9


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("inplace", [False, True])
def test_device_bound(pgmg, plan, dtype, inplace):
    """The caller's array of pgmg_set_problem_device, staged (a torch tensor) and in place
    (pgmg_alloc_grid on a cross-fused fp64 context): read where it lies, before any cycle (an
    fp32 context converts the caller's doubles on load) and after two."""
    import torch
    if inplace:
        plan(cross_min_n=9)
    N = 129
    phi0 = np.random.default_rng(12).standard_normal((N, N))
    with pgmg.Solver(N, dtype=dtype) as s:
        if inplace:
            g = pgmg.DeviceGrid(N, phi0)
            get = g.download
        else:
            g = torch.tensor(phi0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            get = lambda: g.cpu().numpy()   # noqa: E731
        s.set_problem_device(g, None)
        assert s.device_info() == (True, inplace and dtype == "f64")
        _check(pgmg, s, dtype, f"bound, fresh {dtype} inplace={inplace}", CASES[:2])
        assert_bitwise(get(), phi0, "the caller's phi before any cycle")
        s.vcycle(2)
        _check(pgmg, s, dtype, f"bound {dtype} inplace={inplace}")
        assert_bitwise(get(), s.solution(), "the caller's phi")
        # an output that aliases the bound phi
        gx = torch.empty((N, N), dtype=torch.float64, device="cuda")
        ptr = C.c_void_p(g.ptr if inplace else g.data_ptr())
        before = get()
        assert s.lib.pgmg_gradient(s.h, 4, 1.0, ptr, C.c_void_p(gx.data_ptr()), None) == pgmg.PGMG_ERR_ARG
        assert s.lib.pgmg_gradient(s.h, 4, 1.0, None, C.c_void_p(ptr.value + 8 * N), None) == pgmg.PGMG_ERR_ARG
        assert_bitwise(get(), before, "phi after the refused calls")
        if inplace:
            g.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kw", [dict(a=-2.0), dict(h0=0.7 / 64), dict(flags="stored")], ids=str)
def test_off_the_defaults(pgmg, dtype, kw):
    """a = -2 (a negative mesh width), a caller's h0 and PGMG_FLAG_STORED_RHS."""
    N = 65
    kw = dict(kw)
    if kw.get("flags") == "stored":
        kw["flags"] = pgmg.PGMG_FLAG_STORED_RHS
    with pgmg.Solver(N, dtype=dtype, **kw) as s:
        s.set_problem(np.random.default_rng(3).standard_normal((N, N)), None)
        s.vcycle(1)
        assert _h(s) == (-2.0 / 64 if "a" in kw else 0.7 / 64 if "h0" in kw else 1.0 / 64)
        _check(pgmg, s, dtype, f"{kw} {dtype}")


def test_read_only_and_the_carry(pgmg, plan):
    """phi's hash, stats(), carry_info() and dist_info() are the same before and after; four
    one-cycle V calls with a gradient before each take the carry as often as without (at least
    once) and end bitwise as they do without the calls."""
    plan(cross_min_n=33)
    N = 257
    outs = []
    for with_gradient in (False, True):
        with pgmg.Solver(N) as s:
            s.set_problem()
            for _ in range(4):
                if with_gradient:
                    state = (s.solution_hash(), s.stats(), s.stats_detail(), s.carry_info(),
                             s.dist_info(), s.spec_levels())
                    for order in (2, 4):
                        s.gradient(order=order, norm=True)
                    assert (s.solution_hash(), s.stats(), s.stats_detail(), s.carry_info(),
                            s.dist_info(), s.spec_levels()) == state
                s.vcycle(1)
            outs.append((s.solution(), s.stats(), s.carry_info(), s.dist_info()))
    print("carry (took, made, dropped):", outs[0][2], outs[1][2])
    assert outs[0][2][0] > 0, "no call took a carry: nothing shown"
    assert_bitwise(outs[1][0], outs[0][0], "phi after gradients between the cycles")
    assert outs[1][1:] == outs[0][1:]


def test_outputs_and_one_component(pgmg):
    """Caller-given tensors are written in place; through the C entry one NULL output leaves the
    other component's bits and sums that component alone."""
    import torch
    N = 65
    with pgmg.Solver(N) as s:
        s.set_problem(np.random.default_rng(5).standard_normal((N, N)), None)
        wx, wy = grad_model.gradient(s.solution(), 1.0 / 64, 4, 1.0)
        gx = torch.full((N, N), np.nan, dtype=torch.float64, device="cuda")
        gy = torch.full((N, N), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        a, b = s.gradient(gx=gx, gy=gy)
        assert a is gx and b is gy
        assert_bitwise(gx.cpu().numpy(), wx, "gx")
        assert_bitwise(gy.cpu().numpy(), wy, "gy")
        n = C.c_double()
        gy.fill_(7.0)
        torch.cuda.synchronize()
        assert s.lib.pgmg_gradient(s.h, 4, 1.0, C.c_void_p(gx.data_ptr()), None, C.byref(n)) == 0
        assert_bitwise(gx.cpu().numpy(), wx, "gx alone")
        assert bool((gy == 7.0).all())
        assert abs(n.value - grad_model.norm(wx, None)) <= N * N * 2.0 ** -52 * n.value
        assert s.lib.pgmg_gradient(s.h, 4, 1.0, None, C.c_void_p(gy.data_ptr()), C.byref(n)) == 0
        assert_bitwise(gy.cpu().numpy(), wy, "gy alone")
        assert abs(n.value - grad_model.norm(None, wy)) <= N * N * 2.0 ** -52 * n.value
        with pytest.raises(ValueError):
            s.gradient(gx=torch.empty((N, N), dtype=torch.float32, device="cuda"))


def test_errors_enqueue_nothing(pgmg):
    import torch
    ARG, STATE = pgmg.PGMG_ERR_ARG, pgmg.PGMG_ERR_STATE
    N = 33
    keep = np.random.default_rng(2).standard_normal((N, N))
    gx = torch.tensor(keep, dtype=torch.float64, device="cuda")
    gy = torch.tensor(keep, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    px, py = C.c_void_p(gx.data_ptr()), C.c_void_p(gy.data_ptr())
    n = C.c_double(-7.0)
    with pgmg.Solver(N) as s:
        call = s.lib.pgmg_gradient
        assert call(s.h, 4, 1.0, px, py, C.byref(n)) == STATE          # before set_problem
        s.set_problem()
        s.vcycle(1)
        before = (s.solution(), s.stats())
        assert call(None, 4, 1.0, px, py, C.byref(n)) == ARG
        for bad in (0, 1, 3, 6, -2):
            assert call(s.h, bad, 1.0, px, py, C.byref(n)) == ARG, bad
        for bad in (float("nan"), float("inf")):
            assert call(s.h, 4, bad, px, py, C.byref(n)) == ARG, bad
        assert call(s.h, 4, 1.0, None, None, C.byref(n)) == ARG
        assert call(s.h, 4, 1.0, px, px, C.byref(n)) == ARG
        host = np.zeros((N, N))
        assert call(s.h, 4, 1.0, host.ctypes.data_as(C.c_void_p), py, C.byref(n)) == ARG
        assert s.lib.pgmg_gradient_time(s.h, 3, 5, C.byref(n), None) == ARG
        assert s.lib.pgmg_gradient_time(s.h, 4, 0, C.byref(n), None) == ARG
        with pytest.raises(pgmg.PgmgError):
            s.gradient(order=3)
        assert_bitwise(s.solution(), before[0], "phi after refused calls")
        assert s.stats() == before[1]
    torch.cuda.synchronize()
    assert n.value == -7.0 and not host.any()
    assert_bitwise(gx.cpu().numpy(), keep, "gx after refused calls")
    assert_bitwise(gy.cpu().numpy(), keep, "gy after refused calls")


def test_refuses_row_strips(pgmg):
    import torch
    N, world = 513, 2
    hub = pgmg.LoopbackHub(world)
    rc, err = [None] * world, [None] * world
    outs = [torch.zeros((2, N, N), dtype=torch.float64, device="cuda") for _ in range(world)]
    torch.cuda.synchronize()

    def work(r):
        try:
            with pgmg.Solver(N, hub=hub, rank=r, gather_n=65) as s:
                s.set_problem()
                ms = C.c_double()
                rc[r] = (s.lib.pgmg_gradient(s.h, 4, 1.0, C.c_void_p(outs[r][0].data_ptr()),
                                             C.c_void_p(outs[r][1].data_ptr()), None),
                         s.lib.pgmg_gradient_time(s.h, 4, 3, C.byref(ms), None), s.stats()[0])
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
    assert not any(bool(o.any()) for o in outs), "a refused call wrote its outputs"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gradient_time(pgmg, dtype):
    N = 257
    with pgmg.Solver(N, dtype=dtype) as s:
        s.set_problem()
        s.vcycle(1)
        before = s.solution_hash()
        for order in (2, 4):
            ms, nbytes = s.gradient_time(order=order, reps=5)
            print(f"{dtype} order {order}: {ms:.4f} ms, {nbytes:.0f} B")
            assert np.isfinite(ms) and ms > 0.0
            assert nbytes == N * N * (s.elem_bytes + 16)
        assert s.solution_hash() == before
