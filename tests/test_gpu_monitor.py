"""GPU: pgmg_monitor, the on-device convergence monitor (csrc/pgmg_monitor.hip).

The reference's driver measures convergence after every cycle: MultigridTestRunner::run_cycle
(2_part_MG/MultiGridTestRunner.hpp:190-244) computes compute_residual + norm
(DynamicGridUtils.hpp:59-69, :21-27), and with flag_err_norm_iteration the relative error
||phi - u|| / ||u|| over all L = N*N points (:110-122, :252-254).  The oracle restates both
(orc_residual_norm, orc_rel_error, orc_exact).  The monitor's per-point terms are the oracle's
(the same expression order, evaluated in the context's element type, squared and summed in
double); only the summation order differs, and two orders of n non-negative terms differ by at
most (n - 1) 2^-52 relative, so every norm must agree within N^2 2^-52 relative
(solve_rule.norm_tol).

The kernel's decomposition: tiles of TILE = 512 columns (a column pair per lane, 256 lanes)
starting at column 1, bands of BAND = 64 rows.  N = 5, 33: below one tile and one band (33 is
a tail-only context, 5 a one-level one); 129: one tile, three bands with a ragged last one;
513, 1025: one and two full tiles, 9 and 17 bands; 2049: four tiles -- with 4-wave workgroups
the first size where more than two tiles, and so a tile strictly inside the row, exist.
"""
import math

import numpy as np
import pytest

from conftest import assert_bitwise
import solve_rule
from solve_rule import close, oracle_res_norm

pytestmark = pytest.mark.gpu

TILE, BAND = 512, 64
SIZES = [5, 33, 129, 513, 1025, 2049]


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same(a, b):
    """two PgmgMonitorOut with equal bits in every field"""
    return all(_bits(getattr(a, k)) == _bits(getattr(b, k))
               for k in ("res_norm", "err_norm", "exact_norm", "rel_error"))


def _check(s, oracle_mod, o, f, dtype, N, analytic, what):
    """monitor() of the solver's current iterate against the oracle's norms of that iterate"""
    phi = s.solution()
    want_res = oracle_res_norm(oracle_mod, phi, f, dtype, o.c.a / (N - 1))
    m = s.monitor()
    print(f"{what}: res {m.res_norm!r} oracle {want_res!r}")
    assert close(m.res_norm, want_res, N), (what, m.res_norm, want_res)
    assert math.isnan(m.err_norm) and math.isnan(m.rel_error) and math.isnan(m.exact_norm)
    if not analytic:
        return
    want_rel = o.rel_error(phi)
    want_u = oracle_mod.norm(o.exact(N))
    me = s.monitor(error=True)
    print(f"{what}: rel {me.rel_error!r} oracle {want_rel!r}; |u| {me.exact_norm!r} {want_u!r}")
    assert close(me.rel_error, want_rel, N), (what, me.rel_error, want_rel)
    assert close(me.exact_norm, want_u, N), (what, me.exact_norm, want_u)
    assert close(me.err_norm, want_rel * want_u, 2 * N), (what, me.err_norm)
    # the decomposition does not depend on the sums asked for: the same bits either way
    assert _bits(me.res_norm) == _bits(m.res_norm), what
    eo = s.monitor(error=True, residual=False)
    assert _bits(eo.rel_error) == _bits(me.rel_error) and math.isnan(eo.res_norm), what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", SIZES)
def test_monitor_against_oracle(pgmg, oracle_mod, N, dtype):
    """zero phi, after 1 and 3 V-cycles, and a random phi0 with a non-zero boundary; analytic f
    regenerated, analytic f stored (PGMG_FLAG_STORED_RHS) and the rhs_mt64 robustness RHS."""
    o = oracle_mod.Oracle(dtype=dtype)
    rng = np.random.default_rng(1000 + N)
    phi0 = rng.uniform(-1.0, 1.0, (N, N)).astype(o.dt).astype(np.float64)
    assert np.abs(phi0[0]).min() > 0 and np.abs(phi0[:, -1]).min() > 0    # boundary included
    for fkind in ("analytic", "stored", "mt64"):
        analytic = fkind != "mt64"
        f = o.rhs(N) if analytic else oracle_mod.rhs_mt64(N, dtype=dtype)
        flags = pgmg.PGMG_FLAG_STORED_RHS if fkind == "stored" else 0
        with pgmg.Solver(N, dtype=dtype, flags=flags) as s:
            fa = None if analytic else f.astype(np.float64)
            s.set_problem(None, fa)
            _check(s, oracle_mod, o, f, dtype, N, analytic, f"N={N} {dtype} {fkind} zero")
            s.vcycle(1)
            _check(s, oracle_mod, o, f, dtype, N, analytic, f"N={N} {dtype} {fkind} V1")
            s.vcycle(2)
            _check(s, oracle_mod, o, f, dtype, N, analytic, f"N={N} {dtype} {fkind} V3")
            s.set_problem(phi0, fa)
            _check(s, oracle_mod, o, f, dtype, N, analytic, f"N={N} {dtype} {fkind} random")


def test_monitor_other_wave_numbers(pgmg, oracle_mod):
    """p = 2, q = 3: the exact solution's tables follow the context's wave numbers."""
    N = 129
    o = oracle_mod.Oracle(p=2.0, q=3.0)
    f = o.rhs(N)
    with pgmg.Solver(N, p=2.0, q=3.0) as s:
        s.set_problem()
        _check(s, oracle_mod, o, f, "f64", N, True, "p2q3 zero")
        s.vcycle(2)
        _check(s, oracle_mod, o, f, "f64", N, True, "p2q3 V2")


def test_monitor_is_deterministic_across_plans_and_bindings(pgmg, oracle_mod, plan):
    """Two calls give equal bits; so do eager launches (PGMG_FLAG_NO_GRAPH) against the
    default, and the same problem context-owned, bound in place (DeviceGrid) and bound through
    a plain torch device tensor (staged): the decomposition depends on N only, not on pitch,
    address or which array is bound."""
    import torch
    N = 513
    plan(cross_min_n=9)
    outs = {}
    with pgmg.Solver(N) as s:
        s.set_problem()
        s.vcycle(2)
        a, b = s.monitor(error=True), s.monitor(error=True)
        assert _same(a, b)
        outs["own"] = a
        want = s.solution()
    with pgmg.Solver(N, flags=pgmg.PGMG_FLAG_NO_GRAPH) as s:
        s.set_problem()
        s.vcycle(2)
        outs["eager"] = s.monitor(error=True)
    with pgmg.DeviceGrid(N) as g, pgmg.Solver(N) as s:
        s.set_problem_device(g)
        assert s.device_info() == (True, True)
        s.vcycle(2)
        outs["inplace"] = s.monitor(error=True)
        assert_bitwise(g.download(), want, "in place")
    t = torch.zeros((N, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pgmg.Solver(N) as s:
        s.set_problem_device(t)
        assert s.device_info() == (True, False)
        s.vcycle(2)
        outs["staged"] = s.monitor(error=True)
        assert_bitwise(t.cpu().numpy(), want, "staged")
    # a caller's f bound on the device is read in place too
    f = oracle_mod.rhs_mt64(N)
    with pgmg.Solver(N) as s:
        s.set_problem(None, f)
        s.vcycle(2)
        r_own = s.monitor().res_norm
    ft = torch.from_numpy(f).cuda()
    t.zero_()
    torch.cuda.synchronize()
    with pgmg.Solver(N) as s:
        s.set_problem_device(t, ft)
        s.vcycle(2)
        assert _bits(s.monitor().res_norm) == _bits(r_own)
    for k, v in outs.items():
        assert _same(v, outs["own"]), k


def test_monitor_fp32_device_bound(pgmg, oracle_mod):
    """An fp32 context converts the caller's doubles on load as launch_from_double does."""
    import torch
    N = 257
    rng = np.random.default_rng(7)
    phi0 = rng.uniform(-1.0, 1.0, (N, N))            # not representable in fp32
    f = oracle_mod.rhs_mt64(N)                        # doubles
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem(phi0, f)
        own = s.monitor().res_norm
    t, ft = torch.from_numpy(phi0).cuda(), torch.from_numpy(f).cuda()
    torch.cuda.synchronize()
    with pgmg.Solver(N, dtype="f32") as s:
        s.set_problem_device(t, ft)
        assert _bits(s.monitor().res_norm) == _bits(own)
    want = oracle_res_norm(oracle_mod, phi0.astype(np.float32), f.astype(np.float32), "f32")
    assert close(own, want, N), (own, want)


def test_monitor_keeps_the_carry(pgmg, oracle_mod, plan):
    """v(1), monitor, v(1), monitor ...: phi bitwise the oracle, sweeps equal, and every call
    after the first either took a carry or found it dropped (pgmg_carry_info)."""
    N, calls = 513, 6
    plan(cross_min_n=9)
    h = solve_rule.oracle_history(oracle_mod, "V", N)
    with pgmg.Solver(N) as s:
        s.set_problem()
        for k in range(1, calls + 1):
            s.vcycle(1)
            want = h(k, k)
            m = s.monitor(error=True)
            assert close(m.res_norm, want, N), (k, m.res_norm, want)
            assert close(m.rel_error, h.oracle.rel_error(h.phi(k)), N), k
            assert s.history() == []                      # pgmg_history reads only, too
        assert_bitwise(s.solution(), h.phi(calls), "v(1)/monitor sequence")
        assert s.stats()[0] == h.sweeps(calls)
        took, made, dropped = s.carry_info()
    print("carry_info", took, made, dropped)
    assert took + dropped == calls - 1 and took >= 1, (took, made, dropped)


def test_monitor_error_paths(pgmg, oracle_mod):
    N = 129
    f = oracle_mod.rhs_mt64(N)
    with pgmg.Solver(N) as s:
        with pytest.raises(pgmg.PgmgError):
            s.monitor()                                   # no problem yet
        s.set_problem(None, f)
        with pytest.raises(pgmg.PgmgError):
            s.monitor(error=True)                         # the error needs the analytic problem
        with pytest.raises(pgmg.PgmgError):
            s.monitor(residual=False)                     # nothing asked for
        assert math.isfinite(s.monitor().res_norm)
        f[N // 2, N // 3] = np.nan
        s.set_problem(None, f)
        out = pgmg.PgmgMonitorOut()
        import ctypes as C
        assert s.lib.pgmg_monitor(s.h, pgmg.PGMG_MON_RESIDUAL, C.byref(out)) == 0
        assert math.isnan(out.res_norm)
