"""GPU: every cycle path on IEEE special values, against the oracle (which
tests/test_oracle_special.py pins to the compiled reference on the same input families).

For every family of tests/special_values.py the library and the oracle go through the same
calls; after every call phi is compared with special_values.assert_bitwise_nan (equal NaN masks,
every other word bitwise equal: the sign of a zero, subnormals and Inf count), pgmg_stats()[0]
with the oracle's sweeps and pgmg_stats()[1] with Oracle.cut_exits.

No comparison is vacuous: the census floor of the family is asserted on the ORACLE's result
first (special_values.check_floor) -- at least N negative zeros for neg_zero, 100 subnormal
words for tiny, a non-finite word and a NaN share of at most 25 % for the NaN / Inf families.
The reference's default hierarchy (down to 5 x 5, 10 coarsest sweeps) floods the grid with NaN
within a cycle, so the NaN / Inf families run on the shallow hierarchies of SHALLOW (n_coarse 65
at N >= 129, 17 at N = 33, coarse_iter 0); those rest on the oracle alone, coarse_iter being a
literal in the reference.  `tiny` meets its floor from N = 129 on (measured on the oracle: 586
subnormal words after one default V-cycle at 129, 9 at 33), so its tail-only case at N = 33 runs
n_coarse = 17 (114 words).

What these tests were checked against (scratch builds, one mutation each): a check sum that
multiplies by a 0/1 mask instead of selecting turns test_nan_corner_checks_still_fire red; a
check that fires on a NaN sum turns the nan_f cases red.  Dropping the `+ T(0)` of j0stage
turns nothing red, here or in the older tests: a level entered with x0 = 0 has a +0 frame and
gets a correction from below before its post-smooth, so the -0 that J(0) would then make for a
-0 right-hand side meets a +0 in an add before any word of phi is written
(test_neg_zero_bulk_levels_no_exit runs the case; it pins the result, not that expression).
"""
import functools
import math
import warnings

import numpy as np
import pytest

import damp_model
import fmg_bc_model
import fmg_damped_model
import fmg_model
import oracle
import solve_rule
import special_values as sv
from test_gpu_strips import _run_ranks

pytestmark = pytest.mark.gpu

NONFINITE = ("nan_f", "inf_phi", "nan_frame")


def shallow(N):
    """The hierarchy on which one NaN stays local (see the module docstring)."""
    if N >= 129:
        return dict(n_coarse=65, coarse_iter=0)
    if N >= 33:
        return dict(n_coarse=17, coarse_iter=0)
    return dict(coarse_iter=0)


def _okw(fam, N, okw=None):
    kw = dict(shallow(N)) if fam in NONFINITE else {}
    kw.update(okw or {})
    return kw


@functools.lru_cache(maxsize=None)
def _reference(kind, fam, N, calls, dtype, eps, okw, floor=True):
    """The oracle's snapshots [(phi, sweeps, cut_exits) per call], floors checked, shared.
    floor=False: the caller states its own floor (and why the family's cannot hold)."""
    snaps = sv.run_oracle(kind, fam, N, list(calls), dtype=dtype, eps=eps, **dict(okw))
    for phi, _, _ in snaps:
        if floor:
            sv.check_floor(fam, phi, dtype)
    return snaps


def _problem(fam, N, dtype, gen_f=False):
    """(phi0, f) as float64 arrays for set_problem; f None: the analytic f, regenerated."""
    phi0, f = sv.family(fam, N, dtype)
    if f is None and not gen_f:
        f = sv.analytic_f(N, dtype)
    return phi0.astype(np.float64), None if f is None else f.astype(np.float64)


def _run(pgmg, fam, N, kind="V", calls=(1,), dtype="f64", eps=1e-7, okw=None, gen_f=False,
         after=None, what="", floor=True, **cfg):
    okw = _okw(fam, N, okw)
    snaps = _reference(kind, fam, N, tuple(calls), dtype, eps, tuple(sorted(okw.items())), floor)
    phi0, f = _problem(fam, N, dtype, gen_f)
    with pgmg.Solver(N, dtype=dtype, eps=eps, **okw, **cfg) as s:
        s.set_problem(phi0, f)
        run = {"V": s.vcycle, "W": s.wcycle, "F": s.fcycle}[kind]
        for n, (phi, sweeps, cut) in zip(calls, snaps):
            run(n)
            tag = f"{what} {fam} {kind} N={N} {dtype} eps={eps} {okw} calls={calls} after {n}"
            sv.assert_bitwise_nan(s.solution(), phi, tag)
            assert s.stats() == (sweeps, cut), (tag, s.stats(), (sweeps, cut))
        if after is not None:
            after(s)
    return snaps


# ---------------------------------------------------------------------------------------------
# the default fused V path: k_postpre_lds, the carry and the recompute form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [(3,), (1, 1, 1)], ids=["v3", "v1x3"])
@pytest.mark.parametrize("N", [129, 513])
@pytest.mark.parametrize("fam", sv.FAMILIES)
def test_default_fused_v(pgmg, plan, fam, N, calls):
    """f regenerated in-kernel where the family's f is the analytic one (inf_phi, nan_frame),
    stored otherwise; the one-cycle calls carry."""
    plan(cross_min_n=9)

    def after(s):
        assert s.stats_detail()[2] >= 0, "cross-cycle fusion not active"
        s.carry_info()

    _run(pgmg, fam, N, calls=calls, gen_f=True, after=after, what="fused")


@pytest.mark.parametrize("fam", ["point_source", "nan_f"])
def test_wave_tile_inside_a_row_2049(pgmg, plan, fam):
    """N = 2049: the first size with a wave tile strictly inside a row."""
    plan(cross_min_n=9)
    okw = dict(n_coarse=65, coarse_iter=0) if fam == "nan_f" else None
    _run(pgmg, fam, 2049, calls=(1, 1), okw=okw, what="2049")


# ---------------------------------------------------------------------------------------------
# alternative plans
# ---------------------------------------------------------------------------------------------
def _plans(pgmg):
    return {"unfused": (129, dict(flags=pgmg.PGMG_FLAG_UNFUSED)),
            "no_ctile": (129, dict(flags=pgmg.PGMG_FLAG_NO_CTILE)),
            "no_recompute": (129, dict(flags=pgmg.PGMG_FLAG_NO_RECOMPUTE, cross_min_n=9)),
            "exact_dist": (129, dict(flags=pgmg.PGMG_FLAG_EXACT_DIST, cross_min_n=9)),
            "no_carry": (129, dict(flags=pgmg.PGMG_FLAG_NO_CARRY, cross_min_n=9)),
            "stored_rhs": (129, dict(flags=pgmg.PGMG_FLAG_STORED_RHS, cross_min_n=9)),
            "tail_only": (33, {}),
            "one_level": (5, {})}


PLANS = ["unfused", "no_ctile", "no_recompute", "exact_dist", "no_carry", "stored_rhs",
         "tail_only", "one_level"]


@pytest.mark.parametrize("fam", ["neg_zero", "point_source", "nan_f"])
@pytest.mark.parametrize("name", PLANS)
def test_alternative_plans(pgmg, name, fam):
    N, cfg = _plans(pgmg)[name]

    def after(s):
        bulk, top = s.levels()
        if name == "tail_only":
            assert bulk == 0 and top == 33, (bulk, top)
        if name == "one_level":
            assert bulk == 0 and top == 5, (bulk, top)

    # (at N = 33 a second cycle takes the NaN share of nan_f past the cap: 9 %, then 36 %)
    calls = (2, 1) if N == 129 else (1,) if (N == 33 and fam == "nan_f") else (1, 1)
    _run(pgmg, fam, N, calls=calls, after=after, what=name, **cfg)


@pytest.mark.parametrize("fam", ["tiny", "inf_phi", "nan_frame"])
def test_tail_only_other_families(pgmg, fam):
    _run(pgmg, fam, 33, calls=(1,), okw=dict(n_coarse=17), gen_f=True, what="tail_only")


# ---------------------------------------------------------------------------------------------
# W and F cycles
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [2, 3])
@pytest.mark.parametrize("fam", sv.FAMILIES)
def test_w_cycles(pgmg, fam, alpha):
    if fam == "tiny":
        # every check fires, so a W-cycle down to 5 x 5 leaves 39 subnormal words; n_coarse = 17
        # leaves 495 (alpha 2) and 145 (alpha 3) after the first cycle, fewer after the second
        _run(pgmg, fam, 129, kind="W", calls=(1,), okw=dict(alpha=alpha, n_coarse=17),
             what=f"W alpha={alpha}")
        return
    _run(pgmg, fam, 129, kind="W", calls=(1, 1), okw=dict(alpha=alpha), what=f"W alpha={alpha}")


# the F-cycle reads phi only (its right-hand sides are the analytic ones of its own chain):
# the families whose phi0 is special.
@pytest.mark.parametrize("variant", ["default", "no_pin", "no_r2"])
@pytest.mark.parametrize("fam", ["neg_zero", "inf_phi", "nan_frame"])
def test_f_cycles(pgmg, fam, variant):
    """inf_phi: the Inf is restricted down the pyramid and comes back as a NaN region (floor and
    cap asserted).  neg_zero and nan_frame leave no trace in the reference's result, and that is
    what is pinned: the restriction reads no frame word, a restricted -0 is smoothed and
    prolonged into a zeroed grid (-0 + +0 = +0), and the result's frame is the zeroed grid's --
    so the oracle's result is asserted bitwise equal to the F-cycle from phi0 = +0, and the
    library must give the same words, not one -0 or NaN among them."""
    flags = {"default": 0, "no_pin": pgmg.PGMG_FLAG_NO_PIN, "no_r2": pgmg.PGMG_FLAG_NO_R2}[variant]
    snaps = _run(pgmg, fam, 129, kind="F", calls=(1, 1), gen_f=True, what=f"F {variant}",
                 floor=fam == "inf_phi", flags=flags)
    if fam != "inf_phi":
        plain = sv.run_oracle("F", fam, 129, [2], phi0_f=(np.zeros((129, 129)), None),
                              **_okw(fam, 129))[0][0]
        sv.assert_bitwise_nan(snaps[-1][0], plain, f"F-cycle from {fam} vs from +0")
        assert sv.census(snaps[-1][0]) == {"nz": 0, "sub": 0, "inf": 0, "nan": 0}


# ---------------------------------------------------------------------------------------------
# device-bound problems and row strips
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["inplace", "staged"])
@pytest.mark.parametrize("fam", ["neg_zero", "point_source", "nan_f", "inf_phi"])
def test_device_bound(pgmg, fam, binding):
    import torch
    N, calls = 129, (2, 1)
    okw = _okw(fam, N)
    snaps = _reference("V", fam, N, calls, "f64", 1e-7, tuple(sorted(okw.items())))
    phi0, f = _problem(fam, N, "f64", gen_f=True)
    with pgmg.Solver(N, cross_min_n=33, **okw) as s:
        if binding == "inplace":
            g = pgmg.DeviceGrid(N, phi0)
            fd = None if f is None else pgmg.DeviceGrid(N, f)
            read = g.download
        else:
            g = torch.from_numpy(phi0).cuda()
            fd = None if f is None else torch.from_numpy(f).cuda()
            torch.cuda.synchronize()
            read = lambda: g.cpu().numpy()
        s.set_problem_device(g, fd)
        assert s.device_info() == (True, binding == "inplace")
        for n, (phi, sweeps, cut) in zip(calls, snaps):
            s.vcycle(n)
            s.sync()
            sv.assert_bitwise_nan(read(), phi, f"{binding} {fam} after {n}")
            assert s.stats() == (sweeps, cut)
        if binding == "inplace":
            g.close()
            if fd is not None:
                fd.close()


@pytest.mark.parametrize("fam", ["neg_zero", "nan_f"])
def test_two_loopback_strips(pgmg, fam):
    N, cycles = 129, 2
    okw = _okw(fam, N)
    cfg = dict(gather_n=65, tail_n=17, **okw)
    assert pgmg.plan_strips(N, 2, 0, tail_n=17, gather_n=65)[2] == 1   # level 0 is distributed
    snaps = _reference("V", fam, N, (1, 1), "f64", 1e-7, tuple(sorted(okw.items())))
    phi0, f = _problem(fam, N, "f64")
    outs = _run_ranks(pgmg, 2, N, cycles, problem={r: (phi0, f) for r in range(2)}, **cfg)
    for r, out in enumerate(outs):
        sv.assert_bitwise_nan(out[0], snaps[-1][0], f"strips {fam} rank {r}")
    assert outs[0][1] == snaps[-1][1:], (outs[0][1], snaps[-1][1:])


# ---------------------------------------------------------------------------------------------
# neg_zero: norms of exactly 0
# ---------------------------------------------------------------------------------------------
# one V-cycle on f = phi0 = -0.0 (oracle): N -> (negative zeros left, sweeps, cut exits)
NEG_ZERO_FIRES = {5: (25, 1, 1), 9: (33, 3, 3), 33: (129, 7, 7), 129: (513, 11, 11)}
NEG_ZERO_NEVER = {5: (25, 11, 0), 9: (32, 15, 0), 33: (128, 23, 0), 129: (512, 31, 0)}


@pytest.mark.parametrize("eps", [1e-7, 0.0])
@pytest.mark.parametrize("N", [5, 9, 33, 129])
def test_neg_zero_checks(pgmg, N, eps):
    """eps = 1e-7: every check fires on a norm of exactly 0 (one sweep per smoother call);
    eps = 0: sqrt(0) < 0 is false, none fires.  The -0 that survive are the prolongation's
    uncorrected fine row and column 1 and the frame."""
    nz, sweeps, cut = (NEG_ZERO_FIRES if eps else NEG_ZERO_NEVER)[N]
    snaps = _run(pgmg, "neg_zero", N, calls=(1,), eps=eps, what="neg_zero checks")
    phi, s, c = snaps[0]
    assert (sv.census(phi)["nz"], s, c) == (nz, sweeps, cut), (sv.census(phi), s, c)


@pytest.mark.parametrize("plan_name", ["default", "cross", "no_recompute", "no_ctile", "unfused"])
@pytest.mark.parametrize("kind,N", [("V", 257), ("V", 513), ("W", 257)])
def test_neg_zero_bulk_levels_no_exit(pgmg, N, plan_name, kind):
    """eps = 0 on grids with bulk levels below the finest (257: one, 513: two).  No check fires,
    so those levels, entered with x0 = 0, run their full pre-smooth on a right-hand side that is
    -0 wherever the restricted residual is: the first sweep J(0) = 0.25 * ((hh * -0) + 0 + ...)
    is +0, and a shortcut that drops the adds of zero makes it -0, which the prolongation's
    fine += e then carries into phi (-0 + -0 = -0, where the reference has -0 + +0 = +0).  With
    eps = 1e-7 every check fires after J(0) and the one-sweep rare paths run instead; at
    N <= 129 the only bulk level is the finest, which is never entered with x0 = 0."""
    cfg = {"default": {}, "cross": dict(cross_min_n=9),
           "no_recompute": dict(cross_min_n=9, flags=pgmg.PGMG_FLAG_NO_RECOMPUTE),
           "no_ctile": dict(flags=pgmg.PGMG_FLAG_NO_CTILE),
           "unfused": dict(flags=pgmg.PGMG_FLAG_UNFUSED)}[plan_name]

    def after(s):
        assert s.levels()[0] >= 2, s.levels()

    _run(pgmg, "neg_zero", N, kind=kind, calls=(1, 1), eps=0.0, after=after,
         what=f"neg_zero eps=0 {plan_name}", **cfg)


# ---------------------------------------------------------------------------------------------
# nan_corner: non-finite words that only discarded lanes see
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [(3,), (1, 1, 1)], ids=["x3", "1x3"])
@pytest.mark.parametrize("kind,N,plan_name", [("V", 129, "cross"), ("V", 513, "cross"),
                                              ("V", 513, "default"), ("V", 129, "exact_dist"),
                                              ("W", 129, "default"), ("V", 2049, "cross")])
def test_nan_corner_checks_still_fire(pgmg, kind, N, plan_name, calls):
    """NaN and +-Inf in the four corners of phi, eps = 1e3.  No stencil of the reference reads a
    corner, so every residual and every norm is finite and every check fires; the corners stay.
    The kernels do compute residuals on frame lanes (from the corner words and from loads past
    the grid) and throw them away: a check sum that lets such a lane in -- 0 * NaN is NaN --
    stops firing, and the sweep and exit counts show it."""
    cfg = {"default": {}, "cross": dict(cross_min_n=9),
           "exact_dist": dict(cross_min_n=9, flags=pgmg.PGMG_FLAG_EXACT_DIST)}[plan_name]
    snaps = _run(pgmg, "nan_corner", N, kind=kind, calls=calls, eps=1e3, okw={}, gen_f=True,
                 what=f"nan_corner {plan_name}", **cfg)
    phi, sweeps, cut = snaps[-1]
    c = sv.census(phi)
    assert (c["nan"], c["inf"]) == (2, 2) and cut > 0, (c, sweeps, cut)


# ---------------------------------------------------------------------------------------------
# locality: the NaN mask after 1 and 2 cycles on the shallow hierarchies
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N", [("V", 129), ("V", 257), ("V", 513), ("W", 129), ("W", 257)])
@pytest.mark.parametrize("fam", NONFINITE)
def test_nan_locality(pgmg, fam, kind, N):
    okw = dict(n_coarse=65, coarse_iter=0)
    if kind == "W":
        okw["alpha"] = 2
    snaps = _run(pgmg, fam, N, kind=kind, calls=(1, 1), okw=okw, gen_f=True, what="locality")
    shares = [sv.census(p)["nan"] / p.size for p, _, _ in snaps]
    print(f"NaN share {fam} {kind} N={N}: {shares}")
    assert 0 < shares[0] <= shares[1] <= 0.25, shares


# ---------------------------------------------------------------------------------------------
# extreme scales and the speculation planner
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["v2", "v12", "seg2"])
@pytest.mark.parametrize("fam", ["tiny", "huge"])
def test_extreme_scales(pgmg, plan, fam, mode):
    """tiny: r^2 underflows to 0, every check fires; huge: r^2 overflows, the sum is Inf, none
    fires and every grid word stays finite."""
    N = 129
    if mode == "seg2":
        plan(cross_min_n=9, spec_segment=2)
    calls = (2,) if mode == "v2" else (12,)
    # tiny after 12 cycles: phi has grown into the normal range (20 subnormal words left), so
    # the floor of the 12-cycle runs is the one their first two cycles meet (242 words)
    _reference("V", fam, N, (2,), "f64", 1e-7, ())
    snaps = _run(pgmg, fam, N, calls=calls, what=mode, floor=mode == "v2")
    phi, sweeps, cut = snaps[0]
    if mode == "v2":
        o = oracle.Oracle()
        phi0, f = sv.family(fam, N)
        x = phi0.copy()
        o.v_cycle(x, f)
        o.v_cycle(x, f)
        want = (22, 22) if fam == "tiny" else (62, 0)
        assert (o.sweeps, o.early_exits) == want and sweeps == want[0], (o.sweeps, o.early_exits)
    if fam == "huge":
        c = sv.census(phi)
        assert c["inf"] == c["nan"] == 0 and cut == 0, (c, cut)


@pytest.mark.parametrize("seg", [0, 2], ids=["default_spec", "seg2"])
@pytest.mark.parametrize("kind,n", [("V", 12), ("W", 3)])
@pytest.mark.parametrize("fam", ["nan_f", "neg_zero", "huge"])
def test_planner_sees_special_norms(pgmg, plan, fam, kind, n, seg):
    """The speculation planner (spec_level_trend, spec_mark_levels, spec_plan_segment) on norms
    that are NaN, 0 and Inf: results and counters are the oracle's, the plan queries answer.
    nan_f runs the default hierarchy here (the planner needs the bulk levels; the NaN mask and
    the counters are still compared), so its floor is the non-finite one without the cap."""
    plan(cross_min_n=9)      # speculative calls need the cross-cycle finest pass
    if seg:
        plan(spec_segment=seg)
    N = 513
    calls = (n, n)
    o = oracle.Oracle()
    phi0, f = sv.family(fam, N)
    phi = phi0.copy()
    phi0, f = _problem(fam, N, "f64")
    with pgmg.Solver(N) as s:
        s.set_problem(phi0, f)
        for k in calls:
            for _ in range(k):
                (o.v_cycle if kind == "V" else o.w_cycle)(phi, np.ascontiguousarray(f))
            (s.vcycle if kind == "V" else s.wcycle)(k)
            c = sv.census(phi)
            if fam == "nan_f":
                assert c["nan"] >= 1
            elif fam == "neg_zero":
                assert c["nz"] >= N
            sv.assert_bitwise_nan(s.solution(), phi, f"planner {fam} {kind} x{k} seg={seg}")
            assert s.stats() == (o.sweeps, o.cut_exits), (s.stats(), o.sweeps, o.cut_exits)
            sp, rb = s.dist_info()
            print(f"planner {fam} {kind} x{k} seg={seg}: speculative {sp}, rollbacks {rb}, "
                  f"levels {s.spec_levels():#x}, carry {s.carry_info()}")
            assert sp or rb >= 1, "the call never speculated: the planner saw nothing"


# ---------------------------------------------------------------------------------------------
# monitor, solve, damp
# ---------------------------------------------------------------------------------------------
def _same_norm(got, want, N):
    if math.isnan(want):
        return math.isnan(got)
    if want == 0.0 or math.isinf(want):
        return got == want
    return solve_rule.close(got, want, N)


@pytest.mark.parametrize("fam", sv.FAMILIES)
def test_monitor(pgmg, oracle_mod, fam):
    """res_norm is NaN, Inf or 0 exactly where the oracle's sequential norm is; otherwise within
    solve_rule.norm_tol.  Before any cycle and after one."""
    N = 129
    okw = _okw(fam, N)
    snaps = _reference("V", fam, N, (1,), "f64", 1e-7, tuple(sorted(okw.items())))
    phi0, f = _problem(fam, N, "f64")
    with pgmg.Solver(N, **okw) as s:
        s.set_problem(phi0, f)
        for phi in (phi0, snaps[0][0]):
            want = solve_rule.oracle_res_norm(oracle_mod, phi, f)
            got = s.monitor().res_norm
            print(f"monitor {fam}: got {got!r} want {want!r}")
            assert _same_norm(got, want, N), (fam, got, want)
            s.vcycle(1)
    if fam in ("nan_f", "nan_frame"):
        assert math.isnan(want)
    if fam == "huge":
        assert math.isinf(want)
    if fam == "neg_zero":
        assert want == 0.0


@pytest.mark.parametrize("damp", [0.0, 0.5], ids=["solve", "solve_damped"])
@pytest.mark.parametrize("fam", ["nan_f", "neg_zero", "huge"])
def test_solve_stops(pgmg, oracle_mod, fam, damp):
    N = 129
    phi0, f = _problem(fam, N, "f64")
    r0 = solve_rule.oracle_res_norm(oracle_mod, phi0, f)
    _, reason, recs, _ = solve_rule.simulate(lambda i, k: r0 if k == 0 else None)
    want = {"nan_f": solve_rule.NONFINITE, "neg_zero": solve_rule.CONVERGED,
            "huge": solve_rule.NONFINITE}[fam]
    assert reason == want and len(recs) == 1, (reason, recs)
    with pgmg.Solver(N) as s:
        s.set_problem(phi0, f)
        info = s.solve(damp=damp)
        assert (info.cycles, info.reason, info.checks) == (0, want, 1), (info.cycles, info.reason)
        assert _same_norm(info.res0, r0, N) and _same_norm(info.res, r0, N), (info.res0, r0)
        if fam == "neg_zero":
            assert info.res0 == 0.0
        if fam == "huge":
            assert math.isinf(info.res0) and all(math.isinf(r) for _, r, _ in info.history)
        assert s.stats() == (0, 0)


@pytest.mark.parametrize("fam", ["neg_zero", "tiny", "nan_f"])
def test_damp_pass(pgmg, fam):
    """pgmg_damp after one V-cycle against tests/damp_model.py."""
    N = 129
    okw = _okw(fam, N)
    snaps = _reference("V", fam, N, (1,), "f64", 1e-7, tuple(sorted(okw.items())))
    phi0, f = _problem(fam, N, "f64")
    with np.errstate(all="ignore"):
        want, want_norm = damp_model.damp(snaps[0][0], f, 1.0 / (N - 1), 0.5)
    sv.check_floor(fam, want)
    with pgmg.Solver(N, **okw) as s:
        s.set_problem(phi0, f)
        s.vcycle(1)
        got_norm = s.damp(0.5)
        sv.assert_bitwise_nan(s.solution(), want, f"damp {fam}")
        assert _same_norm(got_norm, want_norm, N), (got_norm, want_norm)


# ---------------------------------------------------------------------------------------------
# full multigrid
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fmg_want(fam, N, variant):
    o = oracle.Oracle(n_coarse=17 if N == 129 else 5)
    phi0, f = sv.family(fam, N)
    f = sv.analytic_f(N) if f is None else f
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if variant == "fmg":
            u = fmg_model.fmg(o, f, 2)
        elif variant == "damped":
            u = fmg_damped_model.fmg_damped(o, f, 2, 0.5)
        else:
            u = fmg_bc_model.fmg_bc(o, phi0, f, 2)
    u.setflags(write=False)
    return u, o.sweeps, o.cut_exits


@pytest.mark.parametrize("variant", ["fmg", "damped", "keep"])
@pytest.mark.parametrize("N", [33, 129])
@pytest.mark.parametrize("fam", ["point_source", "tiny", "nan_f", "nan_frame"])
def test_fmg(pgmg, fam, N, variant):
    """fmg(2), fmg(2, damp=0.5) and fmg(2, boundary="keep") against their numpy models.  The
    models' own results meet the floors first: 100 subnormal words for tiny at N = 129, a
    non-finite word for the NaN families (FMG visits
    the 5 x 5 / 17 x 17 level and floods the interior: the mask is what is compared).  nan_frame: boundary="zero" ignores the caller's
    frame, boundary="keep" leaves its NaN and -Inf in place, -Inf bitwise."""
    want, sweeps, cut = _fmg_want(fam, N, variant)
    c = sv.census(want)
    if fam == "tiny" and N == 129:      # (at N = 33 the climb's result holds none)
        assert c["sub"] >= 100, c
    if fam == "nan_f" or (fam == "nan_frame" and variant == "keep"):
        assert c["nan"] + c["inf"] >= 1, c
    phi0, f = _problem(fam, N, "f64")
    with pgmg.Solver(N, n_coarse=17 if N == 129 else 5) as s:
        s.set_problem(phi0, f)
        if variant == "fmg":
            s.fmg(2)
        elif variant == "damped":
            s.fmg(2, damp=0.5)
        else:
            s.fmg(2, boundary="keep")
        got = s.solution()
        sv.assert_bitwise_nan(got, want, f"fmg {variant} {fam} N={N}")
        # (the damping passes of the climb are not smoother sweeps; as tests/test_gpu_fmg_damped.py)
        assert s.stats()[0] == sweeps, (s.stats(), sweeps, cut)
        if variant == "fmg":
            assert s.stats() == (sweeps, cut), (s.stats(), sweeps, cut)
    if fam == "nan_frame" and variant == "keep":
        a, b = N // 3, 2 * N // 3
        assert math.isnan(got[0, a]) and got[b, N - 1] == -math.inf
        for edge_got, edge_in in ((got[0], phi0[0]), (got[-1], phi0[-1]), (got[:, 0], phi0[:, 0]),
                                  (got[:, -1], phi0[:, -1])):
            sv.assert_bitwise_nan(np.ascontiguousarray(edge_got), np.ascontiguousarray(edge_in),
                                  "the caller's frame")


# ---------------------------------------------------------------------------------------------
# fp32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 129, 513])
@pytest.mark.parametrize("fam", sv.FAMILIES)
def test_fp32(pgmg, plan, fam, N):
    """Against liboracle_f32 on the default fused path (N = 129, 513) and the tail-only N = 33.
    A build that flushed fp32 denormals fails `tiny` (1e-36 * f leaves subnormal floats) and
    `neg_zero`."""
    if N > 33:
        plan(cross_min_n=9)
    okw = dict(n_coarse=17) if (fam == "tiny" and N == 33) else None
    _run(pgmg, fam, N, calls=(2, 1) if N > 33 else (1,), dtype="f32", okw=okw, gen_f=True,
         what="fp32")


@pytest.mark.parametrize("binding", ["host", "device"])
def test_abi_f32_conversion(pgmg, binding):
    """fp32 contexts round the caller's doubles to fp32 by IEEE round-to-nearest-even: overflow
    to Inf, gradual underflow (1e-40 stays a subnormal, -1e-46 becomes -0), ties to even, NaN
    stays NaN.

    host: solution() right after set_problem is phi0.astype(float32).
    device (a problem staged through set_problem_device): binding converts nothing -- the
    solution of a device-bound problem IS the caller's array, which holds the caller's own
    doubles until the first call writes it (include/pgmg.h, "Special values", the stated
    deviation) -- so the conversion is pinned where it becomes visible: after one V-cycle the
    array is the fp32 oracle's result from the rounded inputs, and its frame, which no sweep
    writes, is phi0's rounded to fp32 word for word."""
    import torch
    N = 129
    okw = dict(n_coarse=65, coarse_iter=0)     # the NaN of the frame stays near the frame
    phi0, f = sv.abi_f32(N, finite_interior=binding == "device")
    with np.errstate(all="ignore"):
        want0 = phi0.astype(np.float32)
        f32 = f.astype(np.float32)
    c = sv.census(want0)
    assert min(c["sub"], c["inf"], c["nan"], c["nz"]) >= (30 if binding == "device" else 1000), c
    assert np.float32(1.0 + 2.0 ** -24) == 1.0 and np.float32(1.0 + 3 * 2.0 ** -24) > 1.0
    o = oracle.Oracle(dtype="f32", **okw)
    want1 = want0.copy()
    o.v_cycle(want1, f32)
    frame = np.ones((N, N), dtype=bool)
    frame[1:-1, 1:-1] = False
    cf = sv.census(want1[frame])
    assert min(cf["sub"], cf["inf"], cf["nan"], cf["nz"]) >= 30, cf
    if binding == "device":                    # finite words to compare next to the frame's NaN
        assert np.isfinite(want1[1:-1, 1:-1]).sum() >= 0.5 * N * N
    with pgmg.Solver(N, dtype="f32", **okw) as s:
        if binding == "host":
            s.set_problem(phi0, f)
            sv.assert_bitwise_nan(s.solution(), want0.astype(np.float64), "abi_f32 host")
        else:
            g, fd = torch.from_numpy(phi0).cuda(), torch.from_numpy(f).cuda()
            torch.cuda.synchronize()
            s.set_problem_device(g, fd)
            assert s.device_info() == (True, False)
            sv.assert_bitwise_nan(s.solution(), phi0, "abi_f32 device: the caller's array")
        s.vcycle(1)
        got = s.solution()
        sv.assert_bitwise_nan(got, want1.astype(np.float64), f"abi_f32 {binding} after a cycle")
        sv.assert_bitwise_nan(got[frame], want0[frame].astype(np.float64), "the rounded frame")
        assert s.stats() == (o.sweeps, o.cut_exits)
        if binding == "device":
            sv.assert_bitwise_nan(g.cpu().numpy(), want1.astype(np.float64), "the bound array")
