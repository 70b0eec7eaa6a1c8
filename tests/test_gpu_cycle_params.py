"""alpha, n_coarse and coarse_iter off their defaults (3, 5, 10), against the oracle.

pgmg_config's three cycle-shaping parameters steer the part of the library most specialised on
the defaults (pgmg_tail.hip): tail_coarse5_gamma's run-time-count instance (alpha != 3) and its
sequential fallback (alpha >= 4, coarse_iter = 0), the generic tail_gcycle loop wherever tail_w9 /
tail_wq<17> do not apply (n_coarse 3, 9, 17: tail_smooth as the coarsest solve at N = 3, 9, 17,
a 5x5 level as an ordinary level above a 3x3 one), a tail that is one large coarsest solve
(n_coarse >= the tail's top), the W plans of the bulk levels with gamma != 3, the gathered levels
of row strips and pgmg_fmg's coarsest start.

The checker is the CPU oracle (oracle/pgmg_oracle.c), pinned to the reference's own
MultigridSolver off the defaults for alpha and n_coarse by tests/test_oracle_golden.py
(tests/golden/cycles_params.json); coarse_iter is a literal in the reference, there the oracle's
orc_smooth_alloc(c, ..., c->coarse_iter) is the definition.  Tolerance: EXACT.  After every
cycle phi is bitwise the oracle's and pgmg_stats equals (o.sweeps, o.cut_exits): the sweep count,
and the early exits that cut a smoother call short.  o.early_exits itself also counts a check
that fires after a call's LAST sweep; the library never evaluates that check (it cannot change
the result), so its counter is o.early_exits - o.last_exits = o.cut_exits, exactly (where no
such last-sweep exit happens -- eps = 0, or every check firing at once -- that is o.early_exits).

Sizes: N <= 257, 2-4 cycles; every path-targeting case asserts pgmg_levels (bulk levels, the
tail's top) so that a re-routing cannot hollow it out.  alpha > 15 and an n_coarse that would
put more than 65x65 points into the tail are rejected by pgmg_create (tests/test_capi.py) and
are never run here.
"""
import functools

import numpy as np
import pytest

import fmg_model
import oracle
from conftest import assert_bitwise
from test_gpu_strips import _run_ranks, _single

gpu = pytest.mark.gpu

# pgmg_config fields that the oracle takes too; h0 (tests/test_gpu_problem_params.py) is the
# mesh width handed to the oracle's rhs and cycle calls, 0 or absent: a / (N - 1)
ORACLE_KEYS = ("alpha", "n_coarse", "coarse_iter", "v1", "v2", "a", "p", "q", "h0")
EPS5 = [1e-7, 1e-2, 1e-4, 1e3, 0.0]


def _problem(N, dtype, rand):
    """(phi0, f) as float64 arrays holding values of `dtype`; (None, None): phi0 = 0 and the
    analytic f.  rand: a random phi0 with a non-zero boundary and the mt19937_64 robustness
    right-hand side; rand = "phi": that phi0 with the analytic f."""
    if not rand:
        return None, None
    dt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(4242 + N)
    phi0 = rng.uniform(-1.0, 1.0, (N, N)).astype(dt).astype(np.float64)
    assert np.abs(phi0[0]).min() > 0 and np.abs(phi0[:, -1]).min() > 0
    if rand == "phi":
        return phi0, None
    f = oracle.rhs_mt64(N, dtype=dtype).astype(np.float64)
    return phi0, f


@functools.lru_cache(maxsize=None)
def _reference(kind, N, cycles, dtype, eps, rand, okw):
    """The oracle's run, computed once per case and shared: ([(phi, sweeps, cut_exits) after
    every cycle], (early_exits, smooth_calls) at the end).  A W-cycle with alpha = 1 is
    o.v_cycle."""
    kw = dict(okw)
    h = kw.pop("h0", 0.0) or None
    o = oracle.Oracle(eps=eps, dtype=dtype, **kw)
    phi0, f = _problem(N, dtype, rand)
    f = o.rhs(N, h) if f is None else np.ascontiguousarray(f, dtype=o.dt)
    phi = np.zeros((N, N), dtype=o.dt) if phi0 is None else np.array(phi0, dtype=o.dt)
    step = {"V": o.v_cycle, "W": o.v_cycle if kw.get("alpha", 3) == 1 else o.w_cycle}.get(kind)
    snaps = []
    for _ in range(cycles):
        if kind == "F":
            o.f_cycle_outer(phi)
        else:
            step(phi, f, h)
        snap = phi.astype(np.float64)
        snap.setflags(write=False)
        snaps.append((snap, o.sweeps, o.cut_exits))
    return snaps, (o.early_exits, o.smooth_calls)


def _okw(cfg):
    return tuple(sorted((k, cfg[k]) for k in ORACLE_KEYS if k in cfg))


def _check(pgmg, kind, N, cycles=3, dtype="f64", eps=1e-7, rand=False, levels=None, calls=None,
           after=None, **cfg):
    """`cycles` one-cycle calls (or the calls given) of `kind` on one context; phi and the
    statistics against the oracle after every call."""
    calls = [1] * cycles if calls is None else list(calls)
    snaps, _ = _reference(kind, N, sum(calls), dtype, eps, rand, _okw(cfg))
    phi0, f = _problem(N, dtype, rand)
    with pgmg.Solver(N, dtype=dtype, eps=eps, **cfg) as s:
        if levels is not None:
            assert s.levels() == levels, (s.levels(), levels)
        s.set_problem(phi0, f)
        run = {"V": s.vcycle, "W": s.wcycle, "F": s.fcycle}[kind]
        done = 0
        for n in calls:
            run(n)
            done += n
            tag = f"{kind} N={N} {dtype} eps={eps} rand={rand} {cfg} cycle={done}"
            phi, sweeps, cut = snaps[done - 1]
            assert_bitwise(s.solution(), phi, tag)
            assert s.stats() == (sweeps, cut), (tag, s.stats(), (sweeps, cut))
        if after is not None:
            after(s)


def _mix(kind, N, cycles, dtype, eps, rand, **okw):
    """"none" / "all" / "mixed": how the oracle's early exits fell over the case's smoother calls."""
    _, (exits, calls) = _reference(kind, N, cycles, dtype, eps, rand, _okw(okw))
    assert calls > 0
    return "none" if exits == 0 else "all" if exits == calls else "mixed"


# ---------------------------------------------------------------------------------------------
# alpha
# ---------------------------------------------------------------------------------------------
# (N, alpha, eps, dtype, cycles, rand, cfg, levels); levels = (bulk levels, the tail's top)
ALPHA_CASES = [
    # the tail alone (tail_coarse5_gamma<Real, 0>: alpha 2 on the one-reduction path with a
    # run-time count, alpha >= 4 on the sequential fallback; tail_w9 / tail_wq<17> with gamma != 3)
    (33, 1, 1e-7, "f64", 3, False, {}, (0, 33)),
    (33, 2, 1e-7, "f64", 3, False, {}, (0, 33)),
    (33, 4, 1e-4, "f64", 3, False, {}, (0, 33)),
    (33, 2, 1e-2, "f32", 3, False, {}, (0, 33)),
    (33, 15, 1e-7, "f64", 2, False, {}, (0, 33)),
    (33, 15, 1e-4, "f32", 2, False, {}, (0, 33)),
    (17, 15, 1e-2, "f64", 2, False, {}, (0, 17)),
    (17, 15, 0.0, "f32", 2, False, {}, (0, 17)),
    (65, 1, 1e-7, "f64", 3, False, {}, (0, 65)),
    (65, 2, 1e-7, "f64", 4, False, {}, (0, 65)),
    (65, 2, 1e-2, "f64", 3, False, {}, (0, 65)),
    (65, 2, 1e-4, "f64", 3, False, {}, (0, 65)),
    (65, 2, 1e3, "f64", 3, False, {}, (0, 65)),
    (65, 2, 0.0, "f64", 3, False, {}, (0, 65)),
    (65, 4, 1e-7, "f64", 3, False, {}, (0, 65)),
    (65, 4, 1e-4, "f64", 3, False, {}, (0, 65)),
    (65, 4, 1e3, "f64", 3, False, {}, (0, 65)),
    (65, 4, 0.0, "f64", 3, False, {}, (0, 65)),
    (65, 2, 1e-4, "f32", 3, False, {}, (0, 65)),
    (65, 4, 1e-7, "f32", 3, False, {}, (0, 65)),
    (65, 2, 1e-7, "f64", 3, True, {}, (0, 65)),
    (65, 4, 1e-2, "f32", 3, True, {}, (0, 65)),
    # one bulk level
    (129, 1, 1e-4, "f64", 3, False, {}, (1, 65)),
    (129, 2, 1e-7, "f64", 3, False, {}, (1, 65)),
    (129, 2, 1e-4, "f64", 4, False, {}, (1, 65)),
    (129, 2, 1e3, "f64", 3, False, {}, (1, 65)),
    (129, 2, 0.0, "f64", 3, False, {}, (1, 65)),
    (129, 4, 1e-2, "f64", 3, False, {}, (1, 65)),
    (129, 4, 1e-4, "f64", 3, False, {}, (1, 65)),
    (129, 2, 1e-2, "f32", 3, False, {}, (1, 65)),
    (129, 4, 1e-4, "f32", 3, False, {}, (1, 65)),
    (129, 2, 1e-4, "f64", 3, True, {}, (1, 65)),
    # several bulk levels (257, 129, 65, 33 above a 17x17 tail)
    (257, 1, 1e-7, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 2, 1e-7, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 2, 1e-4, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 4, 1e-2, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 4, 1e3, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 2, 0.0, "f64", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 2, 1e-4, "f32", 3, False, {"tail_n": 17}, (4, 17)),
    (257, 4, 1e-7, "f32", 3, True, {"tail_n": 17}, (4, 17)),
]
# the issue's conditions on the inputs, from the oracle's counters (test_exit_mix_of_every_family)
ALPHA_MIX = {"mixed": ("W", 129, 4, "f64", 1e-4, False, dict(alpha=2)),
             "all": ("W", 65, 3, "f64", 1e3, False, dict(alpha=2)),
             "none": ("W", 65, 3, "f64", 0.0, False, dict(alpha=4))}


def _id(c):
    return "-".join(str(x) for x in c if not isinstance(x, (dict, tuple)) or x)


@gpu
@pytest.mark.parametrize("case", ALPHA_CASES, ids=_id)
def test_alpha_wcycle_against_oracle(pgmg, case):
    N, alpha, eps, dtype, cycles, rand, cfg, levels = case
    _check(pgmg, "W", N, cycles, dtype, eps, rand, levels, alpha=alpha, **cfg)


@gpu
@pytest.mark.parametrize("alpha,eps", [(2, 1e-4), (4, 1e-2)])
def test_alpha_three_calls_use_the_w_plans(pgmg, alpha, eps):
    """Calls of 1, 2 and 1 cycles on one context at N = 257 with four bulk levels: from the second
    call on the visits are planned from the previous call's (wplan_gamma = alpha, not 3)."""
    seen = []
    _check(pgmg, "W", 257, dtype="f64", eps=eps, calls=[1, 2, 1], levels=(4, 17), alpha=alpha,
           tail_n=17, after=lambda s: seen.append(s.spec_visit_modes()))
    print("W plan visit modes (no fire, fire, in-stream):", seen)


@gpu
@pytest.mark.parametrize("flag", ["PGMG_FLAG_NO_SPEC_FIRE", "PGMG_FLAG_EXACT_DIST"])
@pytest.mark.parametrize("N,alpha,eps,cfg,levels", [(129, 2, 1e-4, {}, (1, 65)),
                                                    (257, 4, 1e-2, {"tail_n": 17}, (4, 17))])
def test_alpha_without_speculation(pgmg, flag, N, alpha, eps, cfg, levels):
    """Every check decided in-stream (no W plans): the same results."""
    _check(pgmg, "W", N, 3, eps=eps, levels=levels, alpha=alpha, flags=getattr(pgmg, flag), **cfg)


# ---------------------------------------------------------------------------------------------
# n_coarse
# ---------------------------------------------------------------------------------------------
def _n_coarse_grid():
    cases, i = [], 0
    for N in (65, 129):
        for kind in ("V", "W", "F"):
            for n_coarse in (3, 9, 17):
                for dtype in ("f64", "f32"):
                    # every eps with every kind and n_coarse over the grid, mixed by position
                    cases.append((kind, N, n_coarse, EPS5[i % 5], dtype))
                    i += 3
    return cases


@gpu
@pytest.mark.parametrize("kind,N,n_coarse,eps,dtype", _n_coarse_grid())
def test_n_coarse_against_oracle(pgmg, kind, N, n_coarse, eps, dtype):
    """The generic tail_gcycle loop: tail_smooth as the coarsest solve at N = 3, 9, 17 (wave 0
    for 3 and 9, the whole workgroup for 17), 5x5 as an intermediate level above 3x3; the
    F-cycle's chain starting from an n_coarse x n_coarse grid."""
    levels = (0, 65) if N == 65 else (1, 65)
    _check(pgmg, kind, N, 3, dtype, eps, levels=levels, n_coarse=n_coarse)


N_COARSE_MIX = {"mixed": ("W", 65, 3, "f64", 1e-7, False, dict(alpha=2, n_coarse=3)),
                "all": ("V", 65, 3, "f32", 1e3, False, dict(n_coarse=3)),
                "none": ("W", 65, 3, "f64", 1e-7, False, dict(n_coarse=17))}


N_COARSE_PATHS = [
    # a random problem through the generic loop
    ("W", 65, 1e-7, "f64", True, dict(n_coarse=3), {}, (0, 65)),
    ("V", 129, 1e-2, "f32", True, dict(n_coarse=9), {}, (1, 65)),
    ("W", 129, 1e-4, "f64", True, dict(n_coarse=17), {}, (1, 65)),
    # tail_n below n_coarse is raised to it: the tail is the one 17x17 coarsest solve
    ("V", 129, 1e-7, "f64", False, dict(n_coarse=17), {"tail_n": 9}, (3, 17)),
    ("W", 129, 1e-4, "f64", False, dict(n_coarse=17), {"tail_n": 9}, (3, 17)),
    ("W", 129, 1e-2, "f32", False, dict(n_coarse=17), {"tail_n": 9}, (3, 17)),
    # the tail is one 65x65 coarsest solve (tail_smooth_rows<65> with coarse_iter + 1 sweeps)
    ("V", 129, 1e-7, "f64", False, dict(n_coarse=65), {}, (1, 65)),
    ("V", 129, 1e-2, "f32", False, dict(n_coarse=65), {}, (1, 65)),
    ("W", 129, 1e-4, "f64", False, dict(n_coarse=65), {}, (1, 65)),
    ("W", 129, 0.0, "f64", True, dict(n_coarse=65), {}, (1, 65)),
    # a one-level context larger than 5x5
    ("V", 33, 1e-7, "f64", False, dict(n_coarse=33), {}, (0, 33)),
    ("W", 33, 1e-4, "f32", False, dict(n_coarse=33), {}, (0, 33)),
    ("V", 33, 1e-4, "f64", False, dict(n_coarse=100), {}, (0, 33)),
    ("W", 33, 1e3, "f64", True, dict(n_coarse=100), {}, (0, 33)),
    # combined with alpha
    ("W", 65, 1e-7, "f64", False, dict(alpha=2, n_coarse=3), {}, (0, 65)),
    ("W", 129, 1e-4, "f32", False, dict(alpha=2, n_coarse=3), {}, (1, 65)),
    ("W", 65, 1e-2, "f64", False, dict(alpha=4, n_coarse=9), {}, (0, 65)),
    ("W", 129, 1e-4, "f64", False, dict(alpha=4, n_coarse=9), {}, (1, 65)),
    ("W", 65, 0.0, "f32", False, dict(alpha=4, n_coarse=17), {}, (0, 65)),
    ("W", 129, 1e-7, "f64", False, dict(alpha=4, n_coarse=17), {}, (1, 65)),
    ("W", 257, 1e3, "f64", False, dict(alpha=4, n_coarse=9), {"tail_n": 17}, (4, 17)),
]


@gpu
@pytest.mark.parametrize("kind,N,eps,dtype,rand,okw,cfg,levels", N_COARSE_PATHS)
def test_n_coarse_paths_against_oracle(pgmg, kind, N, eps, dtype, rand, okw, cfg, levels):
    _check(pgmg, kind, N, 3, dtype, eps, rand, levels, **okw, **cfg)


@gpu
@pytest.mark.parametrize("kind", ["V", "W"])
@pytest.mark.parametrize("n_coarse", [7, 8])
def test_n_coarse_between_grid_sizes_is_the_next_smaller(pgmg, kind, n_coarse):
    """n_coarse = 7 or 8 at N = 65: the recursion stops at the first N_l <= n_coarse, the 5x5
    level -- bitwise what n_coarse = 5 gives, on the device and in the oracle."""
    N = 65
    _check(pgmg, kind, N, 3, levels=(0, 65), n_coarse=n_coarse)
    assert _reference(kind, N, 3, "f64", 1e-7, False, _okw(dict(n_coarse=n_coarse)))[0][-1][1:] == \
        _reference(kind, N, 3, "f64", 1e-7, False, _okw(dict(n_coarse=5)))[0][-1][1:]
    got = [_single(pgmg, N, 3, kind=kind, n_coarse=n) for n in (n_coarse, 5)]
    assert_bitwise(got[0][0], got[1][0], f"{kind} n_coarse {n_coarse} vs 5")
    assert got[0][1] == got[1][1]


@gpu
@pytest.mark.parametrize("N,n_coarse,levels", [(257, 100, (2, 65)), (65, 1000, (0, 65)),
                                               (33, 33, (0, 33))])
def test_largest_legal_n_coarse(pgmg, N, n_coarse, levels):
    """The configurations next to the ones pgmg_create rejects (tests/test_capi.py): the tail's
    top is at most 65x65 and is the coarsest solve.  One V-cycle each."""
    _check(pgmg, "V", N, 1, levels=levels, n_coarse=n_coarse)


# ---------------------------------------------------------------------------------------------
# coarse_iter
# ---------------------------------------------------------------------------------------------
def _coarse_iter_grid():
    cases = []
    for kind, N in (("W", 65), ("V", 129)):
        for ci in (0, 1, 30, 100):
            for eps in (1e-7, 0.0, 1e3):
                cases.append((kind, N, ci, eps, "f64", {}))
            cases.append((kind, N, ci, 1e-7, "f32", {}))
        # the generic tail_smooth with a single coarsest sweep
        cases.append((kind, N, 0, 1e-7, "f64", dict(n_coarse=9)))
        cases.append((kind, N, 0, 1e3, "f32", dict(n_coarse=9)))
    return cases


@gpu
@pytest.mark.parametrize("kind,N,coarse_iter,eps,dtype,okw", _coarse_iter_grid())
def test_coarse_iter_against_oracle(pgmg, kind, N, coarse_iter, eps, dtype, okw):
    """coarse_iter = 0: tail_coarse5_regs' check loop never runs and tail_coarse5_gamma takes
    the sequential fallback; 30 and 100: long coarsest solves that end at a firing check."""
    levels = (0, 65) if N == 65 else (1, 65)
    _check(pgmg, kind, N, 3, dtype, eps, levels=levels, coarse_iter=coarse_iter, **okw)


@gpu
@pytest.mark.parametrize("kind,N,coarse_iter,dtype", [("W", 65, 30, "f64"), ("V", 129, 0, "f32"),
                                                      ("W", 129, 1, "f64")])
def test_coarse_iter_random_problem(pgmg, kind, N, coarse_iter, dtype):
    _check(pgmg, kind, N, 3, dtype, 1e-4, True, coarse_iter=coarse_iter)


COARSE_ITER_MIX = {"mixed": ("W", 65, 3, "f64", 1e-7, False, dict(coarse_iter=30)),
                   "all": ("W", 65, 3, "f64", 1e3, False, dict(coarse_iter=1)),
                   "none": ("W", 65, 3, "f64", 0.0, False, dict(coarse_iter=100))}


@pytest.mark.parametrize("family,mix", [("alpha", ALPHA_MIX), ("n_coarse", N_COARSE_MIX),
                                        ("coarse_iter", COARSE_ITER_MIX)])
def test_exit_mix_of_every_family(family, mix):
    """Each family runs a case whose smoother calls partly exit early (0 < early_exits <
    smooth_calls over its cycles), one where every call exits and one where none does: the
    oracle's counters of cases the GPU tests above run (CPU only)."""
    for want, (kind, N, cycles, dtype, eps, rand, okw) in mix.items():
        snaps, (exits, calls) = _reference(kind, N, cycles, dtype, eps, rand, _okw(okw))
        print(f"{family} {want}: {kind} N={N} eps={eps} {okw}: {exits} exits in {calls} calls")
        assert _mix(kind, N, cycles, dtype, eps, rand, **okw) == want, (family, want, exits, calls)


def test_exit_mix_cases_are_run_on_the_gpu():
    """The cases test_exit_mix_of_every_family names are cases of the GPU tests' tables."""
    alpha = {("W", c[0], c[4], c[3], c[2], c[5], c[1]) for c in ALPHA_CASES if not c[6]}
    for kind, N, cycles, dtype, eps, rand, okw in ALPHA_MIX.values():
        assert (kind, N, cycles, dtype, eps, rand, okw["alpha"]) in alpha
    grid = {(k, N, 3, d, e, False, n) for k, N, n, e, d in _n_coarse_grid()}
    for want in ("all", "none"):
        kind, N, cycles, dtype, eps, rand, okw = N_COARSE_MIX[want]
        assert (kind, N, cycles, dtype, eps, rand, okw["n_coarse"]) in grid
    kind, N, cycles, dtype, eps, rand, okw = N_COARSE_MIX["mixed"]
    assert (kind, N, eps, dtype, rand, okw, {}, (0, 65)) in N_COARSE_PATHS and cycles == 3
    ci = {(k, N, 3, d, e, False, c) for k, N, c, e, d, o in _coarse_iter_grid() if not o}
    for kind, N, cycles, dtype, eps, rand, okw in COARSE_ITER_MIX.values():
        assert (kind, N, cycles, dtype, eps, rand, okw["coarse_iter"]) in ci


# ---------------------------------------------------------------------------------------------
# the general path, FMG, row strips, the W plan counters
# ---------------------------------------------------------------------------------------------
GENERAL = dict(alpha=2, n_coarse=9, coarse_iter=3)


@gpu
@pytest.mark.parametrize("kind", ["V", "W"])
@pytest.mark.parametrize("variant", ["unfused", "v1=2,v2=0", "norecompute"])
@pytest.mark.parametrize("eps", [1e-7, 1e-2])
def test_general_path_variants(pgmg, kind, variant, eps):
    """(alpha 2, n_coarse 9, coarse_iter 3) at N = 129 on the other kernel sequences of the bulk
    level: one kernel per operation, other smoothing counts, no recomputed pre-smooth."""
    cfg = {"unfused": dict(flags=pgmg.PGMG_FLAG_UNFUSED), "v1=2,v2=0": dict(v1=2, v2=0),
           "norecompute": dict(flags=pgmg.PGMG_FLAG_NO_RECOMPUTE)}[variant]
    _check(pgmg, kind, 129, 3, eps=eps, levels=(1, 65), **GENERAL, **cfg)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_general_path_speculative_v_with_the_carry(pgmg, dtype):
    """cross_min_n = 33: the cross-cycle fused finest level, V calls speculative, each ending
    with the carry pass the next one starts from."""
    def after(s):
        assert s.stats_detail()[2] >= 0, "cross-cycle fusion not active"
        assert s.dist_info()[0], "V calls not speculative"
        info, rollbacks = s.carry_info(), s.dist_info()[1]
        print("carry (used, made, dropped):", info, "rollbacks:", rollbacks)
        assert info[1] + info[2] >= 1 or rollbacks >= 1, (info, rollbacks)

    _check(pgmg, "V", 129, dtype=dtype, calls=[1, 1, 2], levels=(1, 65), after=after,
           cross_min_n=33, **GENERAL)


@functools.lru_cache(maxsize=None)
def _fmg_model(N, dtype, n_coarse, coarse_iter, own_f):
    o = oracle.Oracle(dtype=dtype, n_coarse=n_coarse, coarse_iter=coarse_iter)
    f = oracle.rhs_mt64(N, seed=99, dtype=dtype) if own_f else o.rhs(N)
    u = fmg_model.fmg(o, np.ascontiguousarray(f, dtype=o.dt), 2).astype(np.float64)
    u.setflags(write=False)
    return u, o.sweeps, o.cut_exits, f.astype(np.float64)


@gpu
@pytest.mark.parametrize("own_f", [False, True], ids=["analytic", "own_f"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("coarse_iter", [0, 30])
@pytest.mark.parametrize("n_coarse", [9, 17])
def test_fmg_coarsest_start(pgmg, n_coarse, coarse_iter, dtype, own_f):
    """pgmg_fmg(2) against tests/fmg_model.py: the climb starts from a 9x9 or 17x17 level solved
    by two coarsest smoother calls of coarse_iter + 1 sweeps."""
    N = 129
    want, sweeps, cut, f = _fmg_model(N, dtype, n_coarse, coarse_iter, own_f)
    with pgmg.Solver(N, dtype=dtype, n_coarse=n_coarse, coarse_iter=coarse_iter) as s:
        assert s.levels() == (1, 65)
        s.set_problem(None, f if own_f else None)
        s.fmg(2)
        assert_bitwise(s.solution(), want, f"fmg n_coarse={n_coarse} coarse_iter={coarse_iter} {dtype}")
        assert s.stats() == (sweeps, cut), (s.stats(), sweeps, cut)


@gpu
def test_fmg_n_coarse_3_is_still_an_error(pgmg):
    with pgmg.Solver(129, n_coarse=3, alpha=2, coarse_iter=30) as s:
        s.set_problem()
        with pytest.raises(pgmg.PgmgError):
            s.fmg(2)


@gpu
def test_strips_wcycle_alpha_2_n_coarse_9(pgmg):
    """Two ranks (loopback), N = 129: level 0 on row strips, the 65x65 and 33x33 levels gathered
    (run_gathered with gamma = 2), a 17x17 tail above the 9x9 coarsest level -- bitwise the
    single-GPU result and the oracle's."""
    N, cycles = 129, 3
    cfg = dict(gather_n=65, tail_n=17, alpha=2, n_coarse=9)
    assert pgmg.plan_strips(N, 2, 0, tail_n=17, gather_n=65)[2] == 1   # level 0 is distributed
    snaps, _ = _reference("W", N, cycles, "f64", 1e-7, False, _okw(cfg))
    ref = _single(pgmg, N, cycles, kind="W", **cfg)
    assert_bitwise(ref[0], snaps[-1][0], "single GPU vs oracle")
    assert ref[1] == snaps[-1][1:]
    outs = _run_ranks(pgmg, 2, N, cycles, kind="W", **cfg)
    for r, (phi, stats, _) in enumerate(outs):
        assert_bitwise(phi, ref[0], f"rank {r} of 2")
    assert outs[0][1] == ref[1]


@gpu
@pytest.mark.parametrize("alpha", [2, 4])
def test_w_plan_visit_counters(pgmg, alpha):
    """pgmg_spec_visit_modes.  The counter (pgmg_cycle.hip, w_visit_mode) counts, in the segments
    of a W call that are enqueued speculatively, one visit per bulk level l >= 1 -- level 0's
    visit is not planned and not counted, a rollback's in-stream rerun adds nothing.  So for a
    call of k cycles that is not rolled back the three counts sum to
    k * (alpha + alpha^2 + .. + alpha^(bulk levels - 1)): the bulk-level visits below the finest
    level.  After a V call the counts are zero."""
    N, eps = 257, 1e-7
    snaps, _ = _reference("W", N, 3, "f64", eps, False, _okw(dict(alpha=alpha)))
    with pgmg.Solver(N, eps=eps, alpha=alpha, tail_n=17) as s:
        nb, top = s.levels()
        assert (nb, top) == (4, 17)
        per_cycle = sum(alpha ** l for l in range(1, nb))
        s.set_problem()
        assert s.spec_visit_modes() == (0, 0, 0)
        done = 0
        for k in (1, 2):
            rb0 = s.dist_info()[1]
            s.wcycle(k)
            done += k
            counts = s.spec_visit_modes()
            print(f"alpha={alpha} call of {k}: (no fire, fire, in-stream) = {counts}")
            assert_bitwise(s.solution(), snaps[done - 1][0], f"W alpha={alpha} cycle {done}")
            if s.dist_info()[1] == rb0:
                assert sum(counts) == k * per_cycle, (counts, k, per_cycle)
            else:   # rolled back: the speculative segment's visits, no more
                assert 0 < sum(counts) <= k * per_cycle, (counts, k, per_cycle)
        s.vcycle(1)
        assert s.spec_visit_modes() == (0, 0, 0)
