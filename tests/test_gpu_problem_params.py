"""a, p, q and h0 off their defaults (1, 1, 1, 0) on every path, against the oracle.

pgmg_config's four problem-defining fields: the domain edge a, the wave numbers p and q of the
analytic right-hand side and exact solution, and the caller's mesh width h0.  With the defaults
every run is symmetric under transposition (p = q: sx == sy) and the sine tables are ~1e-16 on
the far boundary, so a mix-up of the x and y tables, a row offset applied to the wrong table or
a wrong boundary term changes no bit.  The parameter sets below break both; the paths are the
ones that read the tables: the tail's fmg_factor * sx[i] * sy[j], the bulk level's stored f,
k_postpre regenerating f from gfx / gsy (and its carry and rare paths), device-bound analytic
problems, the F-cycle's per-level tables and own chain of mesh widths, pgmg_fmg's climb with
h0 * 2^l, the monitor's exact solution, row strips, and the op-level pgmg_rhs.

The checker is the CPU oracle (oracle/pgmg_oracle.c), pinned to the reference's own code for
a, p, q and h by tests/test_oracle_golden.py (tests/golden/cycles_problem.json).  Tolerance:
EXACT for phi and the statistics (see tests/test_gpu_cycle_params.py); the monitor's norms by
the project's rule, solve_rule.close (two summation orders of the same terms).

      a     p     q
P1    1     2     3     asymmetric: a table mix-up shows
P2    2     1     1     dyadic a != 1
P3    3     2     1     non-dyadic a: i * h rounds
P4    0.5   3     5     a < 1, higher modes
P5    1     0.5   1.5   non-integer: f and u are O(1) on column and row N - 1
P6    1     -1    2     negative wave number
P7    1     0     1     f = 0: every check fires at once, all norms 0
P8    1     N-2   1     one undamped Jacobi sweep annihilates this mode: the residual norms sit
                        at rounding level, next to eps
P9    1000  2     2     f ~ 1e-5: checks fire where the defaults' do not
P10   1e-3  1     1     f ~ 2e7: no check fires
NEG   -2    1     2     h < 0, h * h > 0
H1: h0 = 0.7 / (N - 1); H2: h0 = 1 / N; H3: h0 = 1 (every check fires).

Sizes: N <= 257 and 2-4 cycles (the monitor also at 513: its first full tile); every case
asserts the path it is there for.
"""
import functools
import math

import numpy as np
import pytest

import fmg_model
import oracle
from conftest import assert_bitwise
from solve_rule import close, norm_tol, oracle_res_norm
from test_gpu_cycle_params import _check, _mix, _okw, _problem, _reference
from test_gpu_strips import _run_ranks, _single

gpu = pytest.mark.gpu

SETS = {"P1": (1.0, 2.0, 3.0), "P2": (2.0, 1.0, 1.0), "P3": (3.0, 2.0, 1.0), "P4": (0.5, 3.0, 5.0),
        "P5": (1.0, 0.5, 1.5), "P6": (1.0, -1.0, 2.0), "P7": (1.0, 0.0, 1.0), "P8": (1.0, None, 1.0),
        "P9": (1000.0, 2.0, 2.0), "P10": (1e-3, 1.0, 1.0), "NEG": (-2.0, 1.0, 2.0),
        "P0": (1.0, 1.0, 1.0)}
EPS3 = [1e-7, 1e-2, 1e-4]


def prm(name, N):
    """pgmg_config / oracle fields of a set name: "P1", "P5+H1", ..."""
    s, _, h = name.partition("+")
    a, p, q = SETS[s]
    d = dict(a=a, p=float(N - 2) if p is None else p, q=q)
    if h:
        d["h0"] = {"H1": 0.7 / (N - 1), "H2": 1.0 / N, "H3": 1.0}[h]
    return d


def _h(N, kw):
    """the context's finest mesh width"""
    return kw.get("h0") or kw["a"] / (N - 1)


def _oracle(N, name, dtype="f64", eps=1e-7, **kw):
    """(oracle, h, f) of a set"""
    d = prm(name, N)
    h = _h(N, d)
    d.pop("h0", None)
    o = oracle.Oracle(eps=eps, dtype=dtype, **d, **kw)
    return o, h, o.rhs(N, h)


def _f64(x):
    x = x.astype(np.float64)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------
# a. the tail alone (N = 33, 65): fmg_factor * sx[i] * sy[j], every set, V, W and F
# ---------------------------------------------------------------------------------------------
def _tail_cases():
    """(kind, N, set, eps, dtype): every set with every kind at both sizes in fp64, eps mixed by
    position; every set with every kind once in fp32; then the cases the conditions on the
    inputs name (test_exit_mix_of_every_family, test_precision_split)."""
    cases, i = [], 0
    names = [n for n in SETS if n != "P0"]
    for kind in ("V", "W", "F"):
        for name in names:
            for N in (33, 65):
                cases.append((kind, N, name, EPS3[i % 3], "f64"))
                i += 1
            cases.append((kind, (33, 65)[i % 2], name, EPS3[(i + 1) % 3], "f32"))
            i += 2
    for kind in ("V", "W"):
        for N in (33, 65):
            for name in ("P1+H1", "P5+H1", "P1+H2", "P5+H2"):
                cases.append((kind, N, name, EPS3[i % 3], "f64" if (i // 3) % 2 == 0 else "f32"))
                i += 1
    cases += [("F", 65, "P1+H1", 1e-7, "f64"), ("F", 33, "P5+H2", 1e-4, "f32")]
    for c in [x[:5] for x in MIX_CASES] + list(SPLIT):
        if c not in cases:
            cases.append(c)
    return cases


# (kind, N, set, eps, dtype, the exits' mix over three cycles): the oracle's counters decide
MIX_CASES = [("V", 65, "P1", 1e-7, "f64", "none"), ("V", 65, "P4", 1e-7, "f64", "mixed"),
             ("V", 65, "P9", 1e-2, "f64", "all"), ("V", 65, "P7", 1e-4, "f64", "all"),
             ("W", 65, "P0+H1", 1e-7, "f64", "mixed"), ("V", 65, "P0+H3", 1e-7, "f64", "all"),
             ("V", 65, "P10", 1e-7, "f64", "none"), ("V", 65, "P1+H1", 1e-7, "f64", "none")]
MIX_FAMILIES = {"a": ("P10", "P4", "P9"), "p/q": ("P1", "P4", "P7"), "h0": ("P1+H1", "P0+H1", "P0+H3")}
# P8 at N = 65 (p = 63): fp64 fires every check, fp32 none
SPLIT = (("V", 65, "P8", 1e-7, "f64"), ("V", 65, "P8", 1e-7, "f32"))
TAIL_CASES = _tail_cases()


def _id(c):
    return "-".join(str(x) for x in c)


@gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_tail_against_oracle(pgmg, case):
    kind, N, name, eps, dtype = case
    _check(pgmg, kind, N, 3, dtype, eps, levels=(0, N), **prm(name, N))


# ---------------------------------------------------------------------------------------------
# b. one bulk level (N = 129, 2D LDS tiles) and its other kernel sequences
# ---------------------------------------------------------------------------------------------
BULK_SETS = ["P1", "P3", "P5", "P1+H1", "P5+H2"]
BULK_VARIANTS = ["default", "noctile", "unfused", "v1=2,v2=0", "norecompute"]


def _bulk_cases():
    cases, i = [], 0
    for variant in BULK_VARIANTS:
        for kind in ("V", "W"):
            for name in BULK_SETS:
                cases.append((variant, kind, name, EPS3[i % 3], "f64"))
                if name in ("P1", "P5", "P1+H1") or variant == "default":
                    cases.append((variant, kind, name, EPS3[(i + 1) % 3], "f32"))
                i += 1
    cases += [("default", "V", "P9", 1e-2, "f64"), ("default", "W", "P4", 1e-7, "f64"),
              ("default", "V", "P7", 1e-7, "f32"), ("default", "W", "P8", 1e-7, "f64"),
              ("default", "V", "P10", 1e-7, "f64"), ("default", "V", "NEG", 1e-4, "f64"),
              ("default", "W", "P6", 1e-7, "f32"), ("default", "V", "P2", 1e-7, "f64")]
    return cases


@gpu
@pytest.mark.parametrize("case", _bulk_cases(), ids=_id)
def test_bulk_level_against_oracle(pgmg, case):
    variant, kind, name, eps, dtype = case
    N = 129
    cfg = {"default": {}, "noctile": dict(flags=pgmg.PGMG_FLAG_NO_CTILE),
           "unfused": dict(flags=pgmg.PGMG_FLAG_UNFUSED), "v1=2,v2=0": dict(v1=2, v2=0),
           "norecompute": dict(flags=pgmg.PGMG_FLAG_NO_RECOMPUTE)}[variant]

    def after(s):
        assert s.fused == (variant not in ("unfused", "v1=2,v2=0"))
        assert s.stats_detail()[2] == -1, "cross-fused: not the path this case is for"
        assert s.dist_info()[0] is False

    _check(pgmg, kind, N, 3, dtype, eps, levels=(1, 65), after=after, **cfg, **prm(name, N))


# ---------------------------------------------------------------------------------------------
# c. the cross-fused finest level: k_postpre regenerating f from gfx / gsy
# ---------------------------------------------------------------------------------------------
CROSS_SETS = ["P1", "P3", "P5", "P5+H1", "P1+H2"]


def _cross_cases():
    cases, i = [], 0
    for N in (129, 257):
        for name in CROSS_SETS:
            for calls in ((3,), (1, 1, 1), (2, 1)):
                cases.append((N, name, calls, EPS3[i % 3] if i % 2 else 1e-7,
                              "f64" if (i + i // 3) % 3 else "f32"))
                i += 1
    return cases


def _cross_after(pgmg, calls, flags=0, rhs="regenerated", kind="V"):
    def after(s):
        assert s.fused and s.stats_detail()[2] >= 0, "cross-cycle fusion not active"
        assert s.fine_pass_bytes(3) < s.fine_pass_bytes(0) if rhs == "regenerated" else \
            s.fine_pass_bytes(3) >= s.fine_pass_bytes(0), "k_postpre's f: not the path meant"
        spec, rollbacks = s.dist_info()
        assert spec == (not flags & pgmg.PGMG_FLAG_EXACT_DIST)
        took, made, dropped = s.carry_info()
        if flags & pgmg.PGMG_FLAG_NO_CARRY:
            assert (took, made) == (0, 0), (took, made, dropped)
        elif kind == "V" and len(calls) > 1 and spec:
            # every speculative V call ends with the carry pass, and the next call starts from
            # it, unless a call was rolled back
            print("carry (used, made, dropped):", took, made, dropped, "rollbacks", rollbacks)
            assert took > 0 or rollbacks > 0, (took, made, dropped, rollbacks)
    return after


@gpu
@pytest.mark.parametrize("case", _cross_cases(), ids=_id)
def test_cross_fused_against_oracle(pgmg, case):
    """V calls [3], [1, 1, 1] and [2, 1] with cross_min_n = 33: k_pre, k_postpre, the carry."""
    N, name, calls, eps, dtype = case
    _check(pgmg, "V", N, dtype=dtype, eps=eps, calls=calls, levels=(N // 128, 65),
           after=_cross_after(pgmg, calls), cross_min_n=33, **prm(name, N))


CARRY_CASES = [(257, "P1", "f64"), (257, "P5+H1", "f64"), (129, "P5", "f32"), (257, "P1+H1", "f32")]


@gpu
@pytest.mark.parametrize("N,name,dtype", CARRY_CASES)
def test_cross_one_cycle_calls_take_the_carry(pgmg, N, name, dtype):
    """Four one-cycle calls: at least one of them starts from the carry, whatever was rolled
    back (carry_info[0] > 0)."""
    def after(s):
        took, made, dropped = s.carry_info()
        print("carry (used, made, dropped):", took, made, dropped, "rollbacks", s.dist_info()[1])
        assert took > 0, (took, made, dropped)

    _check(pgmg, "V", N, dtype=dtype, calls=[1, 1, 1, 1], levels=(N // 128, 65), after=after,
           cross_min_n=33, **prm(name, N))


AGREE_CASES = [("P1", "f64"), ("P3", "f32"), ("P5", "f64"), ("P5+H1", "f64"), ("P1+H2", "f32")]


@gpu
@pytest.mark.parametrize("kind", ["V", "W"])
@pytest.mark.parametrize("name,dtype", AGREE_CASES)
def test_cross_regenerated_stored_and_uncrossed_agree(pgmg, kind, name, dtype):
    """k_postpre regenerating f, streaming the stored f (PGMG_FLAG_STORED_RHS) and the level
    not cross-fused (PGMG_FLAG_NO_CROSS): all three bitwise the oracle."""
    N = 129
    for flags, rhs in ((0, "regenerated"), (pgmg.PGMG_FLAG_STORED_RHS, "stored")):
        _check(pgmg, kind, N, dtype=dtype, calls=[2, 1], levels=(1, 65), flags=flags,
               after=_cross_after(pgmg, [2, 1], flags, rhs, kind), cross_min_n=33, **prm(name, N))

    def uncrossed(s):
        assert s.fused and s.stats_detail()[2] == -1

    _check(pgmg, kind, N, dtype=dtype, calls=[2, 1], levels=(1, 65), after=uncrossed,
           flags=pgmg.PGMG_FLAG_NO_CROSS, cross_min_n=33, **prm(name, N))


FLAG_CASES = [(129, "P1", "f64"), (257, "P3", "f64"), (129, "P5", "f32"), (257, "P5+H1", "f64")]
FLAG_CALLS = (("V", [1, 1, 2]), ("W", [2, 1]))


@gpu
@pytest.mark.parametrize("flag", ["PGMG_FLAG_NO_CARRY", "PGMG_FLAG_EXACT_DIST", "PGMG_FLAG_NO_GRAPH"])
@pytest.mark.parametrize("N,name,dtype", FLAG_CASES)
def test_cross_fused_flags(pgmg, flag, N, name, dtype):
    flags = getattr(pgmg, flag)
    for kind, calls in FLAG_CALLS:
        _check(pgmg, kind, N, dtype=dtype, calls=calls, levels=(N // 128, 65), flags=flags,
               after=_cross_after(pgmg, calls, flags, kind=kind), cross_min_n=33, **prm(name, N))


RARE_SETS = ["P5", "P5+H1"]
RARE_EPS = [10 ** (k / 12.0) for k in range(96, -24, -1)]


@gpu
@pytest.mark.parametrize("name", RARE_SETS)
def test_cross_rare_paths_regenerated_rhs(pgmg, name):
    """P5 with a random phi0 whose boundary is non-zero and the regenerated f, eps swept as
    test_cross_rare_paths_nonzero_boundary does until both k_postpre rare paths have run."""
    N = 129
    kw = prm(name, N)
    seen = [0, 0]

    def after(s):
        d = s.stats_detail()
        assert d[2] >= 0 and s.fine_pass_bytes(3) < s.fine_pass_bytes(0)
        seen[0] += d[2]
        seen[1] += d[3]

    for eps in RARE_EPS:
        if seen[0] > 0 and seen[1] > 0:
            break
        _check(pgmg, "V", N, eps=eps, rand="phi", calls=[6], levels=(3, 17), after=after,
               tail_n=17, cross_min_n=33, **kw)
    assert seen[0] > 0 and seen[1] > 0, seen


# ---------------------------------------------------------------------------------------------
# d. device-bound analytic problems: set_problem_device(phi, None)
# ---------------------------------------------------------------------------------------------
DEVICE_SETS = ["P1", "P3", "P5", "P5+H1"]


@gpu
@pytest.mark.parametrize("kind", ["V", "W"])
@pytest.mark.parametrize("binding", ["inplace", "staged", "staged-f32"])
@pytest.mark.parametrize("name", DEVICE_SETS)
def test_device_bound_analytic(pgmg, kind, binding, name):
    import torch
    N = 129
    dtype = "f32" if binding == "staged-f32" else "f64"
    kw = prm(name, N)
    snaps, _ = _reference(kind, N, 3, dtype, 1e-7, "phi", _okw(kw))
    phi0, _ = _problem(N, dtype, "phi")
    o, h, f = _oracle(N, name, dtype)
    with pgmg.Solver(N, dtype=dtype, cross_min_n=33, **kw) as s:
        assert s.levels() == (1, 65) and s.stats_detail()[2] >= 0
        if binding == "inplace":
            g = pgmg.DeviceGrid(N, phi0)
            read = g.download
        else:
            g = torch.from_numpy(phi0).cuda()
            torch.cuda.synchronize()
            read = lambda: g.cpu().numpy()
        s.set_problem_device(g, None)
        assert s.device_info() == (True, binding == "inplace")
        run = s.vcycle if kind == "V" else s.wcycle
        for done, n in ((2, 2), (3, 1)):
            run(n)
            s.sync()
            phi, sweeps, cut = snaps[done - 1]
            assert_bitwise(read(), phi, f"{kind} {binding} {name} cycle {done}")
            assert s.stats() == (sweeps, cut)
        _monitor_check(s, o, h, f, dtype, N, snaps[-1][0], f"{kind} {binding} {name}")
        if binding == "inplace":
            g.close()


# ---------------------------------------------------------------------------------------------
# e. the F-cycle: per-level tables, its own chain of mesh widths
# ---------------------------------------------------------------------------------------------
F_VARIANTS = ["default", "nopin", "nor2", "stored", "exact", "n_coarse=9"]


def _f_cfg(pgmg, variant):
    return {"default": {}, "nopin": dict(flags=pgmg.PGMG_FLAG_NO_PIN),
            "nor2": dict(flags=pgmg.PGMG_FLAG_NO_R2), "stored": dict(flags=pgmg.PGMG_FLAG_STORED_RHS),
            "exact": dict(flags=pgmg.PGMG_FLAG_EXACT_DIST), "n_coarse=9": dict(n_coarse=9)}[variant]


def _f_cases():
    cases, i = [], 0
    for variant in F_VARIANTS:
        for N in (129, 257):
            for name in ("P1", "P2", "P3", "P5", "P1+H1"):
                dtype = "f32" if i % 3 == 2 else "f64"
                cases.append((variant, N, name, EPS3[i % 3] if i % 2 else 1e-7, dtype))
                i += 1
    return cases


@gpu
@pytest.mark.parametrize("case", _f_cases(), ids=_id)
def test_fcycle_against_oracle(pgmg, case):
    """Calls of 1 and 2 F-cycles (the second: consecutive F-cycles in one call); cross_min_n =
    33, so the climb's finest level regenerates f from the F chain's tables (fmg_gtab).  P2 and
    P3: the chain starts at 1 / (n_coarse - 1) whatever a is."""
    variant, N, name, eps, dtype = case
    cfg = _f_cfg(pgmg, variant)

    def after(s):
        assert s.fused and s.stats_detail()[2] >= 0
        assert s.dist_info()[0] == (variant != "exact")
        # the F-cycle ran on its own chain; the problem's f and exact solution are still the
        # ones at the context's h (the residual of the F result against the level-0 f)
        o, h, f = _oracle(N, name, dtype)
        _monitor_check(s, o, h, f, dtype, N, s.solution(), f"F {case}")

    _check(pgmg, "F", N, dtype=dtype, eps=eps, calls=[1, 2], levels=(N // 128, 65), after=after,
           cross_min_n=33, **cfg, **prm(name, N))


F_PLAIN_SETS = ["P1", "P3", "P5"]


@gpu
@pytest.mark.parametrize("name", F_PLAIN_SETS)
def test_fcycle_default_plan_one_bulk_level(pgmg, name):
    """Without cross fusion (the default plan at N = 129), two consecutive F calls."""
    def after(s):
        assert s.stats_detail()[2] == -1

    _check(pgmg, "F", 129, calls=[1, 1], levels=(1, 65), after=after, **prm(name, 129))


@functools.lru_cache(maxsize=None)
def _vfvw_reference(N, name, dtype):
    o, h, f = _oracle(N, name, dtype)
    phi = np.zeros((N, N), dtype=o.dt)
    snaps = []
    for kind in "VFVWF":
        if kind == "F":
            o.f_cycle_outer(phi)
        else:
            (o.v_cycle if kind == "V" else o.w_cycle)(phi, f, h)
        snaps.append((_f64(phi), o.sweeps, o.cut_exits))
    return snaps


HANDS_CASES = [(129, "P1+H1", "f64"), (257, "P5+H1", "f64"), (129, "P5+H2", "f32"),
               (257, "P3+H2", "f64")]


@gpu
@pytest.mark.parametrize("cross", [False, True], ids=["plain", "cross"])
@pytest.mark.parametrize("N,name,dtype", HANDS_CASES)
def test_fcycle_hands_h0_back(pgmg, cross, N, name, dtype):
    """V, F, V, W, F on one context with h0 set: pgmg_fcycle overwrites h on every level with
    its own chain and its guard restores the caller's, so the V and W calls after it are the
    oracle's v_cycle(h0) / w_cycle(h0) again."""
    snaps = _vfvw_reference(N, name, dtype)
    cfg = dict(cross_min_n=33) if cross else {}
    with pgmg.Solver(N, dtype=dtype, **cfg, **prm(name, N)) as s:
        assert s.levels() == (N // 128, 65)
        assert (s.stats_detail()[2] >= 0) == cross
        s.set_problem()
        for k, kind in enumerate("VFVWF"):
            {"V": s.vcycle, "W": s.wcycle, "F": s.fcycle}[kind](1)
            phi, sweeps, cut = snaps[k]
            assert_bitwise(s.solution(), phi, f"{name} N={N} {dtype} call {k} ({kind})")
            assert s.stats() == (sweeps, cut), (k, kind, s.stats(), sweeps, cut)


# ---------------------------------------------------------------------------------------------
# f. pgmg_fmg: the climb with h0 * 2^l
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fmg_reference(N, name, nu, dtype):
    o, h, f = _oracle(N, name, dtype)
    u = fmg_model.fmg(o, f, nu, h)
    out = [(_f64(u), o.sweeps, o.cut_exits)]
    for _ in range(2):
        o.v_cycle(u, f, h)
    out.append((_f64(u), o.sweeps, o.cut_exits))
    return out


FMG_CASES = [(65, "P1", "f64"), (65, "P5+H1", "f32"), (129, "P1", "f32"), (129, "P3", "f64"),
             (129, "P5", "f64"), (129, "P1+H1", "f64"), (257, "P1", "f64"), (257, "P3", "f32"),
             (257, "P5", "f64"), (257, "P5+H1", "f64")]


@gpu
@pytest.mark.parametrize("bound", [False, True], ids=["owned", "device-bound"])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("N,name,dtype", FMG_CASES)
def test_fmg_against_model(pgmg, N, name, dtype, nu, bound):
    """Bitwise fmg_model.fmg(o, o.rhs(N, h), nu, h0), then two V-cycles from the result."""
    kw = prm(name, N)
    (u0, sw0, cut0), (u2, sw2, cut2) = _fmg_reference(N, name, nu, dtype)
    levels = (0, 65) if N == 65 else (N // 128, 65)
    with pgmg.Solver(N, dtype=dtype, cross_min_n=33, **kw) as s:
        assert s.levels() == levels and (s.stats_detail()[2] >= 0) == (N > 65)
        if bound:
            rng = np.random.default_rng(N)
            g = pgmg.DeviceGrid(N, rng.standard_normal((N, N)))     # fmg ignores the current phi
            s.set_problem_device(g, None)
            assert s.device_info() == (True, N > 65 and dtype == "f64")
            read = g.download
        else:
            s.set_problem()
            read = s.solution
        s.fmg(nu)
        s.sync()
        assert_bitwise(read(), u0, f"fmg({nu}) N={N} {name} {dtype}")
        assert s.stats() == (sw0, cut0), (s.stats(), sw0, cut0)
        s.vcycle(2)
        s.sync()
        assert_bitwise(read(), u2, f"fmg({nu}) + 2 V N={N} {name} {dtype}")
        assert s.stats() == (sw2, cut2), (s.stats(), sw2, cut2)
        if bound:
            g.close()


# ---------------------------------------------------------------------------------------------
# g. the monitor and pgmg_solve: the exact solution at the context's h
# ---------------------------------------------------------------------------------------------
def _close2(got, want, N):
    """two device results of the same sums in two decompositions (ranks against one GPU): each
    within norm_tol(N) relative of the sequential sum, so within twice that of each other"""
    return abs(got - want) <= 2.0 * norm_tol(N) * abs(want)


def _monitor_check(s, o, h, f, dtype, N, phi, what):
    """pgmg_monitor of the current iterate (phi: its download) against the oracle's residual
    norm, rel_error and exact norm at the context's h."""
    want_res = oracle_res_norm(oracle, phi, f, dtype, h)
    want_u = oracle.norm(o.exact(N, h))
    want_rel = o.rel_error(np.ascontiguousarray(phi, dtype=o.dt), h)
    e = np.asarray(phi, dtype=np.float64) - o.exact(N, h)
    want_err = oracle.norm(e)
    m = s.monitor()
    me = s.monitor(error=True)
    print(f"{what}: res {me.res_norm!r} / {want_res!r}  rel {me.rel_error!r} / {want_rel!r}  "
          f"|u| {me.exact_norm!r} / {want_u!r}  |e| {me.err_norm!r} / {want_err!r}")
    assert close(m.res_norm, want_res, N), (what, m.res_norm, want_res)
    assert math.isnan(m.err_norm) and math.isnan(m.rel_error) and math.isnan(m.exact_norm)
    assert np.float64(me.res_norm).view(np.uint64) == np.float64(m.res_norm).view(np.uint64)
    assert close(me.exact_norm, want_u, N), (what, me.exact_norm, want_u)
    assert close(me.err_norm, want_err, N), (what, me.err_norm, want_err)
    if want_u == 0.0:
        # p = 0: u = 0 at every point, so the header's rel_error = err_norm / exact_norm is
        # x / 0: NaN for phi = 0 (0 / 0), +Inf otherwise -- what the oracle's division gives
        assert me.exact_norm == 0.0
        assert (math.isnan(me.rel_error) and math.isnan(want_rel)) or me.rel_error == want_rel == math.inf
        assert math.isnan(me.rel_error) == (want_err == 0.0)
    else:
        assert close(me.rel_error, want_rel, N), (what, me.rel_error, want_rel)
        assert me.rel_error == me.err_norm / me.exact_norm


def _monitor_cases():
    cases = []
    for N in (33, 129, 513):
        for i, name in enumerate(("P1", "P3", "P5", "P7", "P5+H1")):
            for stored in (False, True):
                dtype = "f32" if (i + stored + N // 128) % 3 == 0 else "f64"
                cases.append((N, name, "stored" if stored else "regenerated", dtype))
    return cases


@gpu
@pytest.mark.parametrize("case", _monitor_cases(), ids=_id)
def test_monitor_against_oracle(pgmg, case):
    """monitor() and monitor(error=True) after 0, 1 and 3 V-cycles and on a random phi0 with a
    non-zero boundary; P7: exact_norm == 0 and res_norm == 0 on phi = 0."""
    N, name, fkind, dtype = case
    kw = prm(name, N)
    o, h, f = _oracle(N, name, dtype)
    snaps, _ = _reference("V", N, 3, dtype, 1e-7, False, _okw(kw))
    phi0, _ = _problem(N, dtype, "phi")
    flags = pgmg.PGMG_FLAG_STORED_RHS if fkind == "stored" else 0
    cfg = dict(cross_min_n=33) if N >= 129 else {}
    with pgmg.Solver(N, dtype=dtype, flags=flags, **cfg, **kw) as s:
        assert (s.stats_detail()[2] >= 0) == (N >= 129)
        s.set_problem()
        _monitor_check(s, o, h, f, dtype, N, np.zeros((N, N)), f"{case} zero")
        if name == "P7":
            m = s.monitor(error=True)
            assert m.res_norm == 0.0 and m.exact_norm == 0.0 and m.err_norm == 0.0
            assert math.isnan(m.rel_error)
        s.vcycle(1)
        assert_bitwise(s.solution(), snaps[0][0], f"{case} V1")
        _monitor_check(s, o, h, f, dtype, N, snaps[0][0], f"{case} V1")
        s.vcycle(2)
        assert_bitwise(s.solution(), snaps[2][0], f"{case} V3")
        _monitor_check(s, o, h, f, dtype, N, snaps[2][0], f"{case} V3")
        s.set_problem(phi0, None)
        _monitor_check(s, o, h, f, dtype, N, phi0, f"{case} random")


MON_BOUND_CASES = [(129, "P1", "f64"), (513, "P5", "f64"), (129, "P5+H1", "f32"), (33, "P3", "f64")]


@gpu
@pytest.mark.parametrize("N,name,dtype", MON_BOUND_CASES)
def test_monitor_device_bound(pgmg, N, name, dtype):
    """The monitor reads a bound array where it lies: a random phi0 with a non-zero boundary,
    in place (fp64, cross-fused) or staged."""
    kw = prm(name, N)
    o, h, f = _oracle(N, name, dtype)
    phi0, _ = _problem(N, dtype, "phi")
    with pgmg.DeviceGrid(N, phi0) as g, pgmg.Solver(N, dtype=dtype, cross_min_n=33, **kw) as s:
        s.set_problem_device(g, None)
        assert s.device_info() == (True, N >= 129 and dtype == "f64")
        _monitor_check(s, o, h, f, dtype, N, phi0, f"bound {N} {name} {dtype}")


SOLVE_CASES = [(129, "P1", "V", "f64"), (129, "P1", "W", "f32"), (257, "P1", "V", "f64"),
               (129, "P5+H1", "V", "f64"), (65, "P1", "F", "f64")]
SOLVE_CYCLES = 4


@gpu
@pytest.mark.parametrize("N,name,cycle,dtype", SOLVE_CASES)
def test_solve_history_against_oracle(pgmg, N, name, cycle, dtype):
    """pgmg_solve with monitor = PGMG_MON_ERROR: every pgmg_history entry (cycles, residual
    norm, rel_error) against the oracle after that many cycles."""
    kw = prm(name, N)
    o, h, f = _oracle(N, name, dtype)
    cycles = SOLVE_CYCLES
    snaps, _ = _reference(cycle, N, cycles, dtype, 1e-7, False, _okw(kw))
    cfg = dict(cross_min_n=33) if N >= 129 else {}
    with pgmg.Solver(N, dtype=dtype, **cfg, **kw) as s:
        s.set_problem()
        info = s.solve(cycle=cycle, rtol=0.0, max_cycles=cycles, error=True)
        assert (info.cycles, info.checks) == (cycles, cycles + 1)
        assert [k for k, _, _ in info.history] == list(range(cycles + 1))
        assert_bitwise(s.solution(), snaps[-1][0], f"solve {cycle} {N} {name}")
        assert s.stats() == snaps[-1][1:]
    for k, res, rel in info.history:
        phi = np.zeros((N, N)) if k == 0 else snaps[k - 1][0]
        want_res = oracle_res_norm(oracle, phi, f, dtype, h)
        want_rel = o.rel_error(np.ascontiguousarray(phi, dtype=o.dt), h)
        print(f"check {k}: res {res!r} / {want_res!r} rel {rel!r} / {want_rel!r}")
        assert close(res, want_res, N), (k, res, want_res)
        assert close(rel, want_rel, N), (k, rel, want_rel)


# ---------------------------------------------------------------------------------------------
# h. row strips (loopback): a strip's row offset into the y table
# ---------------------------------------------------------------------------------------------
STRIP_CASES = [(2, 129, 65, "P1", "f64"), (3, 129, 65, "P5", "f64"), (2, 257, 129, "P1+H1", "f64"),
               (3, 257, 129, "P1", "f64"), (2, 257, 65, "P5", "f64"), (3, 257, 65, "P1+H1", "f64"),
               (3, 129, 65, "P1+H1", "f32"), (2, 257, 129, "P5", "f32")]


STRIP_CALLS = [("V", 3), ("W", 2), ("F", 2)]


@gpu
@pytest.mark.parametrize("kind,n", STRIP_CALLS)
@pytest.mark.parametrize("case", STRIP_CASES, ids=_id)
def test_strips_against_oracle(pgmg, case, kind, n):
    """Every rank's result is bitwise the single-GPU run's and the oracle's; the monitor's norms
    are the same on every rank and agree with the single-GPU run's within the rule."""
    world, N, gather_n, name, dtype = case
    kw = prm(name, N)
    cfg = dict(gather_n=gather_n, cross_min_n=33, dtype=dtype, **kw)
    for r in range(world):
        assert pgmg.plan_strips(N, world, r, 65, gather_n)[2] >= 1      # level 0 is distributed
    snaps, _ = _reference(kind, N, n, dtype, 1e-7, False, _okw(kw))
    want, sweeps, cut = snaps[-1]
    one = _single(pgmg, N, 0, calls=[(kind, n)], monitor=True, **cfg)
    assert_bitwise(one[0], want, f"single GPU vs oracle {case} {kind}")
    assert one[1] == (sweeps, cut) and one[4], "one GPU: cross-fused, speculative"
    outs = _run_ranks(pgmg, world, N, 0, calls=[(kind, n)], monitor=True, **cfg)
    for r, (phi, stats, res, mon, spec) in enumerate(outs):
        assert_bitwise(phi, want, f"rank {r} of {world} {case} {kind}")
        assert spec, f"rank {r}: the strips' calls are not speculative"
        assert mon == outs[0][3], (r, mon, outs[0][3])
        assert close(res, one[2], N), (r, res, one[2])
        for got, ref in zip(mon, one[3]):
            assert _close2(got, ref, N), (r, mon, one[3])
    # rank 0 counts every level's sweeps once (the gathered levels run on every rank)
    assert outs[0][1] == (sweeps, cut), (outs[0][1], sweeps, cut)
    o, h, f = _oracle(N, name, dtype)
    res_norm, err_norm, exact_norm, rel_error = outs[0][3]
    print(f"strips {case} {kind}: res {res_norm!r} rel {rel_error!r} |u| {exact_norm!r}")
    assert close(res_norm, oracle_res_norm(oracle, want, f, dtype, h), N)
    assert close(exact_norm, oracle.norm(o.exact(N, h)), N)
    assert close(rel_error, o.rel_error(np.ascontiguousarray(want, dtype=o.dt), h), N)


# ---------------------------------------------------------------------------------------------
# i. the op level: pgmg_rhs on any W x H
# ---------------------------------------------------------------------------------------------
RHS_SHAPES = [(3, 3), (5, 6), (9, 130), (130, 9), (129, 128), (257, 513), (64, 1030)]


@gpu
@pytest.mark.parametrize("name", ["P1", "P3", "P5", "P6"])
@pytest.mark.parametrize("shape", RHS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ops_rhs_against_oracle(pgmg, shape, name):
    """Bitwise orc_rhs(W, H, h) with h = a / (max(H, W) - 1) and an arbitrary h; the rows after
    the array stay untouched."""
    import ctypes as C
    import torch
    H, W = shape
    a, p, q = SETS[name]
    o = oracle.Oracle(a=a, p=p, q=q)
    for h in (a / (max(H, W) - 1), 0.0173):
        want = np.zeros((H, W))
        o.L.orc_rhs(C.byref(o.c), want.ctypes.data_as(C.c_void_p), W, H, h)
        buf = torch.full((H + 2, W), 7.0, dtype=torch.float64, device="cuda")
        pgmg.ops.rhs(buf[:H], h, a=a, p=p, q=q)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert_bitwise(got[:H], want, f"rhs {H}x{W} {name} h={h}")
        assert np.all(got[H:] == 7.0), "pgmg_rhs wrote past its array"


# ---------------------------------------------------------------------------------------------
# conditions on the inputs: from the oracle alone (CPU)
# ---------------------------------------------------------------------------------------------
def _all_cycle_cases():
    """(kind, N, set name, eps, dtype, cycles, rand, further oracle fields) of every case above
    whose reference is _reference's"""
    out = [(k, N, name, eps, dt, 3, False, ()) for k, N, name, eps, dt in TAIL_CASES]
    out += [(k, 129, name, eps, dt, 3, False, (("v1", 2), ("v2", 0)) if v == "v1=2,v2=0" else ())
            for v, k, name, eps, dt in _bulk_cases()]
    out += [("V", N, name, eps, dt, sum(calls), False, ())
            for N, name, calls, eps, dt in _cross_cases()]
    out += [("V", N, name, 1e-7, dt, 4, False, ()) for N, name, dt in CARRY_CASES]
    out += [(k, 129, name, 1e-7, dt, 3, False, ()) for name, dt in AGREE_CASES for k in "VW"]
    out += [(k, N, name, 1e-7, dt, sum(calls), False, ())
            for N, name, dt in FLAG_CASES for k, calls in FLAG_CALLS]
    out += [("V", 129, name, eps, "f64", 6, "phi", ())
            for name in RARE_SETS for eps in RARE_EPS[:3]]
    out += [(k, 129, name, 1e-7, dt, 3, "phi", ())
            for name in DEVICE_SETS for k in "VW" for dt in ("f64", "f32")]
    out += [("F", N, name, eps, dt, 3, False, (("n_coarse", 9),) if v == "n_coarse=9" else ())
            for v, N, name, eps, dt in _f_cases()]
    out += [("F", 129, name, 1e-7, "f64", 2, False, ()) for name in F_PLAIN_SETS]
    out += [("V", N, name, 1e-7, dt, 3, False, ()) for N, name, _, dt in _monitor_cases()]
    out += [(k, N, name, 1e-7, dt, SOLVE_CYCLES, False, ()) for N, name, k, dt in SOLVE_CASES]
    out += [(k, N, name, 1e-7, dt, n, False, ())
            for _, N, _, name, dt in STRIP_CASES for k, n in STRIP_CALLS]
    return sorted(set(out), key=repr)


def test_asymmetric_cases_have_asymmetric_results():
    """Every case with p != q has an oracle result that differs from its transpose: a mix-up of
    the x and y tables cannot pass it.  (The monitor's random iterates and the device-bound
    and rare-path cases start from a random phi0, asymmetric by itself; pgmg_rhs's shapes are
    not square.)"""
    checked = 0
    for kind, N, name, eps, dtype, cycles, rand, more in _all_cycle_cases():
        kw = dict(prm(name, N), **dict(more))
        if kw["p"] == kw["q"]:
            continue
        phi = _reference(kind, N, cycles, dtype, eps, rand, _okw(kw))[0][-1][0]
        if (kw["p"] == 0 or kw["q"] == 0) and not rand:
            assert not phi.any(), (kind, N, name)      # f = 0: nothing to tell apart
            continue
        assert not np.array_equal(phi, phi.T), (kind, N, name, eps, dtype)
        checked += 1
    for N, name, dtype in HANDS_CASES:
        for k, (phi, _, _) in enumerate(_vfvw_reference(N, name, dtype)):
            assert not np.array_equal(phi, phi.T), (N, name, dtype, k)
    for nu in (1, 2):
        for N, name, dtype in FMG_CASES:
            for u, _, _ in _fmg_reference(N, name, nu, dtype):
                assert not np.array_equal(u, u.T), (N, name, nu)
    for N, name, dtype in MON_BOUND_CASES:
        phi0, _ = _problem(N, dtype, "phi")
        assert not np.array_equal(phi0, phi0.T)
    assert checked >= 250, checked


def test_p5_is_order_one_on_the_far_boundary():
    """P5: |f| and |u| exceed 0.1 somewhere on row N - 1 and on column N - 1, at the default
    mesh width and at H1 and H2, for every size the tests run."""
    for N in (33, 65, 129, 257, 513):
        for name in ("P5", "P5+H1", "P5+H2"):
            for dtype in ("f64", "f32"):
                o, h, f = _oracle(N, name, dtype)
                u = o.exact(N, h)
                for g in (f, u):
                    assert np.abs(g[N - 1]).max() > 0.1 and np.abs(g[:, N - 1]).max() > 0.1, \
                        (N, name, dtype)
    o, h, f = _oracle(129, "P1")     # an integer p: ~1e-13 there, what the defaults leave untested
    assert np.abs(f[128]).max() < 1e-9


def test_exit_mix_of_every_family():
    """For each of the families a, p/q and h0 a GPU-run case whose smoother calls never exit
    early, one where some do and one where all do: the oracle's counters (CPU only)."""
    mix = {(name): (k, N, name, eps, dt, want) for k, N, name, eps, dt, want in MIX_CASES}
    for k, N, name, eps, dt, want in MIX_CASES:
        kw = prm(name, N)
        _, (exits, calls) = _reference(k, N, 3, dt, eps, False, _okw(kw))
        print(f"{name} {k} N={N} eps={eps}: {exits} exits in {calls} calls")
        assert _mix(k, N, 3, dt, eps, False, **kw) == want, (name, want, exits, calls)
    for family, (none, mixed, all_) in MIX_FAMILIES.items():
        assert (mix[none][5], mix[mixed][5], mix[all_][5]) == ("none", "mixed", "all"), family


def test_precision_split():
    """P8 at N = 65 (p = 63): one undamped Jacobi sweep annihilates the mode, the residual norm
    is rounding error: below eps = 1e-7 in fp64 (every call exits), above it in fp32 (none)."""
    got = []
    for k, N, name, eps, dt in SPLIT:
        kw = prm(name, N)
        got.append(_mix(k, N, 3, dt, eps, False, **kw))
    assert got == ["all", "none"], got


def test_exit_mix_cases_are_run_on_the_gpu():
    for c in [x[:5] for x in MIX_CASES] + list(SPLIT):
        assert c in TAIL_CASES, c
    # every path's table holds P1, P3, P5 and an h0 variant, in fp64 and fp32
    tables = {"tail": [(n, d) for _, _, n, _, d in TAIL_CASES],
              "bulk": [(n, d) for _, _, n, _, d in _bulk_cases()],
              "cross": [(n, d) for _, n, _, _, d in _cross_cases()],
              "F": [(n, d) for _, _, n, _, d in _f_cases()],
              "monitor": [(n, d) for _, n, _, d in _monitor_cases()],
              "strips": [(n, d) for _, _, _, n, d in STRIP_CASES]}
    for path, rows in tables.items():
        names = {n for n, _ in rows}
        assert {"P1", "P5"} <= names and any("+H" in n for n in names), (path, names)
        assert path == "strips" or "P3" in names, path
        assert {d for _, d in rows} == {"f64", "f32"}, path
        for must in ("P1", "P5"):
            assert {d for n, d in rows if n.startswith(must)} == {"f64", "f32"}, (path, must)
