"""The late entries off the defaults: pgmg_damp, pgmg_solve_damped, pgmg_fmg_damped, pgmg_fmg_bc
and pgmg_solve_extrap with a, p, q, h0 and alpha, n_coarse, coarse_iter, v1, v2, tail_n away from
(1, 1, 1, 0) and (3, 5, 10, 1, 1, 65), against their models over the CPU oracle.

tests/test_gpu_cycle_params.py and tests/test_gpu_problem_params.py did this for every path that
existed when they were written; the entries above came later and their own tests run at the
defaults, where every run is symmetric under transposition and the sine tables vanish on the far
boundary.  What a default run cannot see:

* k_monitor<..., kMonDamp | kMonRes | kMonGen>, the damping pass that regenerates the analytic f
  from gfx[i] * gsy[j] -- from pgmg_damp (the context's tables) and on level 0 of the damped
  climb (the cycle's tables);
* the damping weight w = (T)(omega * 0.25 * (h * h)) and ih on every level of the pyramid with
  h0 != 0, a != 1 and a < 0;
* pgmg_fmg_bc's frame buffer and pgmg_fmg_damped's per-level damp with n_coarse 9 / 17,
  coarse_iter 0 / 30, v1 != v2 (the unfused general path) and another tail_n;
* pgmg_solve_damped with W-cycles at alpha != 3, F-cycles, and PGMG_MON_ERROR at the context's h0;
* pgmg_solve_extrap's half-resolution context: its h0' = 2 h0, a child with bulk levels of its
  own (N = 129 with tail_n = 17: 65 and 33), a child with another n_coarse.

The parameter sets are test_gpu_problem_params.py's (P1 .. P10, NEG, H1, H2).  Tolerance: EXACT
for phi, the frame and pgmg_stats == (o.sweeps, o.cut_exits); norms by the project's rule,
solve_rule.close (two summation orders of the same terms); rel_error as that module's
_monitor_check compares it.  Sizes: N = 33 / 65 (tail only), 129 (one bulk level; three with
tail_n = 17), 257, and 513 for the damping pass alone (its first full tile).  The op-level
pgmg_damp_grid and pgmg_extrap_grid run on the same sets' mesh widths and solutions.  The conditions on
the inputs (every solve converges, the decisions are comparable, the exits are mixed) are checked
from the models alone in tests/test_late_params_cpu.py.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import damp_model
import extrap_model
import fmg_bc_model
import fmg_damped_model
from conftest import assert_bitwise
from solve_rule import close, norm_tol
from test_gpu_cycle_params import _problem
from test_gpu_extrap import _compare
from test_gpu_problem_params import SETS, _f64, _h, _oracle, prm

gpu = pytest.mark.gpu

CYCLE_KEYS = ("alpha", "n_coarse", "coarse_iter", "v1", "v2")
OMEGAS = (0.5, 1.0, 0.3)
EPS3 = (1e-7, 1e-4, -1.0)
NAMES = [n for n in SETS if n != "P0"]
NU = 2


def _id(c):
    return "-".join(str(dict(x)) if isinstance(x, tuple) and x and isinstance(x[0], tuple) else str(x)
                    for x in c if x != ())


def _cfg(**kw):
    """a hashable pgmg_config fragment"""
    return tuple(sorted(kw.items()))


def _split(name, N, cfg):
    """(pgmg_config fields, the oracle's cycle fields) of a set name and a fragment"""
    kw = dict(prm(name, N), **dict(cfg))
    return kw, {k: v for k, v in kw.items() if k in CYCLE_KEYS}


def _frame_check(got, phi0, what):
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert_bitwise(got[edge], phi0[edge], f"{what}: the frame")


def _exact_frame(o, N, h):
    """the exact solution on the frame, zero inside, in values of the oracle's element type"""
    g = fmg_bc_model.set_frame(np.zeros((N, N)), o.exact(N, h))
    return _f64(g.astype(o.dt))


# ---------------------------------------------------------------------------------------------
# a. pgmg_damp: one pass on a random phi0 with a non-zero boundary
# ---------------------------------------------------------------------------------------------
F_MODES = ("regenerated", "stored", "own")


def _damp_cases():
    """(N, set, f, dtype, omega): every set and three h0 variants at three sizes with the analytic
    f regenerated (kMonGen), the context's stored copy of it and a caller's f, in fp64; every
    set once in fp32 at N = 129; omega by position."""
    cases, i = [], 0
    for name in NAMES + ["P1+H1", "P5+H1", "P5+H2"]:
        for N in (33, 129, 513):
            for fmode in F_MODES:
                cases.append((N, name, fmode, "f64", OMEGAS[i % 3]))
                i += 1
            i += 1
    for name in NAMES + ["P1+H1", "P5+H1", "P5+H2"]:
        cases.append((129, name, F_MODES[i % 3], "f32", OMEGAS[(i // 3) % 3]))
        i += 1
    return cases


def _damp_problem(N, name, fmode, dtype):
    """(h, phi0, the f to hand to set_problem or None, the f the model reads)"""
    o, h, fa = _oracle(N, name, dtype)
    phi0, fr = _problem(N, dtype, True if fmode == "own" else "phi")
    return h, phi0, fr, fa if fr is None else np.ascontiguousarray(fr, dtype=o.dt)


def _damp_check(s, read, phi0, f, h, omega, dtype, what):
    """One pgmg_damp from phi0 (already set on s) against damp_model.damp."""
    N = phi0.shape[0]
    before = s.monitor().res_norm
    got_norm = s.damp(omega)
    s.sync()
    got = read()
    want, want_norm = damp_model.damp(phi0, f, h, omega, dtype)
    print(f"{what}: norm {got_norm!r} (model {want_norm!r})")
    assert_bitwise(got, want, what)
    _frame_check(got, phi0, what)
    assert np.float64(got_norm).view(np.uint64) == np.float64(before).view(np.uint64), \
        (what, got_norm, before)
    assert close(got_norm, want_norm, N), (what, got_norm, want_norm)


@gpu
@pytest.mark.parametrize("case", _damp_cases(), ids=_id)
def test_damp_against_model(pgmg, case):
    N, name, fmode, dtype, omega = case
    h, phi0, fset, f = _damp_problem(N, name, fmode, dtype)
    es = 4 if dtype == "f32" else 8
    flags = pgmg.PGMG_FLAG_STORED_RHS if fmode == "stored" else 0
    with pgmg.Solver(N, dtype=dtype, flags=flags, **prm(name, N)) as s:
        s.set_problem(phi0, fset)
        # the pass regenerates f exactly when it does not stream one (pgmg_monitor_time's bytes)
        streamed = s.monitor_time(reps=1)[1] - es * N * N
        assert streamed == (0 if fmode == "regenerated" else es * (N - 2) ** 2), (case, streamed)
        _damp_check(s, s.solution, phi0, f, h, omega, dtype, f"damp {case}")


@gpu
@pytest.mark.parametrize("fmode", ["regenerated", "own"])
@pytest.mark.parametrize("inplace", [False, True], ids=["staged", "inplace"])
@pytest.mark.parametrize("name,omega", [("P1", 0.3), ("P5+H1", 0.5)])
def test_damp_device_bound(pgmg, plan, name, omega, inplace, fmode):
    """The caller's arrays of pgmg_set_problem_device: phi read and written where it lies."""
    import torch
    plan(cross_min_n=9)
    N = 129
    h, phi0, fset, f = _damp_problem(N, name, fmode, "f64")
    with pgmg.Solver(N, **prm(name, N)) as s:
        if inplace:
            g = pgmg.DeviceGrid(N, np.array(phi0))
            fd = pgmg.DeviceGrid(N, np.array(fset)) if fset is not None else None
            read = g.download
        else:
            g = torch.tensor(np.array(phi0), dtype=torch.float64, device="cuda")
            fd = (torch.tensor(np.array(fset), dtype=torch.float64, device="cuda")
                  if fset is not None else None)
            torch.cuda.synchronize()
            read = lambda: g.cpu().numpy()   # noqa: E731
        s.set_problem_device(g, fd)
        assert s.device_info() == (True, inplace)
        _damp_check(s, read, phi0, f, h, omega, "f64", f"device-bound damp {name} {fmode} {inplace}")
        if inplace:
            g.close()
            if fd is not None:
                fd.close()


# ---------------------------------------------------------------------------------------------
# b. pgmg_fmg_damped and pgmg_fmg_bc
# ---------------------------------------------------------------------------------------------
# (entry, omega): the three calls every case makes, one after another on one context
ENTRIES = (("damped", 0.5), ("bc", 0.0), ("bc", 0.5))
FMG_SETS = ["P1", "P3", "P4", "P5", "P6", "P9", "P10", "NEG", "P1+H1", "P5+H1", "P1+H2"]
FMG_LEVELS = {65: (0, 65), 129: (1, 65), 257: (2, 65)}


@functools.lru_cache(maxsize=None)
def _fmg_problem(N, name, dtype, fkind):
    """(phi0, f for set_problem or None, the model's f): "analytic": the exact solution as the
    frame (non-zero for P5 and every H set); "own": _problem's random phi0 and right-hand side."""
    o, h, fa = _oracle(N, name, dtype)
    if fkind == "own":
        phi0, fr = _problem(N, dtype, True)
        return phi0, fr, np.ascontiguousarray(fr, dtype=o.dt)
    return _exact_frame(o, N, h), None, fa


@functools.lru_cache(maxsize=None)
def _fmg_ref(entry, N, name, dtype, eps, fkind, okw):
    """The model's run, computed once and shared: (phi, sweeps, cut exits) after the entry and
    after two more V-cycles."""
    kind, omega = entry
    o, h, _ = _oracle(N, name, dtype, eps, **dict(okw))
    phi0, _, f = _fmg_problem(N, name, dtype, fkind)
    if kind == "damped":
        u = fmg_damped_model.fmg_damped(o, f, NU, omega, h0=h)
    else:
        u = fmg_bc_model.fmg_bc(o, phi0, f, NU, omega, h0=h)
    first = (_f64(u), o.sweeps, o.cut_exits)
    for _ in range(2):
        o.v_cycle(u, f, h)
    return first, (_f64(u), o.sweeps, o.cut_exits)


def _fmg_check(pgmg, N, name, dtype, eps, fkind, cfg, levels, flags=0, after=None):
    kw, okw = _split(name, N, cfg)
    phi0, fset, _ = _fmg_problem(N, name, dtype, fkind)
    with pgmg.Solver(N, dtype=dtype, eps=eps, flags=flags, **kw) as s:
        assert s.levels() == levels, (s.levels(), levels)
        if after is not None:
            after(s)
        for entry in ENTRIES:
            (u0, sw0, cut0), (u2, sw2, cut2) = _fmg_ref(entry, N, name, dtype, eps, fkind, _cfg(**okw))
            what = f"{entry} N={N} {name} {dtype} eps={eps} f={fkind} {dict(cfg)} flags={flags}"
            s.set_problem(phi0, fset)
            if entry[0] == "damped":
                s.fmg(NU, damp=entry[1])
            else:
                s.fmg(NU, damp=entry[1] or None, boundary="keep")
            got = s.solution()
            assert_bitwise(got, u0, what)
            if entry[0] == "bc":
                _frame_check(got, phi0, what)
            assert s.stats() == (sw0, cut0), (what, s.stats(), sw0, cut0)
            s.vcycle(2)
            assert_bitwise(s.solution(), u2, what + " + 2 V")
            assert s.stats() == (sw2, cut2), (what, s.stats(), sw2, cut2)


def _fmg_cases():
    """(N, set, dtype, eps, f): every set at three sizes in fp64 on the analytic problem, eps by
    position; every set once in fp32; a caller's f where only a and h0 matter."""
    cases, i = [], 0
    for name in FMG_SETS:
        for N in (65, 129, 257):
            cases.append((N, name, "f64", EPS3[i % 3], "analytic"))
            i += 1
        cases.append(((65, 129, 257)[i % 3], name, "f32", EPS3[(i + 1) % 3], "analytic"))
        i += 1
    for k, name in enumerate(("P3", "P9", "NEG", "P1+H1", "P5+H1")):
        cases.append((129, name, "f64", EPS3[k % 3], "own"))
    cases += [(65, "P1+H2", "f64", 1e-7, "own"), (257, "P5+H1", "f32", 1e-4, "own")]
    return cases


@gpu
@pytest.mark.parametrize("case", _fmg_cases(), ids=_id)
def test_fmg_entries_against_models(pgmg, case):
    """pgmg_fmg_damped(0.5), pgmg_fmg_bc(0) and pgmg_fmg_bc(0.5) on the default plan: bitwise
    fmg_damped_model / fmg_bc_model at the context's h0, then two V-cycles from the result."""
    N, name, dtype, eps, fkind = case
    _fmg_check(pgmg, N, name, dtype, eps, fkind, (), FMG_LEVELS[N])


# (variant, N, pgmg_config fragment, levels)
FMG_VARIANTS = [
    ("n_coarse=9", 129, _cfg(n_coarse=9), (1, 65)),
    ("n_coarse=17", 129, _cfg(n_coarse=17), (1, 65)),
    ("coarse_iter=0", 129, _cfg(coarse_iter=0), (1, 65)),
    ("coarse_iter=30", 129, _cfg(coarse_iter=30), (1, 65)),
    ("n_coarse=17,coarse_iter=30", 129, _cfg(n_coarse=17, coarse_iter=30), (1, 65)),
    ("v1=2,v2=3", 129, _cfg(v1=2, v2=3), (1, 65)),
    ("tail_n=9", 129, _cfg(tail_n=9), (4, 9)),
    ("tail_n=17", 129, _cfg(tail_n=17), (3, 17)),
    ("tail_n=17,n_coarse=9,v1=2,v2=3", 129, _cfg(tail_n=17, n_coarse=9, v1=2, v2=3), (3, 17)),
    ("cross", 129, _cfg(cross_min_n=33), (1, 65)),
    ("cross,tail_n=17", 129, _cfg(cross_min_n=33, tail_n=17), (3, 17)),
    ("n_coarse=1000", 65, _cfg(n_coarse=1000), (0, 65)),
]


def _fmg_variant_cases():
    cases, i = [], 0
    for variant, N, cfg, levels in FMG_VARIANTS:
        for name in ("P1", "P5+H1"):
            for stored in (False, True):
                fkind = "own" if (variant, name, stored) in FMG_VARIANT_OWN else "analytic"
                cases.append((variant, N, name, "stored" if stored else "regenerated",
                              EPS3[i % 3], fkind, cfg, levels))
                i += 1
    return cases


# with a caller's f PGMG_FLAG_STORED_RHS changes nothing, so only unflagged cases take one
FMG_VARIANT_OWN = {("n_coarse=17,coarse_iter=30", "P5+H1", False), ("tail_n=9", "P5+H1", False)}


@gpu
@pytest.mark.parametrize("case", _fmg_variant_cases(), ids=lambda c: _id(c[:6]))
def test_fmg_entries_cycle_parameters(pgmg, case):
    """The three entries crossed with the cycle parameters and the plan, with the analytic f
    regenerated on level 0 and with PGMG_FLAG_STORED_RHS: the coarsest start of 9 and 17 points,
    coarsest solves of 1 and 31 sweeps, the unfused general path (v1 != v2), other tails, a
    cross-fused level 0 (its grids rotate between the damps), and no climb at all."""
    variant, N, name, rhs, eps, fkind, cfg, levels = case
    flags = pgmg.PGMG_FLAG_STORED_RHS if rhs == "stored" else 0

    def after(s):
        if N > 65:
            assert s.fused == ("v1=2" not in variant), "not the kernel sequence this case is for"
        assert (s.stats_detail()[2] >= 0) == variant.startswith("cross"), "cross-cycle fusion"

    _fmg_check(pgmg, N, name, "f64", eps, fkind, cfg, levels, flags, after)


# ---------------------------------------------------------------------------------------------
# c. pgmg_solve_damped
# ---------------------------------------------------------------------------------------------
# a case of pgmg_solve_damped: the cycle kind, the pgmg_config fragment, the stop rule, and
#   error: PGMG_MON_ERROR; bound: "inplace" for pgmg_set_problem_device; start: "fmg" for the
#   fmg_bc start from the exact frame; capped: the one case that ends at the cycle cap
SolveCase = namedtuple("SolveCase", "N name kind dtype eps cfg rule error bound start capped",
                       defaults=(False, None, None, False))
RTOL = _cfg(rtol=1e-4, max_cycles=40)
SOLVE_OMEGA = 0.5
SOLVE_LEVELS = {65: (0, 65), 129: (1, 65), 257: (2, 65)}

SOLVE_CASES = [SolveCase(N, name, "V", "f64", 1e-7, (), RTOL)
               for N in (129, 257) for name in ("P1", "P3", "P5+H1", "P9", "NEG")] + [
    SolveCase(129, "P10", "V", "f64", 1e-7, (), RTOL),
    SolveCase(129, "P1", "W", "f64", 1e-7, _cfg(alpha=1), RTOL),
    SolveCase(129, "P5+H1", "W", "f64", 1e-7, _cfg(alpha=2), RTOL),
    SolveCase(129, "P3", "W", "f64", -1.0, _cfg(alpha=4), RTOL),
    SolveCase(129, "P1+H2", "V", "f64", 1e-7, (), _cfg(rtol=1e-4, max_cycles=40, check_every=2)),
    SolveCase(129, "P1+H1", "V", "f64", 1e-7, (), RTOL, error=True),
    SolveCase(257, "P5+H2", "V", "f64", -1.0, (), RTOL, error=True),
    SolveCase(129, "P5+H1", "V", "f32", 1e-7, (), _cfg(rtol=1e-3, max_cycles=40)),
    SolveCase(129, "P5+H1", "V", "f64", 1e-7, _cfg(cross_min_n=33), RTOL, bound="inplace"),
    SolveCase(129, "P5+H1", "V", "f64", 1e-7, _cfg(n_coarse=9, tail_n=17), RTOL, error=True,
              start="fmg"),
    SolveCase(129, "P1", "F", "f64", 1e-7, (), _cfg(rtol=0.0, atol=0.0, max_cycles=3), capped=True),
]


@functools.lru_cache(maxsize=None)
def _solve_start(c):
    """(phi0 or None, the model's namespace with sweeps and exits of the whole call sequence)"""
    kw, okw = _split(c.name, c.N, c.cfg)
    h = _h(c.N, kw)
    a, p, q = kw["a"], kw["p"], kw["q"]
    o, _, f = _oracle(c.N, c.name, c.dtype, c.eps, **okw)
    phi0, u, sweeps, exits = None, None, 0, 0
    if c.start == "fmg":
        phi0 = _exact_frame(o, c.N, h)
        u = fmg_bc_model.fmg_bc(o, phi0, f, NU, SOLVE_OMEGA, h0=h)
        sweeps, exits = o.sweeps, o.cut_exits
    elif c.bound:
        phi0 = u = _problem(c.N, c.dtype, "phi")[0]
    m = damp_model.solve_damped(c.N, phi0=u, kind=c.kind, omega=SOLVE_OMEGA, dtype=c.dtype,
                                eps=c.eps, error=c.error, h0=h, a=a, p=p, q=q, **okw, **dict(c.rule))
    m.sweeps += sweeps
    m.exits += exits
    m.phi = _f64(m.phi)
    return phi0, m


def _solve_compare(info, got, stats, m, N, what):
    """cycles, checks, reason, every pgmg_history entry, res0 / res, phi and the statistics"""
    print(f"{what}: model {m.cycles} cycles, reason {m.reason}, margin {m.margin:.3e}, "
          f"{m.sweeps} sweeps, {m.exits} exits")
    assert m.margin > 100 * norm_tol(N), (what, m.margin)
    assert (info.cycles, info.reason, info.checks) == (m.cycles, m.reason, m.checks), what
    assert len(info.history) == len(m.history)
    for (k, r, e), (mk, mr, me) in zip(info.history, m.history):
        print(f"  check at {k}: res {r!r} / {mr!r}  rel {e!r} / {me!r}")
        assert k == mk and close(r, mr, N), (what, k, r, mr)
        assert close(e, me, N), (what, k, e, me)
    assert close(info.res0, m.history[0][1], N), (what, info.res0)
    assert info.res == info.history[-1][1]
    assert_bitwise(got, m.phi, what)
    assert stats == (m.sweeps, m.exits), (what, stats, m.sweeps, m.exits)


def _levels(N, cfg):
    """pgmg_levels of a case: the table above, or (129 with tail_n = 17) three bulk levels"""
    return {(129, 17): (3, 17)}.get((N, dict(cfg).get("tail_n")), SOLVE_LEVELS[N])


@gpu
@pytest.mark.parametrize("c", SOLVE_CASES, ids=_id)
def test_solve_damped_against_model(pgmg, c):
    kw, _ = _split(c.name, c.N, c.cfg)
    phi0, m = _solve_start(c)
    opts = dict(cycle=c.kind, damp=SOLVE_OMEGA, error=c.error, **dict(c.rule))
    with pgmg.Solver(c.N, dtype=c.dtype, eps=c.eps, **kw) as s:
        assert s.levels() == _levels(c.N, c.cfg)
        if c.bound:
            with pgmg.DeviceGrid(c.N, np.array(phi0)) as g:
                s.set_problem_device(g, None)
                assert s.device_info() == (True, True)
                info = s.solve(**opts)
                got, stats = g.download(), s.stats()
        else:
            s.set_problem(phi0, None)
            info = s.solve(start=c.start, boundary="keep", **opts)
            got, stats = s.solution(), s.stats()
    _solve_compare(info, got, stats, m, c.N, f"solve_damped {_id(c)}")
    if c.start:
        _frame_check(got, phi0, "solve from the fmg_bc start")


# ---------------------------------------------------------------------------------------------
# d. pgmg_solve_extrap
# ---------------------------------------------------------------------------------------------
# the rule of tests/test_gpu_extrap.py: rtol = 0, atol = 1e-10 ||f||_2 over the interior
EX_RULE = dict(max_cycles=40, rtol=0.0)
# f: "analytic" (the exact solution as the frame; f regenerated on the parent, injected for the
# child) or "own"; bound: None, "staged" or "inplace"; levels / child: pgmg_levels of the context
# and of a context with the child's configuration
ExCase = namedtuple("ExCase", "N name f eps cfg levels child bound", defaults=(None,))
EX_SETS = ["P1", "P3", "P5+H1", "P9", "NEG", "P1+H2"]
EX_PLAIN = {65: ((0, 65), (0, 33)), 129: ((1, 65), (0, 65))}
T17 = ((3, 17), (2, 17))      # N = 129, tail_n = 17: the child has the bulk levels 65 and 33

EX_CASES = [ExCase(N, name, "analytic", eps, (), *EX_PLAIN[N])
            for name in EX_SETS for N in (65, 129) for eps in (-1.0, 1e-7)] + [
    ExCase(129, "P1", "analytic", 1e-7, _cfg(tail_n=17), *T17),
    ExCase(129, "P5+H1", "analytic", -1.0, _cfg(tail_n=17), *T17),
    ExCase(129, "NEG", "analytic", 1e-7, _cfg(tail_n=17), *T17),
    ExCase(129, "P1", "analytic", 1e-7, _cfg(n_coarse=9), *EX_PLAIN[129]),
    ExCase(129, "P5+H1", "analytic", 1e-7, _cfg(n_coarse=9, tail_n=17), *T17),
    ExCase(129, "P1", "analytic", -1.0, _cfg(coarse_iter=0), *EX_PLAIN[129]),
    ExCase(129, "P5+H1", "analytic", 1e-7, _cfg(coarse_iter=0), *EX_PLAIN[129]),
    ExCase(129, "P1", "analytic", 1e-7, _cfg(v1=2, v2=3), *EX_PLAIN[129]),
    ExCase(129, "P5+H1", "analytic", -1.0, _cfg(v1=2, v2=3, tail_n=17), *T17),
    ExCase(65, "P3", "own", 1e-7, (), *EX_PLAIN[65]),
    ExCase(129, "P3", "own", -1.0, (), *EX_PLAIN[129]),
    ExCase(129, "NEG", "own", 1e-7, (), *EX_PLAIN[129]),
    ExCase(129, "P1+H2", "own", 1e-7, _cfg(tail_n=17), *T17),
    ExCase(129, "P5+H1", "own", -1.0, _cfg(n_coarse=9, tail_n=17), *T17),
    ExCase(129, "P5+H1", "analytic", 1e-7, _cfg(tail_n=17), *T17, bound="staged"),
    ExCase(129, "P1+H2", "own", 1e-7, _cfg(tail_n=17), *T17, bound="staged"),
    ExCase(129, "P5+H1", "analytic", 1e-7, _cfg(cross_min_n=33, tail_n=17), *T17, bound="inplace"),
    ExCase(129, "P3", "own", 1e-7, _cfg(cross_min_n=33, tail_n=17), *T17, bound="inplace"),
]


@functools.lru_cache(maxsize=None)
def _ex_problem(N, name, fkind):
    """(f, phi0, atol)"""
    o, h, fa = _oracle(N, name)
    if fkind == "own":
        phi0, f = _problem(N, "f64", True)
    else:
        phi0, f = _exact_frame(o, N, h), _f64(fa)
    return f, phi0, 1e-10 * float(np.linalg.norm(f[1:-1, 1:-1]))


@functools.lru_cache(maxsize=None)
def _ex_model(c):
    kw, okw = _split(c.name, c.N, c.cfg)
    f, phi0, atol = _ex_problem(c.N, c.name, c.f)
    m = extrap_model.solve_extrap(c.N, f, phi0, NU, SOLVE_OMEGA, eps=c.eps, h0=_h(c.N, kw),
                                  a=kw["a"], p=kw["p"], q=kw["q"], **okw, atol=atol, **EX_RULE)
    m.phi = _f64(m.phi)
    return m


@gpu
@pytest.mark.parametrize("c", EX_CASES, ids=_id)
def test_solve_extrap_against_model(pgmg, c):
    import torch
    N, Nc = c.N, (c.N + 1) // 2
    kw, _ = _split(c.name, N, c.cfg)
    f, phi0, atol = _ex_problem(N, c.name, c.f)
    m = _ex_model(c)
    own = c.f == "own"
    # the half-resolution context is the library's own; a context of its configuration -- N' =
    # (N + 1) / 2, h0' = 2 h, the rest equal -- pins its level layout.  (a < 0: h < 0, which
    # h0 cannot state; a / (N' - 1) is 2 h bit for bit)
    h2 = 2 * _h(N, kw)
    assert kw["a"] / (Nc - 1) == h2 or "h0" in kw
    with pgmg.Solver(Nc, eps=c.eps, **dict(kw, h0=h2 if h2 > 0 else 0.0)) as child:
        assert child.levels() == c.child, (child.levels(), c.child)
        assert (child.stats_detail()[2] >= 0) == ("cross_min_n" in kw)
    with pgmg.Solver(N, eps=c.eps, **kw) as s:
        assert s.levels() == c.levels, (s.levels(), c.levels)
        grids = []
        if c.bound == "inplace":
            grids = [pgmg.DeviceGrid(N, np.array(phi0))] + ([pgmg.DeviceGrid(N, np.array(f))] if own else [])
            read = grids[0].download
        elif c.bound == "staged":
            grids = [torch.tensor(np.array(a), dtype=torch.float64, device="cuda")
                     for a in ([phi0, f] if own else [phi0])]
            torch.cuda.synchronize()
            read = lambda: grids[0].cpu().numpy()   # noqa: E731
        if c.bound:
            s.set_problem_device(grids[0], grids[1] if own else None)
            assert s.device_info() == (True, c.bound == "inplace")
        else:
            s.set_problem(phi0, f if own else None)
            read = s.solution
        info = s.solve(order=4, damp=SOLVE_OMEGA, nu=NU, atol=atol, **EX_RULE)
        got, stats = read(), s.stats()
        if c.bound == "inplace":
            for g in grids:
                g.close()
    what = f"solve_extrap {_id(c)}"
    _compare(info, got, stats[0], m, N, what)
    assert stats[1] == m.fine.exits, (what, stats, m.fine.exits)
    assert info.coarse_exits == m.coarse.exits, (what, info.coarse_exits, m.coarse.exits)
    _frame_check(got, phi0, what)


# ---------------------------------------------------------------------------------------------
# e. the op level: pgmg_damp_grid and pgmg_extrap_grid on what the sets produce
# ---------------------------------------------------------------------------------------------
# pgmg_damp_grid takes its h as an argument and needs h > 0 (NEG's |h|: h enters as h * h)
OP_DAMP_CASES = [(33, "P3", 0.5), (129, "P9", 0.3), (513, "P10", 1.0), (129, "P1+H1", 0.3),
                 (513, "P5+H2", 0.5), (33, "P4", 1.0), (129, "NEG", 0.3)]


@gpu
@pytest.mark.parametrize("N,name,omega", OP_DAMP_CASES)
def test_ops_damp_grid_at_the_sets_mesh_widths(pgmg, N, name, omega):
    import torch
    o, h, f = _oracle(N, name)
    h = abs(h)
    phi0, _ = _problem(N, "f64", "phi")
    want, want_norm = damp_model.damp(phi0, f, h, omega)
    x = torch.tensor(np.array(phi0), dtype=torch.float64, device="cuda")
    ft = torch.tensor(np.array(f), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got_norm = pgmg.ops.damp(x, ft, h, omega)
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    assert_bitwise(got, want, f"pgmg_damp_grid N={N} {name} omega={omega}")
    _frame_check(got, phi0, f"pgmg_damp_grid N={N} {name}")
    assert close(got_norm, want_norm, N), (got_norm, want_norm)
    pgmg.ops.release()


@gpu
@pytest.mark.parametrize("c", [c for c in EX_CASES if c.eps == 1e-7 and not c.bound and
                               c.name in ("P5+H1", "NEG", "P9")][:6], ids=_id)
def test_ops_extrap_grid_on_the_models_solutions(pgmg, c):
    """The two second-order solutions of an off-default case, extrapolated by the op."""
    import torch
    m = _ex_model(c)
    fine = torch.tensor(np.array(m.phi2), dtype=torch.float64, device="cuda")
    coarse = torch.tensor(np.array(m.coarse.phi), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pgmg.ops.extrapolate(fine, coarse)
    torch.cuda.synchronize()
    assert_bitwise(fine.cpu().numpy(), m.phi, f"pgmg_extrap_grid {_id(c)}")
    pgmg.ops.release()
