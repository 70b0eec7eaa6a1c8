"""GPU: sampled checks.  On a speculative call (one GPU) the finest level's cross-cycle pass
sums its two early-exit checks over a sample of its rows (1 in 6, or 1 in 4): a lower bound of
the full sum, which the validation needs only to show that a check cannot fire.  Words and
statistics must stay exactly those of the in-stream path (PGMG_FLAG_EXACT_DIST), of the full-sum
speculative path (PGMG_FLAG_FULL_CHECKS) and of the oracle: without a firing check, in the
band where a sampled check could fire and the full one does not, on IEEE special values and on
bands that hold no sampled row.

Solver.sampled_info() = (finest passes launched in the sampled form, rollbacks caused only by
sampled checks after which no cross-cycle check fired, 1 while the context sums every row again).
"""
import functools

import numpy as np
import pytest

import special_values as sv
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

SERIES = (1, 1, 3)   # the carry pass; carry + recompute in one pass; recompute, plain, carry
FAST_TOL = 1e-12     # test_gpu_fast.py: relative L2 and max-abs against the exact default, N <= 4097


@functools.lru_cache(maxsize=None)
def _oracle(N, dtype, eps=1e-7):
    """(phi as float64, sweeps, cut exits) of the oracle after sum(SERIES) V-cycles from phi = 0 on
    the analytic f; computed once per size and type, read-only."""
    import oracle
    o = oracle.Oracle(eps=eps, dtype=dtype)
    f = o.rhs(N)
    phi = np.zeros((N, N), dtype=o.dt)
    for _ in range(sum(SERIES)):
        o.v_cycle(phi, f)
    out = phi.astype(np.float64)
    out.setflags(write=False)
    return out, o.sweeps, o.cut_exits


def _series(pgmg, N, flags, dtype="f64", problem=(None, None), calls=SERIES, timed=False, **cfg):
    """solution, stats_detail, dist_info, sampled_info and (timed) the plain k_postpre's symbol"""
    if timed:
        flags |= pgmg.PGMG_FLAG_TIME_FINE
    with pgmg.Solver(N, dtype=dtype, flags=flags, **cfg) as s:
        s.set_problem(*problem)
        assert s.stats_detail()[2] >= 0, "cross-cycle fusion not active"
        for k in calls:
            s.vcycle(k)
        sym = ""
        if timed:
            n, _ = s.fine_pass_time(3)
            assert n > 0, "no plain k_postpre was timed"
            sym = s.fine_pass_info(3)[0]
        return s.solution(), s.stats_detail(), s.dist_info(), s.sampled_info(), sym


CASES = [(N, rhs, dtype, fast)
         for N in (129, 257, 2049) for rhs in ("analytic", "caller")
         for dtype, fast in (("f64", False), ("f32", False), ("f64", True))]


@pytest.mark.parametrize("N,rhs,dtype,fast", CASES)
def test_sampled_equals_in_stream_full_and_oracle(pgmg, plan, N, rhs, dtype, fast):
    plan(cross_min_n=9)
    ref, sweeps, exits = _oracle(N, dtype)
    problem = (None, None)
    if rhs == "caller":   # the same f handed over as an array: streamed from HBM
        problem = (np.zeros((N, N)), sv.analytic_f(N, dtype).astype(np.float64))
    ff = pgmg.PGMG_FLAG_FAST if fast else 0
    kw = dict(dtype=dtype, problem=problem, tail_n=33)
    smp = _series(pgmg, N, ff, timed=True, **kw)
    full = _series(pgmg, N, ff | pgmg.PGMG_FLAG_FULL_CHECKS, timed=True, **kw)
    exact = _series(pgmg, N, ff | pgmg.PGMG_FLAG_EXACT_DIST, **kw)
    print(f"N={N} {rhs} {dtype} fast={fast}: sampled_info {smp[3]} / {full[3]} / {exact[3]}, "
          f"rollbacks {smp[2][1]} / {full[2][1]}, symbols {smp[4]!r} / {full[4]!r}")
    assert smp[3][0] > 0, smp[3]
    assert full[3] == (0, 0, 0) and exact[3] == (0, 0, 0), (full[3], exact[3])
    assert smp[4] and full[4] and smp[4] != full[4], (smp[4], full[4])
    # the sampled form stores what the full-sum form stores, FAST included
    assert_bitwise(smp[0], full[0], "sampled vs PGMG_FLAG_FULL_CHECKS")
    assert smp[1] == full[1], (smp[1], full[1])
    assert smp[1][:2] == [sweeps, exits] and exact[1][:2] == [sweeps, exits], (smp[1], exact[1], sweeps, exits)
    if not fast:
        assert_bitwise(smp[0], exact[0], "sampled vs PGMG_FLAG_EXACT_DIST")
        assert smp[1] == exact[1], (smp[1], exact[1])
        assert_bitwise(smp[0], ref, "sampled vs the oracle")
    else:
        # FAST reorders the pass's sums (and a speculative call's carry pass and recompute form
        # are FAST passes where the in-stream call runs exact k_post / k_pre): the tolerance of
        # test_gpu_fast.py against the exact result
        for other, what in ((exact[0], "in-stream FAST"), (ref, "the oracle")):
            d = smp[0] - other
            rel = np.linalg.norm(d) / np.linalg.norm(other)
            print(f"  FAST vs {what}: rel {rel:.3e} max {np.max(np.abs(d)):.3e}")
            assert rel <= FAST_TOL and np.max(np.abs(d)) <= FAST_TOL, (what, rel)


def _res_norm(phi, f):
    h2 = (phi.shape[0] - 1.0) ** 2
    r = f[1:-1, 1:-1] - h2 * (4 * phi[1:-1, 1:-1] - phi[:-2, 1:-1] - phi[2:, 1:-1]
                              - phi[1:-1, :-2] - phi[1:-1, 2:])
    return float(np.sqrt(np.sum(r * r)))


def test_undecided_band(pgmg, oracle_mod, plan):
    """A ladder of eps (ratio 10^(1/4) = 1.78 < sqrt(6)) across the level-0 residual norms of the
    oracle's cycles: on every rung words and statistics are the oracle's; on some rung a sampled
    check could fire where the full sum does not (out[1] >= 1) -- then the context is in full-sum
    mode, still speculating, and launches no further sampled pass."""
    plan(cross_min_n=9)
    rng = np.random.default_rng(21)
    N = 129
    phi0 = rng.uniform(-1, 1, (N, N))
    f = rng.uniform(-1, 1, (N, N)) * 1e-3
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 0.0
    calls = (4, 1, 1)
    o = oracle_mod.Oracle(eps=-1.0)
    phi = phi0.copy()
    norms = []
    for _ in range(sum(calls)):
        o.v_cycle(phi, f)
        norms.append(_res_norm(phi, f))
    lo, hi = min(norms) / 10.0, max(norms) * 10.0
    ratio = 10.0 ** 0.25
    ladder = [lo * ratio ** k for k in range(int(np.ceil(np.log(hi / lo) / np.log(ratio))) + 1)]
    print(f"level-0 residual norms after each cycle: {['%.3e' % v for v in norms]}; {len(ladder)} rungs")
    landed = 0
    for eps in ladder:
        oo = oracle_mod.Oracle(eps=eps)
        ref = phi0.copy()
        for _ in range(sum(calls)):
            oo.v_cycle(ref, f)
        with pgmg.Solver(N, eps=eps, tail_n=17) as s:
            s.set_problem(phi0, f)
            s.vcycle(calls[0])
            a0, a1, a2 = s.sampled_info()
            mask = s.spec_levels()
            made = lambda: sum(s.carry_info()[1:])   # carries made, kept or dropped
            rb, carries = s.dist_info()[1], made()
            hit = a1 >= 1
            if hit:
                assert a2 == 1 and not mask & 1, (eps, (a0, a1, a2), bin(mask))
            for k in calls[1:]:
                s.vcycle(k)
                if hit:
                    b = s.sampled_info()
                    assert b[0] == a0, (eps, "a sampled pass in full-sum mode", a0, b)
                    # the call speculated: it was validated (a carry made) or rolled back
                    rb2, carries2 = s.dist_info()[1], made()
                    assert rb2 > rb or carries2 > carries, (eps, rb, rb2, carries, carries2)
                    hit = not s.spec_levels() & 1   # (a full sum that fires ends the speculation)
                    rb, carries = rb2, carries2
            print(f"eps {eps:.3e}: sampled_info after the first call {(a0, a1, a2)}, "
                  f"rollbacks {s.dist_info()[1]}, exits {oo.cut_exits}")
            assert_bitwise(s.solution(), ref, f"eps={eps:.3e}")
            assert tuple(s.stats()) == (oo.sweeps, oo.cut_exits), (eps, s.stats(), oo.sweeps, oo.cut_exits)
        landed += a1 >= 1
    assert landed >= 1, "no rung landed between a check's sampled and full norm"


def _special_problem(kind, N, row):
    """(phi0, f) with one special word in row `row` (or, "tiny", a right-hand side whose residuals
    square to 0 and whose iterates hold subnormals)"""
    phi0 = np.zeros((N, N))
    f = sv.analytic_f(N).astype(np.float64)
    col = N // 3
    if kind == "nan_f":
        f[row, col] = np.nan
    elif kind == "inf_phi":
        phi0[row, col] = np.inf
    elif kind == "ninf_phi":
        phi0[row, col] = -np.inf
    elif kind == "tiny":
        f = f * sv.SCALE["tiny", "f64"]
        f[row, col] = 5e-324
    return phi0, f


@pytest.mark.parametrize("kind", ["nan_f", "inf_phi", "ninf_phi", "tiny"])
def test_special_values_by_row(pgmg, plan, kind):
    """One special word in each of 12 consecutive rows in turn: the sampled rows repeat every 6
    (4 with a streamed f) from a band's first row, so whatever the bands' alignment the residuals
    the word reaches first lie in unsampled rows for some placements and in a sampled row for
    others.  Every placement is bitwise the in-stream run's (NaN masks equal), statistics equal."""
    plan(cross_min_n=9)
    N = 129
    for row in range(N // 2, N // 2 + 12):
        phi0, f = _special_problem(kind, N, row)
        out = []
        for flags in (0, pgmg.PGMG_FLAG_EXACT_DIST):
            with pgmg.Solver(N, flags=flags, tail_n=33) as s:
                s.set_problem(phi0, f)
                for k in (2, 1):
                    s.vcycle(k)
                out.append((s.solution(), s.stats_detail(), s.sampled_info()))
        assert out[0][2][0] > 0 and out[1][2] == (0, 0, 0), (out[0][2], out[1][2])
        sv.assert_bitwise_nan(out[0][0], out[1][0], f"{kind} row {row}")
        assert out[0][1] == out[1][1], (kind, row, out[0][1], out[1][1])


@pytest.mark.parametrize("eps", [0.0, -1.0, float("inf")])
@pytest.mark.parametrize("kind", ["plain", "nan_f", "inf_phi"])
def test_special_eps(pgmg, plan, eps, kind):
    """eps = 0 and eps < 0 (no check ever fires), eps = +Inf (every finite norm fires)."""
    plan(cross_min_n=9)
    N = 129
    phi0, f = _special_problem(kind, N, N // 2 + 1)
    out = []
    for flags in (0, pgmg.PGMG_FLAG_EXACT_DIST):
        with pgmg.Solver(N, flags=flags, eps=eps, tail_n=33) as s:
            s.set_problem(phi0, f)
            for k in SERIES:
                s.vcycle(k)
            out.append((s.solution(), s.stats_detail(), s.sampled_info(), s.dist_info()))
    print(f"eps {eps} {kind}: sampled_info {out[0][2]}, rollbacks {out[0][3][1]}, stats {out[0][1]}")
    assert out[0][2][0] > 0, out[0][2]
    sv.assert_bitwise_nan(out[0][0], out[1][0], f"eps={eps} {kind}")
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])


@pytest.mark.parametrize("N", [33, 65])
def test_bands_without_a_sampled_row(pgmg, oracle_mod, plan, N):
    """Grids whose bands are 4 rows high: the sampled row is a band's first, which in the first
    band is the boundary row, so that band sums nothing (were every partial 0 the check could
    fire: a rollback is allowed).  The words are still the oracle's."""
    plan(cross_min_n=9)
    ref, sweeps, exits = _oracle(N, "f64")
    got = _series(pgmg, N, 0, tail_n=17)
    print(f"N={N}: sampled_info {got[3]}, rollbacks {got[2][1]}")
    assert got[3][0] > 0, got[3]
    assert_bitwise(got[0], ref, f"N={N}")
    assert got[1][:2] == [sweeps, exits], (got[1], sweeps, exits)
