"""Speculative calls on converged coarse levels (pgmg_spec.hip "predicted to fire", "segment
planning"), against the same solver with every check decided in-stream (PGMG_FLAG_EXACT_DIST).

On the reference problem the bulk levels above the tail reach eps after ~27 V-cycles and from
then on fire at every check.  A speculative call ends its segment just before a level's
predicted crossing (the level speculates until then), decides the crossing levels in-stream,
and once a level's last two visits were below eps / 4 it is enqueued with its checks
predicted to FIRE (k_pre1 / k_post1, one launch each instead of a pass plus a rare path),
confirmed by the validation; a failed prediction rolls the call back.  Tolerance: EXACT
(bitwise phi, equal sweep and exit counts).
"""
import numpy as np
import pytest

from conftest import assert_bitwise

pytestmark = pytest.mark.gpu


def _calls(pgmg, N, calls, flags=0, kind="V"):
    with pgmg.Solver(N, flags=flags) as s:
        s.set_problem()
        run = {"V": s.vcycle, "W": s.wcycle, "F": s.fcycle}[kind]
        masks = []
        for n in calls:
            run(n)
            masks.append(s.spec_fire_levels() if kind == "V" else s.spec_visit_modes())
        return s.solution(), s.stats_detail(), s.dist_info(), masks


@pytest.mark.parametrize("N,calls", [(2049, [3, 40]), (4097, [3, 40]), (2049, [60]),
                                     (2049, [1] * 45), (2049, [7] * 8), (4097, [5, 20, 20])])
def test_fire_prediction_bitwise(pgmg, oracle_mod, golden_cycles, N, calls):
    phi, det, info, masks = _calls(pgmg, N, calls)
    ref, rdet, _, _ = _calls(pgmg, N, calls, flags=pgmg.PGMG_FLAG_EXACT_DIST)
    assert_bitwise(phi, ref, f"N={N} calls={calls}")
    assert det == rdet
    # BASELINE configs[1]'s call shapes at 4097 against the reference's own 43 cycles
    case = next((c for c in golden_cycles if c["kind"] == "V" and c["N"] == N
                 and c["eps"] == 1e-7 and len(c["cycles"]) >= sum(calls)), None)
    if case is not None:
        want = case["cycles"][sum(calls) - 1]
        assert oracle_mod.fnv_hash(phi) == want["hash"], (N, calls)
        assert det[0] == want["sweeps"], (N, calls, det, want)
    assert info[0] and info[1] == 0, info      # speculative, never rolled back
    # 129 / 257 fire from cycles 27 / 30 at 2049 and fall under eps/4 a few cycles later; a
    # 3 + 40 call ends before a split for them pays (segment planning), longer runs get there
    if N == 2049 and sum(calls) >= 45:
        assert masks[-1] & ~1, masks            # converged coarse levels predicted to fire


@pytest.mark.parametrize("kind,N,calls", [("W", 4097, [1] * 5), ("W", 1025, [1] * 10),
                                          ("W", 2049, [2, 3]), ("W", 513, [3, 3]),
                                          ("F", 2049, [2, 8]), ("F", 1025, [1] * 12)])
def test_fire_prediction_w_f_bitwise(pgmg, kind, N, calls):
    """W- and F-cycles: the second and third gamma visits of a level start from the previous
    visit's iterate, not from 0; their predicted-to-fire passes read x0 and store x1 (k_pre1 /
    k_post1 without RECOMP).  W calls speculate on one GPU at every N (pgmg_cycle.hip "W-cycle
    plans": each visit of a bulk level planned from the same visit of the previous cycle);
    F-cycles run in-stream."""
    phi, det, info, masks = _calls(pgmg, N, calls, kind=kind)
    ref, rdet, _, _ = _calls(pgmg, N, calls, flags=pgmg.PGMG_FLAG_EXACT_DIST, kind=kind)
    assert_bitwise(phi, ref, f"{kind} N={N} calls={calls}")
    assert det == rdet
    print(kind, N, calls, "visit modes (no fire, fire, in-stream)", masks, "rollbacks", info[1])
    if kind == "W":   # W plans: a failed prediction ends them for the problem (one rollback)
        assert info[1] <= 1, info
    if kind == "W" and N == 4097:   # from the second call on most visits are planned
        assert info[1] == 0 and masks[-1][0] > 0 and masks[-1][1] > 0, masks


def test_fire_prediction_golden(pgmg, plan, golden_cycles):
    """The reference's own 30-cycle hashes and sweep counts at N = 513 with the cross-fused
    speculative path (cross_min_n = 9): one call, calls of 10 and calls of 1."""
    plan(cross_min_n=9)
    case = next(c for c in golden_cycles if c["kind"] == "V" and c["N"] == 513
                and c["eps"] == 1e-7 and len(c["cycles"]) >= 30)
    want = case["cycles"][29]
    for calls in ([30], [10, 10, 10], [1] * 30, [3, 27]):
        with pgmg.Solver(513) as s:
            s.set_problem()
            for n in calls:
                s.vcycle(n)
            assert s.solution_hash(0) == want["hash"], calls
            assert s.stats()[0] == want["sweeps"], calls


def test_failed_fire_prediction_rolls_back(pgmg, oracle_mod):
    """A device-bound problem whose right-hand side the caller changes between calls: after
    the coarse levels converged (predicted to fire), f gets a large random perturbation in
    place, so the next call's "fires" predictions fail -- the call is rolled back and rerun
    in-stream, bitwise the in-stream solver's result."""
    import torch
    N = 2049
    f0 = oracle_mod.Oracle().rhs(N)
    rng = np.random.default_rng(3)
    bump = torch.tensor(rng.uniform(-1, 1, (N, N)), device="cuda:0")
    out = []
    for flags in (0, pgmg.PGMG_FLAG_EXACT_DIST):
        phi = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
        f = torch.tensor(f0, device="cuda:0")
        with pgmg.Solver(N, flags=flags) as s:
            s.set_problem_device(phi, f)
            for _ in range(12):
                s.vcycle(4)
            fire = s.spec_fire_levels()
            f.add_(bump)
            torch.cuda.synchronize()
            s.vcycle(4)
            out.append((phi.cpu().numpy(), s.stats_detail(), s.dist_info(), fire))
    (a, da, ia, fire), (b, db, _, _) = out
    assert fire & ~1, bin(fire)
    assert ia[1] >= 1, ia
    assert_bitwise(a, b, "after the rollback")
    assert da == db


def test_history_reset_by_set_eps_and_set_problem(pgmg):
    """The speculation history has one reset, shared by pgmg_set_eps and a new problem: after
    either, no level is marked (in-stream or predicted to fire), the rollback count stands, and
    the solver goes on exactly as one that never had the history.  N = 2049, 3 + 40 V-cycles:
    the smallest shape here whose coarse levels get marked (smaller grids are not cross-fused
    and do not speculate on V-cycles, so their spec_levels() bit 0 is constant)."""
    N, calls = 2049, (3, 40)

    def marks(s):
        return s.spec_fire_levels() | s.spec_levels()

    def three_more(s):
        before = s.stats()
        s.vcycle(3)
        return s.solution_hash(), tuple(a - b for a, b in zip(s.stats(), before))

    with pgmg.Solver(N) as s, pgmg.Solver(N, flags=pgmg.PGMG_FLAG_EXACT_DIST) as ref:
        for x in (s, ref):
            x.set_problem()
            for n in calls:
                x.vcycle(n)
        assert marks(s) != 0, "no level marked: the resets below would pass vacuously"
        rollbacks = s.dist_info()[1]
        s.set_eps(s.cfg.eps)
        assert (s.spec_levels(), s.spec_fire_levels()) == (0, 0)
        assert s.dist_info()[1] == rollbacks
        assert three_more(s) == three_more(ref)      # the in-stream solver from the same state

        for n in calls:
            s.vcycle(n)
        assert marks(s) != 0
        s.set_problem()
        assert (s.spec_levels(), s.spec_fire_levels()) == (0, 0)
        with pgmg.Solver(N) as fresh:
            fresh.set_problem()
            assert three_more(s) == three_more(fresh)
