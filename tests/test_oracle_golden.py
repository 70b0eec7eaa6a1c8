"""CPU: pin the oracle (oracle/pgmg_oracle.c) to the reference's own outputs.

The golden fixtures in tests/golden/ were produced by the reference's CPU multigrid
(2_part_MG/MultiGrid.hpp, Smoother.hpp, DynamicGridUtils.hpp) compiled unmodified by
oracle/Makefile and driven by oracle/ref_harness.cpp (tests/golden/make_golden.py).
"""
import numpy as np
import pytest

from conftest import GOLDEN, assert_bitwise

MAX_N_CPU = 1025  # keep the CPU suite to a few minutes


def _cases(golden_cycles):
    return [c for c in golden_cycles if c["N"] <= MAX_N_CPU]


def test_golden_cycles_hashes(oracle_mod, golden_cycles):
    """Every cycle's FNV hash, centre value, residual norm and sweep count match."""
    checked = 0
    for case in _cases(golden_cycles):
        kind, N, eps = case["kind"], case["N"], case["eps"]
        o = oracle_mod.Oracle(eps=eps)
        f = o.rhs(N)
        phi = np.zeros((N, N))
        h = 1.0 / (N - 1)
        for row in case["cycles"]:
            if kind == "V":
                o.v_cycle(phi, f)
            elif kind == "W":
                o.w_cycle(phi, f)
            else:
                o.f_cycle_outer(phi)
            tag = f"{kind} N={N} eps={eps} cycle={row['cycle']}"
            assert oracle_mod.fnv_hash(phi) == row["hash"], tag
            assert phi[N // 2, N // 2] == row["center"], tag
            assert o.sweeps == row["sweeps"], tag
            assert o.early_exits == row["exits"], tag
            r = oracle_mod.residual(phi, f, h)
            assert oracle_mod.norm(r) == row["res"], tag
            assert o.rel_error(phi) == row["relerr"], tag
            checked += 1
    assert checked > 100


def test_golden_cycles_params_hashes(oracle_mod):
    """The oracle off the defaults: alpha and n_coarse against the reference's own
    MultigridSolver (tests/golden/cycles_params.json, written by make_golden.py from
    oracle/_ref/ref_harness with alpha as the constructor argument and N_coarse set).  Every
    cycle's hash, centre value, sweep and exit counts, residual norm and relative error.

    coarse_iter cannot be pinned this way: the reference fixes it as the literal 10
    (MultiGrid.hpp:61, :100).  For coarse_iter the oracle's own
    orc_smooth_alloc(c, ..., c->coarse_iter) at the recursion floor is the definition."""
    import json
    cases = json.loads((GOLDEN / "cycles_params.json").read_text())
    checked = 0
    seen = set()
    for case in cases:
        kind, N, eps = case["kind"], case["N"], case["eps"]
        alpha, n_coarse = case["alpha"], case["n_coarse"]
        assert N <= 257 and len(case["cycles"]) <= 4
        seen.add((kind, alpha, n_coarse))
        o = oracle_mod.Oracle(eps=eps, alpha=alpha, n_coarse=n_coarse)
        f = o.rhs(N)
        phi = np.zeros((N, N))
        h = 1.0 / (N - 1)
        for row in case["cycles"]:
            if kind == "V":
                o.v_cycle(phi, f)
            elif kind == "W":
                o.w_cycle(phi, f)
            else:
                o.f_cycle_outer(phi)
            tag = f"{kind} N={N} eps={eps} alpha={alpha} n_coarse={n_coarse} cycle={row['cycle']}"
            assert oracle_mod.fnv_hash(phi) == row["hash"], tag
            assert phi[N // 2, N // 2] == row["center"], tag
            assert o.sweeps == row["sweeps"], tag
            assert o.early_exits == row["exits"], tag
            r = oracle_mod.residual(phi, f, h)
            assert oracle_mod.norm(r) == row["res"], tag
            assert o.rel_error(phi) == row["relerr"], tag
            checked += 1
    # the fixture covers what it is there for (a regenerated file cannot quietly shrink)
    assert {a for k, a, _ in seen if k == "W"} >= {1, 2, 4, 15}
    for kind, floors in (("V", {3, 9, 17, 33, 65, 100}), ("W", {3, 9, 17}), ("F", {3, 9})):
        assert {n for k, _, n in seen if k == kind} >= floors, kind
    assert checked >= 90


def test_golden_cycles_problem_hashes(oracle_mod):
    """The oracle with the problem's constants off the defaults: a, p, q (the reference's
    globals, globals.cpp:2-4) and, for V and W, the caller's mesh width h (MultiGrid.hpp:57's
    argument, also compute_rhs's, compute_exact_solution's and compute_residual's) against the
    reference's own code (tests/golden/cycles_problem.json, written by make_golden.py from
    oracle/_ref/ref_harness).  Every cycle's hash, centre value, sweep and exit counts,
    residual norm and relative error.  A relerr of null is the reference's NaN: p = 0, where
    the exact solution is 0 everywhere and ||e|| / ||u|| is 0 / 0."""
    import json
    import math
    cases = json.loads((GOLDEN / "cycles_problem.json").read_text())
    checked = 0
    seen, hs = set(), set()
    for case in cases:
        kind, N, eps = case["kind"], case["N"], case["eps"]
        a, p, q, h = case["a"], case["p"], case["q"], case["h"]
        assert N <= 129 and len(case["cycles"]) <= 3
        assert h is None or kind != "F"
        seen.add((kind, a, p, q))
        if h is not None:
            hs.add((kind, "H1" if h == 0.7 / (N - 1) else "H2" if h == 1.0 / N else h))
        o = oracle_mod.Oracle(eps=eps, a=a, p=p, q=q)
        hh = a / (N - 1) if h is None else h
        f = o.rhs(N, hh)
        phi = np.zeros((N, N))
        for row in case["cycles"]:
            if kind == "V":
                o.v_cycle(phi, f, hh)
            elif kind == "W":
                o.w_cycle(phi, f, hh)
            else:
                o.f_cycle_outer(phi)
            tag = f"{kind} N={N} eps={eps} a={a} p={p} q={q} h={h} cycle={row['cycle']}"
            assert oracle_mod.fnv_hash(phi) == row["hash"], tag
            assert phi[N // 2, N // 2] == row["center"], tag
            assert o.sweeps == row["sweeps"], tag
            assert o.early_exits == row["exits"], tag
            r = oracle_mod.residual(phi, f, hh)
            assert oracle_mod.norm(r) == row["res"], tag
            if row["relerr"] is None:
                assert p == 0 and math.isnan(o.rel_error(phi, hh)), tag
            else:
                assert o.rel_error(phi, hh) == row["relerr"], tag
                if h is None:   # the entry without h is the same at a / (N - 1)
                    assert o.rel_error(phi) == row["relerr"], tag
            checked += 1
    # the fixture covers what it is there for (a regenerated file cannot quietly shrink)
    sets = {(1.0, 2.0, 3.0), (2.0, 1.0, 1.0), (3.0, 2.0, 1.0), (0.5, 3.0, 5.0), (1.0, 0.5, 1.5),
            (1.0, -1.0, 2.0), (1.0, 0.0, 1.0), (1000.0, 2.0, 2.0), (1e-3, 1.0, 1.0),
            (-2.0, 1.0, 2.0)}
    for kind in "VWF":
        mine = {(a, p, q) for k, a, p, q in seen if k == kind}
        assert mine >= sets, (kind, sets - mine)
        assert any(p >= 31 and q == 1 for a, p, q in mine), kind          # P8: p = N - 2
        assert any(math.log2(abs(a)) % 1 for a, p, q in mine), kind       # a non-dyadic a
        assert any(p % 1 for a, p, q in mine), kind                       # a non-integer p
        assert any(p != q for a, p, q in mine), kind
    for kind in "VW":
        assert {t for k, t in hs if k == kind} >= {"H1", "H2"}, kind
    assert checked >= 140


@pytest.mark.parametrize("name", sorted(p.name for p in GOLDEN.glob("phi_*.npy")))
def test_golden_phi_vectors(oracle_mod, name):
    stem = name[len("phi_"):-len(".npy")]
    kind, rest = stem[0], stem[1:]
    parts = rest.split("_")
    N = int(parts[0])
    k = int(parts[1][1:])
    eps = float(parts[2][3:]) if len(parts) > 2 else 1e-7
    ref = np.load(GOLDEN / name, allow_pickle=False)
    phi, _ = oracle_mod.run_cycles(kind, N, k, eps=eps)
    assert_bitwise(phi, ref, name)


@pytest.mark.parametrize("N", [17, 33, 65])
def test_golden_ops(oracle_mod, N):
    z = np.load(GOLDEN / f"ops_N{N}.npz", allow_pickle=False)
    x, f, e, h, eps = z["x"], z["f"], z["e"], float(z["h"]), float(z["eps"])
    assert_bitwise(oracle_mod.residual(x, f, h), z["residual"], "residual")
    assert_bitwise(oracle_mod.restrict(x), z["restrict"], "restrict")
    assert_bitwise(oracle_mod.prolong(x, e), z["prolong"], "prolong")
    for it, key in ((1, "smooth1"), (10, "smooth10")):
        o = oracle_mod.Oracle(eps=eps)
        s = x.copy()
        o.smooth(s, f, h, it)
        assert_bitwise(s, z[key], key)


def test_prolongation_quirk(oracle_mod):
    """interior-ones 5x5 coarse -> fine row/col 1 stay 0, Nf-2 gets 0.5."""
    c = np.zeros((5, 5))
    c[1:4, 1:4] = 1.0
    fine = oracle_mod.prolong(np.zeros((9, 9)), c)
    assert np.all(fine[1, :] == 0) and np.all(fine[:, 1] == 0)
    assert np.all(fine[2:7, 2:7] == 1.0)
    assert np.all(fine[7, 2:7] == 0.5) and np.all(fine[2:7, 7] == 0.5)


def test_restriction_of_ones(oracle_mod):
    c = oracle_mod.restrict(np.ones((9, 9)))
    assert np.all(c[1:4, 1:4] == 1.0)
    assert c[0].sum() == 0 and c[-1].sum() == 0 and c[:, 0].sum() == 0 and c[:, -1].sum() == 0
