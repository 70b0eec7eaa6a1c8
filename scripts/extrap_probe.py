#!/usr/bin/env python3
"""Measure pgmg_solve_extrap on one MI355X (DESIGN.md §4d "Fourth-order solves").  Prints one
JSON object and saves it (default profiles/extrap/probe.json).

    python scripts/extrap_probe.py [--sizes 1025,2049,4097] [--big 16385] [--rounds 7]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.  Every shape is warmed up before it is timed (round 0 is dropped).  The problem
is the analytic one with p = q = 1 from phi = 0 (its exact frame is zero), eps < 0, nu = 2,
rtol = 0 and atol = max(--atol, 0.8 N^2 2^-52) * ||f||_2 with ||f||_2 = pi^2 (N - 1) (the
analytic value for p = q = 1, a = 1; the second term is twice the floor fp64 residuals reach,
above 1e-10 from N = 2049 up), at most 40 cycles.
  time_N  solve(order=4, damp) against solve(damp, start="fmg", boundary="keep") with the same
          options, alternated in one process: host wall ms of each (the extrapolated call's own
          elapsed_ms; perf_counter around the two calls of the second-order one), extrap_ms, the
          cycle counts and both rel_errors; medians over the rounds and the ratio.
  headline  N = --small extrapolated beside N = --big second order (its atol --big-atol: the
          target of the small size lies below what fp64 residuals reach at the big one): wall
          ms and rel_error of each.
  passes_N  at --big: extrap_ms of solve(order=4, max_cycles=0) (both FMG climbs, check 0, the
          extrapolation) and pgmg_fmg_interp_time in the same process, each with its algorithmic
          bytes and its fraction of the 8 TB/s peak.
"""
import argparse
import json
import math
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

PEAK = 8.0e12


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def fnorm(n):
    return math.pi ** 2 * (n - 1)


def second_order(s, a, atol, max_cycles=40):
    s.set_problem()
    t0 = time.perf_counter()
    info = s.solve(damp=a.omega, start="fmg", boundary="keep", rtol=0.0, atol=atol,
                   max_cycles=max_cycles)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, info, s.monitor(error=True).rel_error


def fourth_order(s, a, atol, max_cycles=40):
    s.set_problem()
    info = s.solve(order=4, damp=a.omega, rtol=0.0, atol=atol, max_cycles=max_cycles)
    return info.total_ms, info, s.monitor(error=True).rel_error


def rel_atol(a, n):
    """--atol, but no lower than twice the floor fp64 residuals reach, 0.4 N^2 2^-52"""
    return max(a.atol, 0.8 * n * n * 2.0 ** -52)


def step_time(a):
    import _pkgload
    pg = _pkgload.load()
    atol = rel_atol(a, a.n) * fnorm(a.n)
    t2, t4, tx = [], [], []
    with pg.Solver(a.n, eps=-1.0) as s:
        for rnd in range(a.rounds + 1):
            ms4, i4, e4 = fourth_order(s, a, atol)
            ms2, i2, e2 = second_order(s, a, atol)
            if rnd:
                t2.append(ms2)
                t4.append(ms4)
                tx.append(i4.extrap_ms)
    return {"n": a.n, "omega": a.omega, "atol_over_fnorm": rel_atol(a, a.n), "rounds": a.rounds,
            "order2_wall_ms": spread(t2), "order4_wall_ms": spread(t4), "extrap_ms": spread(tx),
            "ratio_order4_over_order2": round(statistics.median(t4) / statistics.median(t2), 4),
            "order2": {"cycles": i2.cycles, "reason": i2.reason, "rel_error": e2},
            "order4": {"cycles": i4.cycles, "reason": i4.reason, "coarse_cycles": i4.coarse.cycles,
                       "coarse_reason": i4.coarse.reason, "rel_error": e4}}


def step_headline(a):
    import _pkgload
    pg = _pkgload.load()
    out = {"small_n": a.small, "big_n": a.n, "omega": a.omega}
    t = []
    with pg.Solver(a.small, eps=-1.0) as s:
        for rnd in range(a.rounds + 1):
            ms, info, err = fourth_order(s, a, a.atol * fnorm(a.small))
            if rnd:
                t.append(ms)
    out["small_order4"] = {"wall_ms": spread(t), "rel_error": err, "cycles": info.cycles,
                           "coarse_cycles": info.coarse.cycles, "atol_over_fnorm": a.atol}
    t = []
    with pg.Solver(a.n, eps=-1.0) as s:
        for rnd in range(3):
            ms, info, err = second_order(s, a, a.big_atol * fnorm(a.n), max_cycles=10)
            if rnd:
                t.append(ms)
    out["big_order2"] = {"wall_ms": spread(t), "rel_error": err, "cycles": info.cycles,
                         "reason": info.reason, "atol_over_fnorm": a.big_atol, "timed_rounds": 2}
    out["error_ratio_big2_over_small4"] = out["big_order2"]["rel_error"] / out["small_order4"]["rel_error"]
    out["time_ratio_big2_over_small4"] = round(
        out["big_order2"]["wall_ms"]["median"] / out["small_order4"]["wall_ms"]["median"], 2)
    return out


def step_passes(a):
    import _pkgload
    pg = _pkgload.load()
    n, nc = a.n, (a.n + 1) // 2
    b1 = 8.0 * nc * n + 8.0 * nc * nc + 8.0 * nc * nc
    b2 = 8.0 * nc * nc + 16.0 * n * n
    tx = []
    with pg.Solver(n, eps=-1.0) as s:
        for rnd in range(a.rounds + 1):
            s.set_problem()
            info = s.solve(order=4, damp=a.omega, rtol=0.0, atol=0.0, max_cycles=0)
            if rnd:
                tx.append(info.extrap_ms)
        s.set_problem()
        ims, ib = s.fmg_interp_time(reps=20)
    x = statistics.median(tx)
    out = {"n": n, "rounds": a.rounds, "extrap_ms": spread(tx), "extrap_bytes": b1 + b2,
           "extrap_bytes_per_fine_point": round((b1 + b2) / (n * n), 3),
           "extrap_fraction_of_peak": round((b1 + b2) / (x * 1e-3) / PEAK, 4),
           "interp_ms": round(ims, 5), "interp_bytes": ib,
           "interp_fraction_of_peak": round(ib / (ims * 1e-3) / PEAK, 4)}
    out["extrap_over_interp_fraction"] = round(out["extrap_fraction_of_peak"] /
                                               out["interp_fraction_of_peak"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--sizes", default="1025,2049,4097")
    ap.add_argument("--big", type=int, default=16385)
    ap.add_argument("--small", type=int, default=1025)
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--atol", type=float, default=1e-10, help="atol / ||f||_2")
    ap.add_argument("--big-atol", type=float, default=1e-7, help="atol / ||f||_2 at --big")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "extrap" / "probe.json"))
    ap.add_argument("--step", choices=["time", "headline", "passes"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    if a.step:
        fn = {"time": step_time, "headline": step_headline, "passes": step_passes}[a.step]
        print(json.dumps(fn(a)))
        return 0
    res = {"rounds": a.rounds, "omega": a.omega}
    steps = [(f"time_{n}", "time", n) for n in (int(x) for x in a.sizes.split(","))]
    steps += [("headline", "headline", a.big), (f"passes_{a.big}", "passes", a.big)]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--small", str(a.small), "--omega", str(a.omega), "--atol",
               str(a.atol), "--big-atol", str(a.big_atol), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"step {name} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}",
                  file=sys.stderr)
            return 1
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"{name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
