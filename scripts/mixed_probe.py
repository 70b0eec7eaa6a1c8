#!/usr/bin/env python3
"""Measure pgmg_solve_mixed on one MI355X (DESIGN.md §4g "Mixed-precision refinement").  Prints
one JSON object and saves it (default profiles/mixed/probe.json).

    python scripts/mixed_probe.py [--sizes 1025,4097,16385] [--rounds 7]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.  Every shape is warmed up before it is timed (round 0 is dropped); the routes of
one comparison alternate in one process.  eps < 0, omega = 0.5, rtol = 0, phi = 0 at the start.
  solve_N   per problem (oracle.rhs_mt64 with a zero frame as a caller's f; the analytic one with
            p = q = 1) and per target atol / ||f||_2 (--atols; on the analytic problem no lower
            than 0.8 N^2 2^-52, twice the floor its fp64 residual reaches -- targets that
            collapse onto that bound are measured once): solve_mixed with nu = 2 and nu = 3
            (host wall ms of the call, steps, reason, the three device times) against
            solve(damp, start="fmg", boundary="keep") on the same context (perf_counter around
            the call, cycles, reason); medians over the rounds and the ratio mixed / fp64,
            whichever way it falls.
  passes_N  pgmg_mixed_time of both passes beside pgmg_monitor_time and pgmg_damp_time in the
            same process, each with its algorithmic bytes and its fraction of the 8 TB/s peak;
            and the fp32 context's fmg(nu, damp) at nu = 2 and 3: device ms between the call's
            own events and host wall ms to the sync.
"""
import argparse
import json
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


def problems(n):
    """[(name, f or None, ||f||_2 over the interior)]"""
    import math
    import numpy as np
    import oracle
    f = np.array(oracle.rhs_mt64(n))
    return [("mt64", f, float(np.linalg.norm(f[1:-1, 1:-1]))),
            ("analytic", None, math.pi ** 2 * (n - 1))]


def step_solve(a):
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    out = {"n": n, "omega": a.omega, "rounds": a.rounds, "problems": {}}
    with pg.Solver(n, eps=-1.0) as s:
        for name, f, fn in problems(n):
            floor = 0.8 * n * n * 2.0 ** -52 if f is None else 0.0
            targets = sorted({max(t, floor) for t in a.atol_list}, reverse=True)
            res = []
            for rel in targets:
                atol = rel * fn
                t = {"mixed_nu2": [], "mixed_nu3": [], "fp64": []}
                dev = {"mixed_nu2": [], "mixed_nu3": []}
                last = {}
                for rnd in range(a.rounds + 1):
                    for nu in (2, 3):
                        s.set_problem(None, f)
                        info = s.solve_mixed(atol=atol, max_steps=a.max_steps, nu=nu, damp=a.omega)
                        key = f"mixed_nu{nu}"
                        last[key] = {"steps": info.cycles, "reason": info.reason,
                                     "res_over_fnorm": info.res / fn,
                                     "inner_sweeps": info.inner_sweeps}
                        if rnd:
                            t[key].append(info.total_ms)
                            dev[key].append((info.defect_ms, info.inner_ms, info.correct_ms))
                    s.set_problem(None, f)
                    t0 = time.perf_counter()
                    info = s.solve(damp=a.omega, start="fmg", boundary="keep", rtol=0.0, atol=atol,
                                   max_cycles=a.max_cycles)
                    ms = (time.perf_counter() - t0) * 1e3
                    last["fp64"] = {"cycles": info.cycles, "reason": info.reason,
                                    "res_over_fnorm": info.res / fn}
                    if rnd:
                        t["fp64"].append(ms)
                rec = {"atol_over_fnorm": rel}
                for key in t:
                    rec[key] = dict(last[key], wall_ms=spread(t[key]))
                for key in dev:
                    k = max(last[key]["steps"], 1)
                    rec[key]["defect_ms_per_check"] = round(
                        statistics.median(d[0] for d in dev[key]) / (last[key]["steps"] + 1), 5)
                    rec[key]["inner_ms_per_step"] = round(statistics.median(d[1] for d in dev[key]) / k, 5)
                    rec[key]["correct_ms_per_step"] = round(statistics.median(d[2] for d in dev[key]) / k, 5)
                    rec[key]["ratio_over_fp64"] = round(
                        rec[key]["wall_ms"]["median"] / rec["fp64"]["wall_ms"]["median"], 4)
                res.append(rec)
            out["problems"][name] = res
    return out


def step_passes(a):
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    out = {"n": n, "reps": a.reps}

    def frac(ms, b):
        return {"ms": round(ms, 5), "bytes": b, "fraction_of_peak": round(b / (ms * 1e-3) / PEAK, 4)}

    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem()
        s.mixed_time(0, reps=2)          # (creates the fp32 context)
        runs = {"defect": lambda: s.mixed_time(0, reps=a.reps),
                "correct": lambda: s.mixed_time(1, reps=a.reps),
                "monitor": lambda: s.monitor_time(reps=a.reps),
                "damp": lambda: s.damp_time(a.omega, reps=a.reps)}
        t = {k: [] for k in runs}
        b = {}
        for rnd in range(a.rounds + 1):
            for k, fn in runs.items():
                ms, b[k] = fn()
                if rnd:
                    t[k].append(ms)
        for k in runs:
            out[k] = dict(frac(statistics.median(t[k]), b[k]), ms_spread=spread(t[k]))
        out["defect_over_monitor_fraction"] = round(out["defect"]["fraction_of_peak"] /
                                                    out["monitor"]["fraction_of_peak"], 4)
    with pg.Solver(n, eps=-1.0, dtype="f32") as s:
        for nu in (2, 3):
            dev, wall = [], []
            for rnd in range(a.rounds + 1):
                s.set_problem()
                s.sync()
                t0 = time.perf_counter()
                s.fmg(nu, a.omega)
                s.sync()
                w = (time.perf_counter() - t0) * 1e3
                if rnd:
                    wall.append(w)
                    dev.append(s.last_elapsed_ms())
            out[f"fp32_fmg_damped_nu{nu}"] = {"device_ms": spread(dev), "wall_ms": spread(wall)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--sizes", default="1025,4097,16385")
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--atols", default="1e-9,1e-11", help="targets atol / ||f||_2")
    ap.add_argument("--max-steps", type=int, default=8)
    ap.add_argument("--max-cycles", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixed" / "probe.json"))
    ap.add_argument("--step", choices=["solve", "passes"])
    ap.add_argument("--timeout", type=int, default=420, help="seconds per step")
    a = ap.parse_args()
    a.atol_list = [float(x) for x in a.atols.split(",")]
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    if a.step:
        print(json.dumps({"solve": step_solve, "passes": step_passes}[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "omega": a.omega}
    sizes = [int(x) for x in a.sizes.split(",")]
    steps = [(f"passes_{n}", "passes", n) for n in sizes] + [(f"solve_{n}", "solve", n) for n in sizes]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--omega", str(a.omega), "--atols", a.atols, "--max-steps",
               str(a.max_steps), "--max-cycles", str(a.max_cycles), "--rounds", str(a.rounds),
               "--reps", str(a.reps)]
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
