#!/usr/bin/env python3
"""Measure pgmg_gradient on one MI355X (DESIGN.md §4e "Gradient of the solution").  Prints one
JSON object and saves it (default profiles/gradient/probe.json).

    python scripts/gradient_probe.py [--sizes 1025,4097,16385] [--error-sizes 1025,2049]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N_dtype  on the analytic problem after one V-cycle, alternated in one process over
          --rounds timed rounds after one dropped warm round: pgmg_gradient_time at order 2 and at
          order 4 (both components and the norm, 20 passes each), pgmg_monitor_time (residual)
          and pgmg_fmg_interp_time (k_interp_cubic, level 1 -> level 0; it overwrites phi, which
          the other passes only read).  Per pass: min / median / max of the rounds' ms, the
          algorithmic bytes and the fraction of the 8 TB/s peak at the median.
  error_N  the analytic problem with p = q = 1 from phi = 0 (its exact frame is zero), eps < 0,
          nu = 2, omega = 0.5, rtol = 0, atol = max(1e-10, 0.8 N^2 2^-52) ||f||_2, at most 40
          cycles: the relative error of the field, sqrt(sum (gx - u_x)^2 + (gy - u_y)^2) /
          sqrt(sum u_x^2 + u_y^2) over all points, for the second-order solve and for
          solve(order=4), each with both stencil orders.
"""
import argparse
import json
import math
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

PEAK = 8.0e12
REPS = 20


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    runs = {"gradient_order2": lambda s: s.gradient_time(order=2, reps=REPS),
            "gradient_order4": lambda s: s.gradient_time(order=4, reps=REPS),
            "monitor": lambda s: s.monitor_time(reps=REPS),
            "interp_cubic": lambda s: s.fmg_interp_time(reps=REPS)}
    ms = {k: [] for k in runs}
    nbytes = {}
    with pg.Solver(a.n, dtype=a.dtype) as s:
        s.set_problem()
        s.vcycle(1)
        for rnd in range(a.rounds + 1):
            for k, fn in runs.items():
                t, b = fn(s)
                nbytes[k] = b
                if rnd:
                    ms[k].append(t)
    out = {"n": a.n, "dtype": a.dtype, "rounds": a.rounds, "reps": REPS}
    for k in runs:
        med = statistics.median(ms[k])
        out[k] = {"ms": spread(ms[k]), "bytes": nbytes[k],
                  "bytes_per_point": round(nbytes[k] / (a.n * a.n), 3),
                  "fraction_of_peak": round(nbytes[k] / (med * 1e-3) / PEAK, 4)}
    return out


def step_error(a):
    import numpy as np
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    atol = max(1e-10, 0.8 * n * n * 2.0 ** -52) * math.pi ** 2 * (n - 1)
    t = np.arange(n) / (n - 1)
    ux = np.pi * np.outer(np.sin(np.pi * t), np.cos(np.pi * t))
    uy = np.pi * np.outer(np.cos(np.pi * t), np.sin(np.pi * t))
    den = float(np.sqrt(np.sum(ux ** 2 + uy ** 2)))

    def err(s, order):
        gx, gy = s.gradient(order=order)
        gx, gy = gx.cpu().numpy(), gy.cpu().numpy()
        return float(np.sqrt(np.sum((gx - ux) ** 2 + (gy - uy) ** 2))) / den

    out = {"n": n, "atol": atol}
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem()
        i2 = s.solve(damp=0.5, start="fmg", boundary="keep", rtol=0.0, atol=atol, max_cycles=40)
        out["phi2"] = {"cycles": i2.cycles, "reason": i2.reason,
                       "rel_error": s.monitor(error=True).rel_error,
                       "field_error_order2": err(s, 2), "field_error_order4": err(s, 4)}
        s.set_problem()
        i4 = s.solve(order=4, damp=0.5, rtol=0.0, atol=atol, max_cycles=40)
        out["phi4"] = {"cycles": i4.cycles, "reason": i4.reason, "coarse_cycles": i4.coarse.cycles,
                       "rel_error": s.monitor(error=True).rel_error,
                       "field_error_order2": err(s, 2), "field_error_order4": err(s, 4)}
    out["gain_phi4_order4_over_phi2_order2"] = (out["phi2"]["field_error_order2"] /
                                                out["phi4"]["field_error_order4"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--sizes", default="1025,4097,16385")
    ap.add_argument("--error-sizes", default="1025,2049")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gradient" / "probe.json"))
    ap.add_argument("--step", choices=["pass", "error"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    if a.step:
        print(json.dumps({"pass": step_pass, "error": step_error}[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "peak_bytes_per_s": PEAK}
    steps = [(f"pass_{n}_{dt}", "pass", n, dt) for n in (int(x) for x in a.sizes.split(","))
             for dt in ("f64", "f32")]
    steps += [(f"error_{n}", "error", n, "f64") for n in (int(x) for x in a.error_sizes.split(","))]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n, dt in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--dtype", dt, "--rounds", str(a.rounds)]
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
