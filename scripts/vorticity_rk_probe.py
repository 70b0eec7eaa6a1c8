#!/usr/bin/env python3
"""Measure pgmg_vorticity_step_rk on one MI355X (DESIGN.md §4h "Runge-Kutta time stepping").
Prints one JSON object and saves it (default profiles/vorticity_rk/probe.json).

    python scripts/vorticity_rk_probe.py [--sizes 4097,16385] [--call-sizes 1025,4097]
                                         [--cavity-sizes 129]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N    on the analytic problem after one V-cycle, alternated in one process over --rounds timed
            rounds after one dropped warm round: pgmg_vorticity_rk_time(0) (the stage with its copy
            back, 48 B per point) and (1) (the stage with vmax, 32 B per point), beside
            pgmg_vorticity_time(0) and (1) (the Euler pass: 40 and 24 B per point).  Per pass: min /
            median / max of the rounds' ms, the algorithmic bytes and the fraction of the 8 TB/s
            peak at the median.
  call_N    one whole order-3 step of the lid cavity at Re = 100 (started from 20 Euler steps)
            against three Euler steps of the same dt, alternated in one process, each from the
            same state.  Host wall ms, and the cycles each side took.
  cavity_N  the lid-driven cavity at Re = 1000 from rest to T = 100, atol = 1e-6, at most 30 cycles
            per solve, at order 3 and at order 1, each at dt = h (cfl about 0.9, diffusion
            4 nu dt / h^2 = 0.51 at N = 129) and at dt = 1.6 h (cfl about 1.4, diffusion 0.82): the
            minimum of psi and the minimum of u on the vertical centreline beside Ghia et al.'s
            (-0.1179, -0.3829), the cycles and the wall time; a run that leaves the finite numbers
            is stopped and reported as such.
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
sys.path.insert(0, str(ROOT / "tests"))

PEAK = 8.0e12
REPS = 20
WALLS = (0.0, 1.0, 0.0, 0.0)
RULE = dict(rtol=0.0, atol=1e-6, max_cycles=30)


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    runs = {"stage_with_copy": lambda s: s.vorticity_rk_time(0, reps=REPS),
            "stage_with_vmax": lambda s: s.vorticity_rk_time(1, reps=REPS),
            "step_with_copy": lambda s: s.vorticity_time(0, reps=REPS),
            "step_with_vmax": lambda s: s.vorticity_time(1, reps=REPS)}
    ms = {k: [] for k in runs}
    nbytes = {}
    with pg.Solver(a.n) as s:
        s.set_problem()
        s.vcycle(1)
        for rnd in range(a.rounds + 1):
            for k, fn in runs.items():
                t, b = fn(s)
                nbytes[k] = b
                if rnd:
                    ms[k].append(t)
    out = {"n": a.n, "rounds": a.rounds, "reps": REPS}
    for k in runs:
        med = statistics.median(ms[k])
        out[k] = {"ms": spread(ms[k]), "bytes": nbytes[k],
                  "bytes_per_point": round(nbytes[k] / (a.n * a.n), 3),
                  "fraction_of_peak": round(nbytes[k] / (med * 1e-3) / PEAK, 4)}
    return out


def step_call(a):
    import numpy as np
    import _pkgload
    pg = _pkgload.load()
    n, nu = a.n, 0.01
    h = 1.0 / (n - 1)
    dt = 0.8 * h * h / (4.0 * nu)
    out = {"n": n, "rounds": a.rounds, "dt": dt, "nu": nu}
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        s.vorticity_step(dt, nu, WALLS, nsteps=20, **RULE)
        psi0, w0 = s.solution(), s.rhs()

        def run(order, nsteps):
            s.set_problem(psi0, w0)
            t = time.perf_counter()
            info = s.vorticity_step(dt, nu, WALLS, nsteps=nsteps, order=order, **RULE)
            return (time.perf_counter() - t) * 1e3, info.cycles, info.step_ms

        sides = (("order3_one_step", 3, 1), ("euler_three_steps", 1, 3))
        ms = {k: [] for k, _, _ in sides}
        dev = {k: [] for k, _, _ in sides}
        cyc = {}
        for rnd in range(a.rounds + 1):
            for k, order, nsteps in sides:
                t, cyc[k], d = run(order, nsteps)
                if rnd:
                    ms[k].append(t)
                    dev[k].append(d)
        for k, _, _ in sides:
            out[k] = {"ms": spread(ms[k]), "passes_and_copies_device_ms": spread(dev[k]),
                      "cycles": cyc[k]}
        out["order3_over_three_euler"] = round(statistics.median(ms["order3_one_step"]) /
                                               statistics.median(ms["euler_three_steps"]), 3)
    return out


def step_cavity(a):
    import numpy as np
    import torch
    import _pkgload
    pg = _pkgload.load()
    n, nu = a.n, 1e-3
    c = (n - 1) // 2
    out = {"n": n, "nu": nu, "T": 100.0, "ghia": {"psi_min": -0.1179, "u_min_centreline": -0.3829}}
    for order, dt_over_h in ((3, 1.0), (1, 1.0), (3, 1.6), (1, 1.6)):
        dt = dt_over_h / (n - 1)
        steps = int(round(100.0 / dt))
        t0 = time.perf_counter()
        with pg.Solver(n, eps=-1.0) as s:
            s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
            done, cycles, worst, reasons, cfl = 0, 0, 0.0, set(), 0.0
            while done < steps:
                k = min(200, steps - done)
                info = s.vorticity_step(dt, nu, WALLS, nsteps=k, order=order, **RULE)
                done += k
                cycles += info.cycles
                worst = max(worst, info.worst_res)
                reasons.add(info.worst_reason)
                cfl = max(cfl, info.cfl)
                if done % 2000 == 0:
                    print(f"cavity {n} order {order} dt {dt_over_h} h: step {done} / {steps}, cfl "
                          f"{info.cfl:.3f}", file=sys.stderr, flush=True)
                if not np.isfinite(info.cfl) or not np.isfinite(info.worst_res):
                    break
            u, _ = s.velocity()
            torch.cuda.synchronize()
            u = u.cpu().numpy()
            psi = s.solution()
        finite = bool(np.isfinite(psi).all())
        j = int(np.argmin(u[:, c])) if finite else -1
        out[f"order{order}_dt_{dt_over_h}h"] = {
            "dt": dt, "steps": steps, "steps_done": done, "finite": finite, "cycles": cycles,
            "cycles_per_step": round(cycles / max(done, 1), 3), "worst_res": worst,
            "worst_reasons": sorted(reasons), "cfl_max": cfl, "diffusion": info.diffusion,
            "psi_min": float(psi.min()) if finite else None,
            "u_min_centreline": float(u[j, c]) if finite else None,
            "y_of_u_min": j / (n - 1) if finite else None,
            "wall_s": round(time.perf_counter() - t0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4097)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--call-sizes", default="1025,4097")
    ap.add_argument("--cavity-sizes", default="129")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vorticity_rk" / "probe.json"))
    ap.add_argument("--step", choices=["pass", "call", "cavity"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    fns = {"pass": step_pass, "call": step_call, "cavity": step_cavity}
    if a.step:
        print(json.dumps(fns[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "peak_bytes_per_s": PEAK}
    ints = lambda t: [int(x) for x in t.split(",") if x]
    steps = [(f"pass_{n}", "pass", n) for n in ints(a.sizes)]
    steps += [(f"call_{n}", "call", n) for n in ints(a.call_sizes)]
    steps += [(f"cavity_{n}", "cavity", n) for n in ints(a.cavity_sizes)]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"step {name} failed ({p.returncode}); stopping\n{p.stdout}", file=sys.stderr)
            return 1
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"{name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
