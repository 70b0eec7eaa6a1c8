#!/usr/bin/env python3
"""Measure pgmg_vorticity_step on one MI355X (DESIGN.md §4h "Vorticity transport").  Prints one
JSON object and saves it (default profiles/vorticity/probe.json).

    python scripts/vorticity_probe.py [--sizes 4097,16385] [--call-sizes 1025,4097]
                                      [--cavity-sizes 65,129]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N    on the analytic problem after one V-cycle, alternated in one process over --rounds timed
            rounds after one dropped warm round: pgmg_vorticity_time(0) (the step with its copy
            back, 40 B per point) and (1) (the step with vmax, 24 B per point), beside
            pgmg_gradient_time (order 2) and pgmg_monitor_time.  Per pass: min / median / max of the
            rounds' ms, the algorithmic bytes and the fraction of the 8 TB/s peak at the median.
  call_N    one whole step of the lid cavity (started from 20 steps) against the by-hand route
            through the public entries, alternated in one process: ops.wall_vorticity, Solver.gradient
            and ops.gradient into temporaries, ops.residual for the Laplacian, torch elementwise
            passes, a download, set_problem(psi, omega) and solve(damp=0.5).  Host wall ms.
  cavity_N  the lid-driven cavity at Re = 100 from rest to T = 40: u at the centre, the minimum of u
            on the vertical centreline and its y, the minimum of psi, beside Ghia et al.'s
            (-0.2058, -0.2109 at 0.4531, -0.1034).  dt = 0.8 h^2 / (4 nu) (diffusion 0.8), atol =
            1e-6, at most 30 cycles per step.
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
NU = 0.01
WALLS = (0.0, 1.0, 0.0, 0.0)
RULE = dict(rtol=0.0, atol=1e-6, max_cycles=30)


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def _dt(n):
    h = 1.0 / (n - 1)
    return 0.8 * h * h / (4.0 * NU)


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    runs = {"step_with_copy": lambda s: s.vorticity_time(0, reps=REPS),
            "step_with_vmax": lambda s: s.vorticity_time(1, reps=REPS),
            "gradient_order2": lambda s: s.gradient_time(order=2, reps=REPS),
            "monitor": lambda s: s.monitor_time(reps=REPS)}
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
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    dt = _dt(n)
    dev = torch.device("cuda", 0)
    zero = torch.zeros((n, n), dtype=torch.float64, device=dev)
    lap, wx, wy = torch.empty_like(zero), torch.empty_like(zero), torch.empty_like(zero)
    out = {"n": n, "rounds": a.rounds, "dt": dt}
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        s.vorticity_step(dt, NU, WALLS, nsteps=20, **RULE)
        psi0, w0 = s.solution(), s.rhs()

        def fused():
            s.set_problem(psi0, w0)
            t = time.perf_counter()
            info = s.vorticity_step(dt, NU, WALLS, **RULE)
            return (time.perf_counter() - t) * 1e3, info.cycles

        def by_hand():
            s.set_problem(psi0, w0)
            w = torch.tensor(w0, dtype=torch.float64, device=dev)
            psi = torch.tensor(psi0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            pg.ops.wall_vorticity(psi, w, h, WALLS)
            px, py = s.gradient(order=2)
            pg.ops.gradient(w, h, wx, wy, order=2)
            pg.ops.residual(lap, w, zero, h)           # 0 - (-lap_h w) on the interior
            adv = py * wx - px * wy
            new = w + dt * (NU * lap - adv)
            new[0, :], new[-1, :], new[:, 0], new[:, -1] = w[0, :], w[-1, :], w[:, 0], w[:, -1]
            s.set_problem(s.solution(), new.cpu().numpy())
            info = s.solve(damp=0.5, **RULE)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, info.cycles

        ms = {"vorticity_step": [], "by_hand": []}
        cyc = {}
        for rnd in range(a.rounds + 1):
            for k, fn in (("vorticity_step", fused), ("by_hand", by_hand)):
                t, cyc[k] = fn()
                if rnd:
                    ms[k].append(t)
        out.update({"vorticity_step_ms": spread(ms["vorticity_step"]),
                    "by_hand_ms": spread(ms["by_hand"]), "cycles": cyc,
                    "by_hand_over_vorticity_step": round(statistics.median(ms["by_hand"]) /
                                                         statistics.median(ms["vorticity_step"]), 3)})
    pg.ops.release()
    return out


def step_cavity(a):
    import numpy as np
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    dt = _dt(n)
    steps = int(round(40.0 / dt))
    t0 = time.perf_counter()
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        done, cycles, worst, reasons = 0, 0, 0.0, set()
        while done < steps:
            k = min(1000, steps - done)
            info = s.vorticity_step(dt, NU, WALLS, nsteps=k, **RULE)
            done += k
            cycles += info.cycles
            worst = max(worst, info.worst_res)
            reasons.add(info.worst_reason)
            print(f"cavity {n}: step {done} / {steps}, cfl {info.cfl:.3f}", file=sys.stderr, flush=True)
        u, _ = s.velocity()
        torch.cuda.synchronize()
        u = u.cpu().numpy()
        psi = s.solution()
    c = (n - 1) // 2
    j = int(np.argmin(u[:, c]))
    return {"n": n, "dt": dt, "steps": steps, "T": steps * dt, "cycles": cycles,
            "cycles_per_step": round(cycles / steps, 3), "worst_res": worst,
            "worst_reasons": sorted(reasons), "cfl": info.cfl, "diffusion": info.diffusion,
            "u_centre": float(u[c, c]), "u_min_centreline": float(u[j, c]), "y_of_u_min": j / (n - 1),
            "psi_min": float(psi.min()), "wall_s": round(time.perf_counter() - t0, 2),
            "ghia": {"u_centre": -0.2058, "u_min_centreline": -0.2109, "y_of_u_min": 0.4531,
                     "psi_min": -0.1034}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4097)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--call-sizes", default="1025,4097")
    ap.add_argument("--cavity-sizes", default="65,129")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vorticity" / "probe.json"))
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
