#!/usr/bin/env python3
"""Measure pgmg_boussinesq_step_rk on one MI355X (DESIGN.md §4j "Runge-Kutta time stepping").
Prints one JSON object and saves it (default profiles/boussinesq_rk/probe.json).

    python scripts/boussinesq_rk_probe.py [--sizes 4097,16385] [--call-sizes 1025,4097]
                                          [--cavity-sizes 129]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N    on the analytic problem after one V-cycle, alternated in one process over --rounds timed
            rounds after one dropped warm round: pgmg_boussinesq_rk_time(0) (the stage with both
            copies back, 88 B per point) and (1) (the stage with vmax, 56 B per point), (2) and (3)
            (the same at the pass's other built depth), beside pgmg_boussinesq_time(0 / 1) (the
            Euler pass: 72 and 40 B per point) and pgmg_vorticity_rk_time(0 / 1) (48 and 32).  Per
            pass: min / median / max of the rounds' ms, the algorithmic bytes and the fraction of
            the 8 TB/s peak at the median.
  fused_N   the fused stage through ops.boussinesq_stage against the by-hand route through the
            public ops -- ops.boussinesq_step into temporaries (40 B per point), then one torch
            kernel per field on the interior views that reads the saved field and the temporary
            and writes the output (torch.lerp: the one-kernel form of a * x0 + b * e for a + b = 1;
            24 B per point each, 88 in all) --, alternated in one process; device ms per pass from
            events around REPS passes.
  call_N    one whole order-3 step of the heated cavity at Ra = 10^3 (started from 20 Euler steps)
            against three Euler steps of the same dt, alternated in one process, each from the
            same state.  Host wall ms, the device ms of the passes and copies, the cycles.
  cavity_N  de Vahl Davis's cavity at Ra = 10^6, Pr = 0.71 from rest and T = 1 - x to T_end = 0.3,
            atol = 1e-6, at most 30 cycles per solve, at order 3 and at order 1, each at the
            largest dt of a descending ladder that stays finite (the ladder is in units of h^2: at
            this Ra and N the diffusion numbers bind before cfl does; dt / h is reported too):
            |psi| at the centre, max |u| on x = 1/2 and max |v| on y = 1/2 (the parabola through
            the three samples at the peak) beside the published 16.32, 64.63, 219.36, the steps,
            the cycles and the wall time; a run that leaves the finite numbers is stopped and
            reported as such.
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
PR = 0.71
WALLS = (0.0, 0.0, 0.0, 0.0)
RULE = dict(rtol=0.0, atol=1e-6, max_cycles=30)
PUBLISHED_1E6 = {"psi_mid": 16.32, "umax": 64.63, "vmax": 219.36}
LADDER = {3: (0.4, 0.3125, 0.25, 0.2), 1: (0.3125, 0.25, 0.2, 0.125)}   # dt / h^2, descending


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def _conduction(n):
    import numpy as np
    x = np.arange(n) / (n - 1)
    T = np.repeat((1.0 - x)[None, :], n, axis=0)
    T[:, 0], T[:, -1] = 1.0, 0.0
    return T


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    runs = {"stage_with_copies": lambda s: s.boussinesq_rk_time(0, reps=REPS),
            "stage_with_vmax": lambda s: s.boussinesq_rk_time(1, reps=REPS),
            "stage_other_depth_with_copies": lambda s: s.boussinesq_rk_time(2, reps=REPS),
            "stage_other_depth_with_vmax": lambda s: s.boussinesq_rk_time(3, reps=REPS),
            "bouss_with_copies": lambda s: s.boussinesq_time(0, reps=REPS),
            "bouss_with_vmax": lambda s: s.boussinesq_time(1, reps=REPS),
            "vort_stage_with_copy": lambda s: s.vorticity_rk_time(0, reps=REPS),
            "vort_stage_with_vmax": lambda s: s.vorticity_rk_time(1, reps=REPS)}
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


def step_fused(a):
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    dt, nu, kappa, buoy, ca, cb = h * h / 8.0, PR, 1.0, (0.0, 710.0), 0.75, 0.25
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n)
    psi, w, T, w0, T0 = (torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
                         for _ in range(5))
    wout, tout, ew, et = (torch.empty_like(psi) for _ in range(4))
    inner = (slice(1, -1), slice(1, -1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def by_hand():
        pg.ops.boussinesq_step(psi, w, T, ew, et, h, dt, nu, kappa, buoy)
        torch.lerp(ew[inner], w0[inner], ca, out=wout[inner])
        torch.lerp(et[inner], T0[inner], ca, out=tout[inner])

    def timed(fn):
        for _ in range(2):
            fn()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    runs = {"fused": lambda: pg.ops.boussinesq_stage(psi, w, T, w0, T0, wout, tout, h, dt, nu, kappa,
                                                     buoy, ca, cb),
            "by_hand": by_hand}
    ms = {k: [] for k in runs}
    for rnd in range(a.rounds + 1):
        for k, fn in runs.items():
            t = timed(fn)
            if rnd:
                ms[k].append(t)
    pg.ops.release()
    return {"n": n, "rounds": a.rounds, "reps": REPS, "fused_ms": spread(ms["fused"]),
            "by_hand_ms": spread(ms["by_hand"]),
            "fused_fraction_of_peak": round(56.0 * n * n / (statistics.median(ms["fused"]) * 1e-3) / PEAK, 4),
            "by_hand_over_fused": round(statistics.median(ms["by_hand"]) / statistics.median(ms["fused"]), 3),
            "byte_models": 88.0 / 56.0}


def step_call(a):
    import numpy as np
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    dt, nu, kappa, buoy = h * h / 8.0, PR, 1.0, (0.0, 710.0)
    out = {"n": n, "rounds": a.rounds, "dt": dt}
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        T = torch.tensor(_conduction(n), dtype=torch.float64, device="cuda:0")
        s.boussinesq_step(T, dt, nu, kappa, buoy, WALLS, nsteps=20, **RULE)
        psi0, w0, T0 = s.solution(), s.rhs(), T.clone()

        def run(order, nsteps):
            s.set_problem(psi0, w0)
            T.copy_(T0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            info = s.boussinesq_step(T, dt, nu, kappa, buoy, WALLS, nsteps=nsteps, order=order, **RULE)
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


def _peak(v):
    import numpy as np
    v = np.abs(v)
    k = int(np.argmax(v))
    if k == 0 or k == len(v) - 1:
        return float(v[k])
    d = v[k - 1] - 2.0 * v[k] + v[k + 1]
    return float(v[k] - (v[k + 1] - v[k - 1]) ** 2 / (8.0 * d))


def _cavity_run(pg, n, ra, order, dt, t_end):
    import numpy as np
    import torch
    h = 1.0 / (n - 1)
    steps = int(round(t_end / dt))
    buoy = (0.0, ra * PR)
    t0 = time.perf_counter()
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        T = torch.tensor(_conduction(n), dtype=torch.float64, device="cuda:0")
        done, cycles, worst, cfl = 0, 0, 0.0, 0.0
        while done < steps:
            k = min(500, steps - done)
            info = s.boussinesq_step(T, dt, PR, 1.0, buoy, WALLS, nsteps=k, order=order, **RULE)
            done += k
            cycles += info.cycles
            if not np.isfinite(info.cfl) or not np.isfinite(info.worst_res):
                break
            worst = max(worst, info.worst_res)
            cfl = max(cfl, info.cfl)
            if done % 5000 == 0:
                print(f"cavity {n} order {order} dt {dt:.3e}: step {done} / {steps}, cfl {info.cfl:.3f}",
                      file=sys.stderr, flush=True)
        psi = s.solution()
    finite = bool(np.isfinite(psi).all()) and done == steps
    r = {"order": order, "dt": dt, "dt_over_h2": dt / (h * h), "dt_over_h": dt / h, "steps": steps,
         "steps_done": done, "finite": finite, "cycles": cycles,
         "cycles_per_step": round(cycles / max(done, 1), 3), "cfl_max": cfl,
         "diffusion": 4.0 * PR * dt / (h * h), "diffusion_t": 4.0 * dt / (h * h),
         "wall_s": round(time.perf_counter() - t0, 2)}
    if finite:
        mid = (n - 1) // 2
        u = np.zeros(n)
        u[1:-1] = (psi[2:, mid] - psi[:-2, mid]) / (2.0 * h)
        v = -(psi[mid, 2:] - psi[mid, :-2]) / (2.0 * h)
        r.update({"worst_res": worst, "psi_mid": float(abs(psi[mid, mid])), "umax": _peak(u),
                  "vmax": _peak(v)})
    return r


def step_cavity(a):
    import _pkgload
    pg = _pkgload.load()
    n, ra, t_end = a.n, 1e6, 0.3
    h = 1.0 / (n - 1)
    out = {"n": n, "ra": ra, "pr": PR, "T_end": t_end, "published": PUBLISHED_1E6}
    for order in (3, 1):
        tried = []
        for c in LADDER[order]:
            r = _cavity_run(pg, n, ra, order, c * h * h, t_end)
            tried.append(r)
            if r["finite"]:
                break
        out[f"order{order}"] = tried
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4097)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--call-sizes", default="1025,4097")
    ap.add_argument("--cavity-sizes", default="129")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "boussinesq_rk" / "probe.json"))
    ap.add_argument("--step", choices=["pass", "fused", "call", "cavity"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    fns = {"pass": step_pass, "fused": step_fused, "call": step_call, "cavity": step_cavity}
    if a.step:
        print(json.dumps(fns[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "peak_bytes_per_s": PEAK}
    ints = lambda t: [int(x) for x in t.split(",") if x]
    steps = [(f"pass_{n}", "pass", n) for n in ints(a.sizes)]
    steps += [(f"fused_{n}", "fused", n) for n in ints(a.sizes)]
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
