#!/usr/bin/env python3
"""Measure pgmg_boussinesq_step on one MI355X (DESIGN.md §4j "Buoyancy-driven flow").  Prints one
JSON object and saves it (default profiles/boussinesq/probe.json).

    python scripts/boussinesq_probe.py [--sizes 4097,16385] [--call-sizes 1025,4097]
                                       [--cavity-sizes 65,129] [--rayleigh 1e3,1e4,1e5]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N      on the analytic problem after one V-cycle, alternated in one process over --rounds
              timed rounds after one dropped warm round: pgmg_boussinesq_time(0) (the step with both
              copies back, 72 B per point) and (1) (the step with vmax, 40 B per point), beside
              pgmg_vorticity_time(0 / 1) and pgmg_gradient_time (order 2).  Per pass: min / median /
              max of the rounds' ms, the algorithmic bytes and the fraction of the 8 TB/s peak at
              the median.
  fused_N     the fused pass through ops.boussinesq_step against the by-hand route through the
              public ops -- two ops.vorticity_step (w and T), one ops.gradient of T (both
              components), one torch axpy on the interior for the source (88 B per point by
              the ops' own models) --, alternated in one process; device ms per pass from events around REPS
              passes.
  call_N      one whole step of the heated cavity at Ra = 10^3 (started from 20 steps) against the
              by-hand route with its set_problem round trip: ops.wall_vorticity, ops.wall_scalar,
              the by-hand passes above, a download, set_problem(psi, w) and solve(damp=0.5).  Host
              wall ms.
  cavity_R_N  de Vahl Davis's cavity at Ra = R, Pr = 0.71 from rest and T = 1 - x to T_end = 0.5,
              dt = h^2 / 8, atol = 1e-6, at most 30 cycles per step: |psi| at the centre, max |u| on
              x = 1/2 and max |v| on y = 1/2 (grid samples, and the parabola through the three
              samples at the peak), Nu on x = 1/2, the relative change of max |psi| over the last
              tenth, beside the published values.
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
PUBLISHED = {1e3: (1.174, 3.649, 3.697, 1.118), 1e4: (5.071, 16.178, 19.617, None),
             1e5: (9.111, 34.73, 68.59, None)}


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
    runs = {"bouss_with_copies": lambda s: s.boussinesq_time(0, reps=REPS),
            "bouss_with_vmax": lambda s: s.boussinesq_time(1, reps=REPS),
            "vort_with_copy": lambda s: s.vorticity_time(0, reps=REPS),
            "vort_with_vmax": lambda s: s.vorticity_time(1, reps=REPS),
            "gradient_order2": lambda s: s.gradient_time(order=2, reps=REPS)}
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


def _by_hand_pass(pg, psi, w, T, wout, tout, gx, gy, h, dt, nu, kappa, buoy):
    """the step through the public ops: 24 + 24 + 24 B per point, and one torch axpy on the interior
    per non-zero buoyancy component (16 B per point each; one for gravity along -y)"""
    pg.ops.vorticity_step(psi, w, wout, h, dt, nu)
    pg.ops.vorticity_step(psi, T, tout, h, dt, kappa)
    pg.ops.gradient(T, h, gx, gy, order=2)
    inner = (slice(1, -1), slice(1, -1))
    if buoy[1] != 0.0:
        wout[inner].add_(gx[inner], alpha=dt * buoy[1])
    if buoy[0] != 0.0:
        wout[inner].add_(gy[inner], alpha=-dt * buoy[0])


def step_fused(a):
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    dt, nu, kappa, buoy = h * h / 8.0, PR, 1.0, (0.0, 710.0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n)
    psi, w, T = (torch.randn((n, n), dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    wout, tout, gx, gy = (torch.empty_like(psi) for _ in range(4))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(2):
            fn()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    runs = {"fused": lambda: pg.ops.boussinesq_step(psi, w, T, wout, tout, h, dt, nu, kappa, buoy),
            "by_hand": lambda: _by_hand_pass(pg, psi, w, T, wout, tout, gx, gy, h, dt, nu, kappa, buoy)}
    ms = {k: [] for k in runs}
    for rnd in range(a.rounds + 1):
        for k, fn in runs.items():
            t = timed(fn)
            if rnd:
                ms[k].append(t)
    pg.ops.release()
    return {"n": n, "rounds": a.rounds, "reps": REPS, "fused_ms": spread(ms["fused"]),
            "by_hand_ms": spread(ms["by_hand"]),
            "fused_fraction_of_peak": round(40.0 * n * n / (statistics.median(ms["fused"]) * 1e-3) / PEAK, 4),
            "by_hand_over_fused": round(statistics.median(ms["by_hand"]) / statistics.median(ms["fused"]), 3)}


def step_call(a):
    import numpy as np
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    dt, nu, kappa, buoy = h * h / 8.0, PR, 1.0, (0.0, 710.0)
    dev = torch.device("cuda", 0)
    wout, tout, gx, gy = (torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(4))
    out = {"n": n, "rounds": a.rounds, "dt": dt}
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        T = torch.tensor(_conduction(n), dtype=torch.float64, device=dev)
        s.boussinesq_step(T, dt, nu, kappa, buoy, WALLS, nsteps=20, **RULE)
        psi0, w0, T0 = s.solution(), s.rhs(), T.clone()

        def fused():
            s.set_problem(psi0, w0)
            T.copy_(T0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            info = s.boussinesq_step(T, dt, nu, kappa, buoy, WALLS, **RULE)
            return (time.perf_counter() - t) * 1e3, info.cycles

        def by_hand():
            s.set_problem(psi0, w0)
            T.copy_(T0)
            w = torch.tensor(w0, dtype=torch.float64, device=dev)
            psi = torch.tensor(psi0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            pg.ops.wall_vorticity(psi, w, h, WALLS)
            pg.ops.wall_scalar(T, 3)
            _by_hand_pass(pg, psi, w, T, wout, tout, gx, gy, h, dt, nu, kappa, buoy)
            T.copy_(tout)
            s.set_problem(psi0, wout.cpu().numpy())
            info = s.solve(damp=0.5, **RULE)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, info.cycles

        ms = {"boussinesq_step": [], "by_hand": []}
        cyc = {}
        for rnd in range(a.rounds + 1):
            for k, fn in (("boussinesq_step", fused), ("by_hand", by_hand)):
                t, cyc[k] = fn()
                if rnd:
                    ms[k].append(t)
        out.update({"boussinesq_step_ms": spread(ms["boussinesq_step"]),
                    "by_hand_ms": spread(ms["by_hand"]), "cycles": cyc,
                    "by_hand_over_boussinesq_step": round(statistics.median(ms["by_hand"]) /
                                                          statistics.median(ms["boussinesq_step"]), 3)})
    pg.ops.release()
    return out


def _peak(v):
    import numpy as np
    v = np.abs(v)
    k = int(np.argmax(v))
    if k == 0 or k == len(v) - 1:
        return float(v[k])
    d = v[k - 1] - 2.0 * v[k] + v[k + 1]
    return float(v[k] - (v[k + 1] - v[k - 1]) ** 2 / (8.0 * d))


def step_cavity(a):
    import numpy as np
    import torch
    import _pkgload
    pg = _pkgload.load()
    n, ra = a.n, a.ra
    h = 1.0 / (n - 1)
    dt = h * h / 8.0
    steps = int(round(0.5 / dt))
    buoy = (0.0, ra * PR)
    t0 = time.perf_counter()
    with pg.Solver(n, eps=-1.0) as s:
        s.set_problem(np.zeros((n, n)), np.zeros((n, n)))
        T = torch.tensor(_conduction(n), dtype=torch.float64, device="cuda:0")
        done, cycles, worst, reasons, before, cfl = 0, 0, 0.0, set(), None, 0.0
        last_tenth = steps - steps // 10
        while done < steps:
            k = min(2048, steps - done, last_tenth - done if done < last_tenth else steps)
            info = s.boussinesq_step(T, dt, PR, 1.0, buoy, WALLS, nsteps=k, **RULE)
            done += k
            cycles += info.cycles
            worst = max(worst, info.worst_res)
            cfl = max(cfl, info.cfl)
            reasons.add(info.worst_reason)
            if done == last_tenth:
                before = float(np.max(np.abs(s.solution())))
            print(f"cavity Ra={ra:g} N={n}: step {done} / {steps}, cfl {info.cfl:.3f}", file=sys.stderr,
                  flush=True)
        psi = s.solution()
        T = T.cpu().numpy()
    mid = (n - 1) // 2
    u = np.zeros(n)
    u[1:-1] = (psi[2:, mid] - psi[:-2, mid]) / (2.0 * h)
    v = -(psi[mid, 2:] - psi[mid, :-2]) / (2.0 * h)
    q = u * T[:, mid] - (T[:, mid + 1] - T[:, mid - 1]) / (2.0 * h)
    pub = PUBLISHED.get(ra)
    return {"n": n, "ra": ra, "dt": dt, "steps": steps, "cycles": cycles,
            "cycles_per_step": round(cycles / steps, 3), "worst_res": worst,
            "worst_reasons": sorted(reasons), "cfl_max": cfl, "diffusion": info.diffusion,
            "diffusion_t": info.diffusion_t, "psi_mid": float(abs(psi[mid, mid])),
            "umax_samples": float(np.max(np.abs(u))), "umax": _peak(u),
            "vmax_samples": float(np.max(np.abs(v))), "vmax": _peak(v),
            "nu_mid": float(h * (q.sum() - 0.5 * (q[0] + q[-1]))),
            "last_tenth_change": abs(float(np.max(np.abs(psi))) - before) / before,
            "wall_s": round(time.perf_counter() - t0, 2),
            "published": dict(zip(("psi_mid", "umax", "vmax", "nu_mid"), pub)) if pub else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4097)
    ap.add_argument("--ra", type=float, default=1e3)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--call-sizes", default="1025,4097")
    ap.add_argument("--cavity-sizes", default="65,129")
    ap.add_argument("--rayleigh", default="1e3,1e4,1e5")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "boussinesq" / "probe.json"))
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
    steps = [(f"pass_{n}", "pass", n, 0.0) for n in ints(a.sizes)]
    steps += [(f"fused_{n}", "fused", n, 0.0) for n in ints(a.sizes)]
    steps += [(f"call_{n}", "call", n, 0.0) for n in ints(a.call_sizes)]
    steps += [(f"cavity_{ra:g}_{n}", "cavity", n, ra) for ra in (float(x) for x in a.rayleigh.split(",") if x)
              for n in ints(a.cavity_sizes)]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n, ra in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--ra", str(ra), "--rounds", str(a.rounds)]
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
