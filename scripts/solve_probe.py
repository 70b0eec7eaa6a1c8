#!/usr/bin/env python3
"""Measure the convergence monitor and pgmg_solve on one MI355X (DESIGN.md "Convergence
monitor").  Prints one JSON object and saves it (default profiles/solve/probe.json).

    python scripts/solve_probe.py [--n 16385] [--reps 20] [--rounds 5] [--k 4] [--out PATH]

N = 16385, fp64.  Every GPU step is a child process of its own under a time limit; the driver
stops at the first step that fails.  Every shape is warmed up before it is timed.
  monitor   device ms per pgmg_monitor pass (hipEvents around `reps` back-to-back passes,
            pgmg_monitor_time) and its share of the 8 TB/s HBM peak under the byte model
            (8 B per point of phi, + 8 B per interior point of a stored f), for residual /
            analytic f, residual / stored f, residual + error; the `pgmg_residual` op pass
            (24 B per interior point) timed the same way in the same process; and the host wall
            time per synchronous call of pgmg_monitor (residual, stored f) against
            pgmg_residual_norm -- the parent's code, unchanged -- alternated in the same
            process, `rounds` rounds of `reps` calls each, with the spread over the rounds.
  solve     wall ms of a V solve that stops after k cycles (check_every = 1, k + 1 checks)
            against pgmg_vcycle(k) in one call and against k x (pgmg_vcycle(1) +
            pgmg_residual_norm()), today's way of watching convergence.
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
PEAK = 8e12


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_monitor(a):
    import torch
    import _pkgload
    pg = _pkgload.load()
    n, reps = a.n, a.reps
    out = {}
    forms = [("residual_analytic_f", 0, dict()),
             ("residual_stored_f", pg.PGMG_FLAG_STORED_RHS, dict()),
             ("residual_error", 0, dict(error=True))]
    # the op pass on reference-layout arrays, events around `reps` back-to-back calls
    x = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
    f = torch.empty_like(x)
    r = torch.zeros_like(x)
    h = 1.0 / (n - 1)
    pg.ops.rhs(f, h)

    def op_pass():
        pg.ops.residual(r, x, f, h)
        pg.ops.residual(r, x, f, h)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pg.ops.residual(r, x, f, h)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    op_ms = []
    mon_ms = {name: [] for name, _, _ in forms}
    mon_bytes = {}
    solvers = {}
    for name, flags, kw in forms:
        if flags not in solvers:
            s = pg.Solver(n, flags=flags)
            s.set_problem()
            s.vcycle(2)
            s.sync()
            solvers[flags] = s
    for _ in range(a.rounds):            # the op pass and the monitor forms alternate
        op_ms.append(op_pass())
        for name, flags, kw in forms:
            ms, b = solvers[flags].monitor_time(reps, **kw)
            mon_ms[name].append(ms)
            mon_bytes[name] = b
    opb = 24.0 * (n - 2) ** 2
    out["op_residual"] = {"ms": spread(op_ms), "bytes": opb,
                          "share_of_peak": round(opb / (statistics.median(op_ms) * 1e-3) / PEAK, 4)}
    for name, _, _ in forms:
        med = statistics.median(mon_ms[name])
        out["monitor_" + name] = {"ms": spread(mon_ms[name]), "bytes": mon_bytes[name],
                                  "bytes_per_point": round(mon_bytes[name] / (n * n), 3),
                                  "share_of_peak": round(mon_bytes[name] / (med * 1e-3) / PEAK, 4)}
    del x, f, r
    # wall time per synchronous call: the monitor (residual, stored f) against
    # pgmg_residual_norm, alternated
    s = solvers[pg.PGMG_FLAG_STORED_RHS]
    v_mon, v_old = s.monitor().res_norm, s.residual_norm()
    wall = {"monitor": [], "residual_norm": []}
    for _ in range(a.rounds):
        for key, call in (("monitor", s.monitor), ("residual_norm", s.residual_norm)):
            call()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            wall[key].append((time.perf_counter() - t0) * 1e3 / reps)
    out["wall_ms_per_call_stored_f"] = {k: spread(v) for k, v in wall.items()}
    out["values"] = {"monitor": v_mon, "residual_norm": v_old,
                     "rel_diff": abs(v_mon - v_old) / v_old}
    for s in solvers.values():
        s.close()
    return out


def step_solve(a):
    import _pkgload
    pg = _pkgload.load()
    n, k = a.n, a.k
    out = {"k": k}
    t = {"solve": [], "vcycle_k_one_call": [], "k_x_vcycle1_residual_norm": []}
    with pg.Solver(n) as s:
        def solve():
            info = s.solve(cycle="V", rtol=1e-30, max_cycles=k, check_every=1)
            assert info.cycles == k and info.reason == pg.PGMG_STOP_MAX_CYCLES, info.cycles
            return info

        def one_call():
            s.vcycle(k)
            s.sync()

        def today():
            for _ in range(k):
                s.vcycle(1)
                s.residual_norm()

        for rnd in range(a.rounds + 1):       # round 0 warms every shape up
            for key, call in (("solve", solve), ("vcycle_k_one_call", one_call),
                              ("k_x_vcycle1_residual_norm", today)):
                s.set_problem()
                c0 = s.carry_info()
                t0 = time.perf_counter()
                r = call()
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    t[key].append(ms)
                if key == "solve":
                    out["history"] = [[c, res] for c, res, _ in r.history]
                    # (took, made, dropped) of this solve's one-cycle calls
                    out["carry_info"] = [b - a for a, b in zip(c0, s.carry_info())]
    out["wall_ms"] = {key: spread(v) for key, v in t.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "solve" / "probe.json"))
    ap.add_argument("--step", choices=["monitor", "solve"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"monitor": step_monitor, "solve": step_solve}[a.step](a)))
        return 0
    res = {"n": a.n, "reps": a.reps, "rounds": a.rounds, "dtype": "f64", "peak_bytes_per_s": PEAK}
    for step in ("monitor", "solve"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(a.n), "--reps", str(a.reps), "--rounds", str(a.rounds), "--k", str(a.k)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"step {step} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}",
                  file=sys.stderr)
            return 1
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
    txt = json.dumps(res, indent=1)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(txt + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
