#!/usr/bin/env python3
"""Measure pgmg_fmg_damped on one MI355X (DESIGN.md §4c "Damped FMG").  Prints one JSON object
and saves it (default profiles/fmg_damped/probe.json).

    python scripts/fmg_damped_probe.py [--sizes 4097,16385] [--dtypes f64,f32] [--rounds 5]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.  Every shape is warmed up before it is timed (round 0 is dropped).
  time_N_DTYPE_{analytic,stored}_f
          the analytic problem, f regenerated in the level-0 passes (flags 0) or streamed
          (PGMG_FLAG_STORED_RHS): device ms (hipEvents around the call, pgmg_last_elapsed_ms) of
          fmg(2) and of fmg(2, damp=omega), alternated in the same process, their difference, and
          the device ms of one damping pass at that size (pgmg_damp_time: pass, scatters and a
          reduction the FMG's damps skip) -- the difference should be about 2 x 4/3 of it.
  solve_N_DTYPE
          oracle.rhs_mt64 (a caller's f), target 1e-6 x the residual norm of phi = 0 given as atol:
          ||r|| / ||f|| after fmg(2) and after fmg(2, damp), the damped cycles
          solve(damp, start="fmg") needs after the damped FMG and the wall ms of the whole call
          (FMG + cycles + a check per cycle), against solve(damp) from zero: its cycles and wall ms.
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


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_time(a):
    import _pkgload
    pg = _pkgload.load()
    flags = pg.PGMG_FLAG_STORED_RHS if a.stored else 0
    out = {"n": a.n, "dtype": a.dtype, "stored_f": bool(a.stored), "omega": a.omega}
    with pg.Solver(a.n, dtype=a.dtype, flags=flags) as s:
        plain, damped = [], []
        for rnd in range(a.rounds + 1):
            for ms, kw in ((plain, {}), (damped, {"damp": a.omega})):
                s.set_problem()
                s.fmg(2, **kw)
                s.sync()
                if rnd:
                    ms.append(s.last_elapsed_ms())
        out["fmg_device_ms"] = spread(plain)
        out["fmg_damped_device_ms"] = spread(damped)
        out["difference_ms"] = round(statistics.median(damped) - statistics.median(plain), 5)
        s.set_problem()
        s.vcycle(1)
        ms, nbytes = s.damp_time(a.omega, a.reps)
        out["damp_pass_ms"] = round(ms, 5)
        out["damp_pass_bytes"] = nbytes
        out["difference_in_passes"] = round(out["difference_ms"] / ms, 3)
    return out


def step_solve(a):
    import numpy as np
    import _pkgload
    import oracle
    pg = _pkgload.load()
    n = a.n
    f = oracle.rhs_mt64(n)
    fnorm = float(np.sqrt(np.sum(np.square(f[1:-1, 1:-1], dtype=np.float64))))
    out = {"n": n, "dtype": a.dtype, "omega": a.omega, "rtol_of_zero_residual": 1e-6}
    with pg.Solver(n, dtype=a.dtype) as s:
        s.set_problem(None, f)
        r0 = s.monitor().res_norm
        target = 1e-6 * r0
        out["res_of_zero"] = r0
        out["norm_f_interior"] = fnorm
        for key, kw in (("fmg", {}), ("fmg_damped", {"damp": a.omega})):
            s.set_problem(None, f)
            s.fmg(2, **kw)
            out[f"res_over_f_after_{key}"] = s.monitor().res_norm / fnorm
        for key, kw in (("from_damped_fmg", {"start": "fmg", "nu": 2}), ("from_zero", {})):
            wall = []
            for rnd in range(a.rounds + 1):
                s.set_problem(None, f)
                s.sync()
                t0 = time.perf_counter()
                info = s.solve(rtol=0.0, atol=target, max_cycles=40, damp=a.omega, **kw)
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    wall.append(ms)
            out[key] = {"cycles": info.cycles, "reason": info.reason, "res_over_target": info.res / target,
                        "wall_ms": spread(wall)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stored", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fmg_damped" / "probe.json"))
    ap.add_argument("--step", choices=["time", "solve"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"time": step_time, "solve": step_solve}[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "reps": a.reps, "omega": a.omega}
    steps = []
    for n in (int(x) for x in a.sizes.split(",")):
        for dt in a.dtypes.split(","):
            for stored in (0, 1):
                steps.append((f"time_{n}_{dt}_{'stored' if stored else 'analytic'}_f", "time", n, dt,
                              stored))
            steps.append((f"solve_{n}_{dt}", "solve", n, dt, 1))
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n, dt, stored in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--dtype", dt, "--omega", str(a.omega), "--reps", str(a.reps),
               "--rounds", str(a.rounds), "--stored", str(stored)]
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
