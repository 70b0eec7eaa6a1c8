#!/usr/bin/env python3
"""Measure the damping pass and the damped solve on one MI355X (DESIGN.md "Damping pass").
Prints one JSON object and saves it (default profiles/damp/probe.json).

    python scripts/damp_probe.py [--n 16385] [--solve-n 4097] [--reps 20] [--rounds 5] [--out PATH]

fp64.  Every GPU step is a child process of its own under a time limit; the driver stops at the
first step that fails.  Every shape is warmed up before it is timed (the *_time entries run two
warm passes themselves).
  pass    device ms per pgmg_damp pass (all its launches: the pass, the two scatters of its
          deferred edges, the reduction) and per pgmg_monitor pass (two launches), alternated in the same
          process over `rounds` rounds of `reps` back-to-back passes, for the analytic
          (regenerated) f and the stored f; each one's share of the 8 TB/s HBM peak under its byte
          model (the monitor's + 8 B per interior point written); the ratio damp / monitor
          beside the ratio of the byte models.
  solve   oracle.rhs_mt64 at --solve-n, rtol 1e-6, at most 30 V-cycles: wall ms, cycles, stop
          reason and cycles per second of solve(damp=0.5) against solve(), and the residual norm
          of the phi the damped solve leaves against the norm it reported; and the rate of the
          one-cycle chunks at --n (analytic problem, 8 V-cycles with a check each): the plain
          solve's take the carry, the damped solve's cannot.
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
PEAK = 8e12


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    n, reps = a.n, a.reps
    out = {}
    for name, flags in (("analytic_f", 0), ("stored_f", pg.PGMG_FLAG_STORED_RHS)):
        with pg.Solver(n, flags=flags) as s:
            s.set_problem()
            s.vcycle(2)
            s.sync()
            mon, damp = [], []
            for _ in range(a.rounds):
                ms, mb = s.monitor_time(reps)
                mon.append(ms)
                ms, db = s.damp_time(a.omega, reps)
                damp.append(ms)
            mm, dm = statistics.median(mon), statistics.median(damp)
            out[name] = {
                "monitor": {"ms": spread(mon), "bytes": mb,
                            "share_of_peak": round(mb / (mm * 1e-3) / PEAK, 4)},
                "damp": {"ms": spread(damp), "bytes": db,
                         "share_of_peak": round(db / (dm * 1e-3) / PEAK, 4)},
                "ratio_ms": round(dm / mm, 4), "ratio_bytes": round(db / mb, 4)}
    return out


def step_solve(a):
    import _pkgload
    import oracle
    pg = _pkgload.load()
    n = a.solve_n
    f = oracle.rhs_mt64(n)
    out = {"n": n, "rtol": 1e-6, "max_cycles": 30, "omega": a.omega}
    with pg.Solver(n) as s:
        for key, kw in (("plain", {}), ("damped", {"damp": a.omega})):
            wall = []
            for rnd in range(a.rounds + 1):       # round 0 warms the shape up
                s.set_problem(None, f)
                t0 = time.perf_counter()
                info = s.solve(rtol=1e-6, max_cycles=30, **kw)
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    wall.append(ms)
            med = statistics.median(wall)
            out[key] = {"wall_ms": spread(wall), "cycles": info.cycles, "reason": info.reason,
                        "res_over_res0": info.res / info.res0,
                        "cycles_per_s": round(info.cycles / (med * 1e-3), 1)}
            if key == "damped":
                out[key]["res_reported"] = info.res
                out[key]["res_of_phi_left"] = s.monitor().res_norm
    # the rate of the one-cycle chunks at full size: the analytic problem at --n, 8 V-cycles with
    # a check each (a target nothing reaches); plain chunks take the carry, damped ones cannot
    k = 8
    out["rate"] = {"n": a.n, "cycles": k}
    with pg.Solver(a.n) as s:
        for key, kw in (("plain", {}), ("damped", {"damp": a.omega})):
            wall = []
            for rnd in range(a.rounds + 1):
                s.set_problem()
                t0 = time.perf_counter()
                info = s.solve(rtol=1e-30, max_cycles=k, **kw)
                ms = (time.perf_counter() - t0) * 1e3
                assert info.cycles == k, info.cycles
                if rnd:
                    wall.append(ms)
            out["rate"][key] = {"wall_ms": spread(wall), "cycles_per_s":
                                round(k / (statistics.median(wall) * 1e-3), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--solve-n", type=int, default=4097)
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "damp" / "probe.json"))
    ap.add_argument("--step", choices=["pass", "solve"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"pass": step_pass, "solve": step_solve}[a.step](a)))
        return 0
    res = {"n": a.n, "reps": a.reps, "rounds": a.rounds, "dtype": "f64", "peak_bytes_per_s": PEAK}
    for step in ("pass", "solve"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(a.n), "--solve-n", str(a.solve_n), "--omega", str(a.omega),
               "--reps", str(a.reps), "--rounds", str(a.rounds)]
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
