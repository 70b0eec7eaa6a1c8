#!/usr/bin/env python3
"""Measure pgmg_fmg_bc on one MI355X (DESIGN.md §4c "FMG with Dirichlet data").  Prints one JSON
object and saves it (default profiles/fmg_bc/probe.json).

    python scripts/fmg_bc_probe.py [--sizes 4097,16385] [--rounds 7]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.  Every shape is warmed up before it is timed (round 0 is dropped).
  time_N_{analytic,stored}_f
          the analytic problem from phi = 0 (a zero frame: all four entries compute the same two
          results), f regenerated in the level-0 passes (flags 0) or streamed
          (PGMG_FLAG_STORED_RHS): device ms (hipEvents around the call, pgmg_last_elapsed_ms) of
          fmg(2), fmg(2, boundary="keep"), fmg(2, damp) and fmg(2, damp, boundary="keep"), the four
          alternated in the same process; medians over the rounds and the ratios new / old.
  accuracy_N
          p = q = 0.5 (the exact solution is not zero on the far boundary), phi0 = 0 with the exact
          frame: the device monitor's rel_error after fmg(2, boundary="keep"), after
          fmg(2, damp, boundary="keep") and after the zero-boundary fmg(2), each over disc, the
          same monitor after 40 V-cycles from phi0.  Once with the default eps = 1e-7 and once with
          eps = 1e-30 (key suffix _eps0): this problem's residuals are small enough for the
          smoother's early exit to fire on the fine levels of large grids, which moves both the
          FMG iterate and disc; without the exits the ratio is the model's at every size.
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

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
    out = {"n": a.n, "stored_f": bool(a.stored), "omega": a.omega, "rounds": a.rounds}
    kinds = (("fmg", {}), ("fmg_bc", {"boundary": "keep"}), ("fmg_damped", {"damp": a.omega}),
             ("fmg_bc_damped", {"damp": a.omega, "boundary": "keep"}))
    ms = {k: [] for k, _ in kinds}
    with pg.Solver(a.n, flags=flags) as s:
        for rnd in range(a.rounds + 1):
            for key, kw in kinds:
                s.set_problem()
                s.fmg(2, **kw)
                s.sync()
                if rnd:
                    ms[key].append(s.last_elapsed_ms())
    for key, _ in kinds:
        out[f"{key}_device_ms"] = spread(ms[key])
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["ratio_bc_over_fmg"] = round(med["fmg_bc"] / med["fmg"], 5)
    out["ratio_bc_damped_over_fmg_damped"] = round(med["fmg_bc_damped"] / med["fmg_damped"], 5)
    out["added_ms"] = round(med["fmg_bc"] - med["fmg"], 5)
    out["added_damped_ms"] = round(med["fmg_bc_damped"] - med["fmg_damped"], 5)
    return out


def step_accuracy(a):
    import _pkgload
    import oracle
    pg = _pkgload.load()
    n, p, q = a.n, 0.5, 0.5
    phi0 = oracle.Oracle(p=p, q=q).exact(n)
    phi0[1:-1, 1:-1] = 0.0
    out = {"n": n, "p": p, "q": q, "omega": a.omega}
    for sfx, cfg in (("", {}), ("_eps0", {"eps": 1e-30})):
        with pg.Solver(n, p=p, q=q, **cfg) as s:
            s.set_problem(phi0)
            s.vcycle(40)
            disc = s.monitor(error=True).rel_error
            out["disc" + sfx] = disc
            out["disc_early_exits" + sfx] = s.stats()[1]
            for key, kw in (("fmg_bc", {"boundary": "keep"}),
                            ("fmg_bc_damped", {"damp": a.omega, "boundary": "keep"}),
                            ("fmg_zero_frame", {})):
                s.set_problem(phi0)
                s.fmg(2, **kw)
                s.sync()
                rel = s.monitor(error=True).rel_error
                out[f"{key}_rel_error{sfx}"] = rel
                out[f"{key}_over_disc{sfx}"] = rel / disc
                out[f"{key}_early_exits{sfx}"] = s.stats()[1]
                out[f"{key}_device_ms{sfx}"] = round(s.last_elapsed_ms(), 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--stored", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fmg_bc" / "probe.json"))
    ap.add_argument("--step", choices=["time", "accuracy"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    if a.step:
        print(json.dumps({"time": step_time, "accuracy": step_accuracy}[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "omega": a.omega}
    steps = []
    for n in (int(x) for x in a.sizes.split(",")):
        for stored in (0, 1):
            steps.append((f"time_{n}_{'stored' if stored else 'analytic'}_f", "time", n, stored))
        steps.append((f"accuracy_{n}", "accuracy", n, 0))
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n, stored in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--omega", str(a.omega), "--rounds", str(a.rounds),
               "--stored", str(stored)]
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
