#!/usr/bin/env python3
"""Measure pgmg_project on one MI355X (DESIGN.md §4f "Projection").  Prints one JSON object and
saves it (default profiles/project/probe.json).

    python scripts/project_probe.py [--sizes 1025,4097,16385] [--update-sizes 4097,16385]
                                    [--call-sizes 1025,2049,4097] [--error-sizes 257,1025,2049]

Every GPU step is a child process of its own under a time limit; the driver stops at the first
step that fails.
  pass_N    on the analytic problem after one V-cycle, alternated in one process over --rounds timed
            rounds after one dropped warm round: pgmg_project_time(0) (the divergence with its
            output and norm) and (1) (the update of both components) at order 2 and 4, beside
            pgmg_gradient_time (order 4) and pgmg_monitor_time.  Per pass: min / median / max of the
            rounds' ms, the algorithmic bytes and the fraction of the 8 TB/s peak at the median.
  update_N  the update pass against its by-hand equivalent, alternated in one process: (a)
            ops.gradient_add on (u, v), 40 B per point; (b) Solver.gradient into two temporaries
            and two torch add_, 72 B per point.  20 back to back between two events each, order 4.
  call_N    project at both orders on the table's field (p = q = 1) against the by-hand route
            through the public entries with its host round trip of f: ops.divergence, download,
            set_problem(phi, f), solve, Solver.gradient, two add_.  Host wall ms, after one warm
            call of each.
  error_N   err and div_after / div_before of both orders on the table's fields (tests/
            test_proj_cpu.py), eps < 0, nu = 2, omega = 0.5, rtol = 0, atol = max(1e-10,
            0.8 N^2 2^-52) ||f||_2, at most 40 cycles.
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
RULE = dict(rtol=0.0, max_cycles=40)


def spread(v):
    return {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
            "max": round(max(v), 5)}


def step_pass(a):
    import _pkgload
    pg = _pkgload.load()
    runs = {"divergence_order2": lambda s: s.project_time(0, order=2, reps=REPS),
            "divergence_order4": lambda s: s.project_time(0, order=4, reps=REPS),
            "update_order2": lambda s: s.project_time(1, order=2, reps=REPS),
            "update_order4": lambda s: s.project_time(1, order=4, reps=REPS),
            "gradient_order4": lambda s: s.gradient_time(order=4, reps=REPS),
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


def step_update(a):
    import torch
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    with pg.Solver(n) as s:
        s.set_problem()
        s.vcycle(1)
        dev = torch.device("cuda", 0)
        u = torch.zeros((n, n), dtype=torch.float64, device=dev)
        v = torch.zeros_like(u)
        gx, gy = torch.empty_like(u), torch.empty_like(u)
        phi = torch.tensor(s.solution(), dtype=torch.float64, device=dev)
        h = 1.0 / (n - 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def fused():
            pg.ops.gradient_add(phi, h, u, v, order=4, scale=-1.0)

        def by_hand():
            s.gradient(order=4, scale=-1.0, gx=gx, gy=gy)
            u.add_(gx)
            v.add_(gy)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / REPS

        ms = {"fused": [], "by_hand": []}
        for rnd in range(a.rounds + 1):
            for k, fn in (("fused", fused), ("by_hand", by_hand)):
                t = timed(fn)
                if rnd:
                    ms[k].append(t)
        pg.ops.release()
    ratios = [b / f for f, b in zip(ms["fused"], ms["by_hand"])]
    return {"n": n, "rounds": a.rounds, "reps": REPS, "fused_ms": spread(ms["fused"]),
            "by_hand_ms": spread(ms["by_hand"]), "by_hand_over_fused": spread(ratios),
            "fused_bytes_per_point": 40, "by_hand_bytes_per_point": 72,
            "note": "by_hand includes pgmg_gradient's synchronisation per call"}


def _atol(n, f):
    import numpy as np
    return max(1e-10, 0.8 * n * n * 2.0 ** -52) * float(np.linalg.norm(f[1:-1, 1:-1]))


def step_call(a):
    import numpy as np
    import torch
    import _pkgload
    import proj_model
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    us, vs, _, _, phi0 = proj_model.table_fields(1.0, 1.0, n)
    dev = torch.device("cuda", 0)
    ut0, vt0 = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (us, vs))
    out = {"n": n, "rounds": a.rounds}
    with pg.Solver(n, eps=-1.0) as s:
        for order in (2, 4):
            f = pg.ops.divergence(ut0, vt0, h, order=order, scale=-1.0).cpu().numpy()
            atol = _atol(n, f)

            def fused():
                u, v = ut0.clone(), vt0.clone()
                torch.cuda.synchronize()
                t = time.perf_counter()
                info = s.project(u, v, order=order, atol=atol, **RULE)
                return (time.perf_counter() - t) * 1e3, info.solve.fine.cycles

            def by_hand():
                u, v = ut0.clone(), vt0.clone()
                s.set_problem(phi0, None)
                torch.cuda.synchronize()
                t = time.perf_counter()
                fh = pg.ops.divergence(u, v, h, order=order, scale=-1.0).cpu().numpy()
                s.set_problem(s.solution(), fh)
                if order == 4:
                    info = s.solve(order=4, damp=0.5, atol=atol, **RULE)
                else:
                    info = s.solve(damp=0.5, start="fmg", boundary="keep", atol=atol, **RULE)
                gx, gy = s.gradient(order=order, scale=-1.0)
                u.add_(gx)
                v.add_(gy)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * 1e3, info.cycles

            s.set_problem(phi0, None)
            ms = {"project": [], "by_hand": []}
            cyc = {}
            for rnd in range(a.rounds + 1):
                for k, fn in (("project", fused), ("by_hand", by_hand)):
                    t, cyc[k] = fn()
                    if rnd:
                        ms[k].append(t)
            out[f"order{order}"] = {"project_ms": spread(ms["project"]),
                                    "by_hand_ms": spread(ms["by_hand"]), "cycles": cyc,
                                    "by_hand_over_project": round(
                                        statistics.median(ms["by_hand"]) /
                                        statistics.median(ms["project"]), 3)}
    pg.ops.release()
    return out


def step_error(a):
    import numpy as np
    import torch
    import _pkgload
    import proj_model
    pg = _pkgload.load()
    n = a.n
    h = 1.0 / (n - 1)
    out = {"n": n}
    dev = torch.device("cuda", 0)
    for p, q in ((1.0, 1.0), (0.5, 1.5)):
        us, vs, wx, wy, phi0 = proj_model.table_fields(p, q, n)
        den = float(np.sqrt(np.sum(wx ** 2 + wy ** 2)))
        for order in (2, 4):
            with pg.Solver(n, eps=-1.0) as s:
                s.set_problem(phi0, None)
                u, v = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (us, vs))
                f = pg.ops.divergence(u, v, h, order=order, scale=-1.0).cpu().numpy()
                info = s.project(u, v, order=order, atol=_atol(n, f), measure_after=True, **RULE)
                torch.cuda.synchronize()
                err = float(np.sqrt(np.sum((u.cpu().numpy() - wx) ** 2 +
                                           (v.cpu().numpy() - wy) ** 2))) / den
                out[f"p{p}_q{q}_order{order}"] = {
                    "err": err, "div_after_over_before": info.div_after / info.div_before,
                    "cycles": info.solve.fine.cycles, "reason": info.solve.fine.reason,
                    "coarse_cycles": info.solve.coarse.cycles, "div_ms": info.div_ms,
                    "update_ms": info.update_ms, "elapsed_ms": info.elapsed_ms}
    pg.ops.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4097)
    ap.add_argument("--sizes", default="1025,4097,16385")
    ap.add_argument("--update-sizes", default="4097,16385")
    ap.add_argument("--call-sizes", default="1025,2049,4097")
    ap.add_argument("--error-sizes", default="257,1025,2049")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "project" / "probe.json"))
    ap.add_argument("--step", choices=["pass", "update", "call", "error"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 timed rounds")
    fns = {"pass": step_pass, "update": step_update, "call": step_call, "error": step_error}
    if a.step:
        print(json.dumps(fns[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "peak_bytes_per_s": PEAK}
    ints = lambda t: [int(x) for x in t.split(",") if x]
    steps = [(f"pass_{n}", "pass", n) for n in ints(a.sizes)]
    steps += [(f"update_{n}", "update", n) for n in ints(a.update_sizes)]
    steps += [(f"call_{n}", "call", n) for n in ints(a.call_sizes)]
    steps += [(f"error_{n}", "error", n) for n in ints(a.error_sizes)]
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, step, n in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--rounds", str(a.rounds)]
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
