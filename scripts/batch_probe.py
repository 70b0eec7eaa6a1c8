#!/usr/bin/env python3
"""Measure the batch entries on one MI355X.  Prints one JSON object and saves it
(default profiles/batch/probe.json).

    python scripts/batch_probe.py [--rounds 7] [--reps 50] [--out PATH]

fp64.  Every GPU step is a child process of its own under a time limit; the driver stops at the
first step that fails.
  cycle   pgmg_batch_time for one V-cycle at N = 17, 33, 65 and B = 1, 256, 512, 4096: device us
          per launch (hipEvents around `reps` launches back to back after two warm ones), the
          median of `rounds` rounds with the batch sizes alternated inside each round;
          problems x cycles per second; t(B = 256) / t(B = 1), which is 1 when 256 CUs run 256
          workgroups side by side.
  solve   a mixed batch (oracle.rhs_mt64, 16 seeds, each plain and scaled by 1e-3, atol =
          1e-6 ||f_seed1||, rtol 0, at most 30 V-cycles, omega 1/2) of B = 256 and 4096 problems
          at N = 33 and 65, two routes alternated in one process, host wall time around a device
          synchronisation, medians of `rounds`:
            batch    BatchSolver.solve on the [B, N, N] tensors, one launch;
            by_hand  today's public route: one Solver(N) reused, per problem
                     set_problem_device(phi[b], f[b]) and solve(damp=0.5) with the same options.
          Both routes must give the same cycle counts (checked; reported).
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

NS_CYCLE = (17, 33, 65)
BS_CYCLE = (1, 256, 512, 4096)


def spread(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3),
            "max": round(max(v), 3)}


def step_cycle(a):
    import _pkgload
    pg = _pkgload.load()
    out = {}
    for N in NS_CYCLE:
        bs = pg.BatchSolver(N)
        for B in BS_CYCLE:      # warm every shape up
            bs.time(B, reps=5)
        us = {B: [] for B in BS_CYCLE}
        for _ in range(a.rounds):
            for B in BS_CYCLE:
                us[B].append(bs.time(B, n=1, kind="V", reps=a.reps) * 1e3)
        med = {B: statistics.median(us[B]) for B in BS_CYCLE}
        out[str(N)] = {
            "us_per_launch": {str(B): spread(us[B]) for B in BS_CYCLE},
            "problem_cycles_per_s": {str(B): round(B / (med[B] * 1e-6)) for B in BS_CYCLE},
            "t256_over_t1": round(med[256] / med[1], 3),
            "t512_over_t256": round(med[512] / med[256], 3),
            "t4096_over_t256": round(med[4096] / med[256], 3)}
    return out


def step_solve(a):
    import numpy as np
    import torch
    import _pkgload
    import oracle
    pg = _pkgload.load()
    N, B = a.n, a.b
    seeds = list(range(1, 17))
    fs = []
    for s in seeds:
        f = oracle.rhs_mt64(N, s)
        fs += [f, f * 1e-3]
    atol = 1e-6 * float(np.sqrt((fs[0] ** 2).sum()))
    opts = dict(rtol=0.0, atol=atol, max_cycles=30)
    f = torch.from_numpy(np.stack([fs[b % len(fs)] for b in range(B)])).cuda()
    phi = torch.zeros_like(f)
    bs = pg.BatchSolver(N)
    wall = {"batch": [], "by_hand": []}
    cyc = {}
    with pg.Solver(N) as s:
        for rnd in range(a.rounds + 1):     # round 0 warms both routes up
            phi.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = bs.solve(phi, f, damp=0.5, **opts)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            cyc["batch"] = r.cycles.cpu().numpy().astype(int)
            reasons = r.reason.cpu().numpy()
            phi.zero_()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            hand = []
            for b in range(B):
                s.set_problem_device(phi[b], f[b])
                hand.append(s.solve(damp=0.5, **opts).cycles)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            cyc["by_hand"] = np.array(hand)
            if rnd:
                wall["batch"].append((t1 - t0) * 1e3)
                wall["by_hand"].append((t3 - t2) * 1e3)
    mb, mh = statistics.median(wall["batch"]), statistics.median(wall["by_hand"])
    total = int(cyc["batch"].sum())
    return {"N": N, "B": B, "atol": atol, "max_cycles": 30, "omega": 0.5,
            "cycles_equal": bool((cyc["batch"] == cyc["by_hand"]).all()),
            "cycles_min_max_sum": [int(cyc["batch"].min()), int(cyc["batch"].max()), total],
            "all_converged": bool((reasons == 1).all()),
            "batch_wall_ms": spread(wall["batch"]), "by_hand_wall_ms": spread(wall["by_hand"]),
            "batch_problems_per_s": round(B / (mb * 1e-3)),
            "by_hand_problems_per_s": round(B / (mh * 1e-3)),
            "speedup": round(mh / mb, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "probe.json"))
    ap.add_argument("--step", choices=["cycle", "solve"])
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"cycle": step_cycle, "solve": step_solve}[a.step](a)))
        return 0
    res = {"rounds": a.rounds, "reps": a.reps, "dtype": "f64"}

    def child(step, *extra):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--rounds", str(a.rounds), "--reps", str(a.reps), *extra]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"step {step} {extra} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}",
                  file=sys.stderr)
            return None
        return json.loads(p.stdout.strip().splitlines()[-1])

    res["cycle"] = child("cycle")
    if res["cycle"] is None:
        return 1
    res["solve"] = []
    for N in (33, 65):
        for B in (256, 4096):
            r = child("solve", "--n", str(N), "--b", str(B))
            if r is None:
                return 1
            res["solve"].append(r)
    txt = json.dumps(res, indent=1)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(txt + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
