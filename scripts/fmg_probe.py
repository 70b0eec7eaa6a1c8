#!/usr/bin/env python3
"""Measure pgmg_fmg on one MI355X.  Prints one JSON object and saves it
(default profiles/fmg/probe.json).

    python scripts/fmg_probe.py [--n 16385] [--sizes 4097,16385] [--reps 20] [--rounds 5]

fp64.  Every GPU step is a child process of its own under a time limit; the driver stops at the
first step that fails.  Every shape is warmed up before it is timed.
  interp    device ms per cubic interpolation pass level 1 -> level 0 at N = --n
            (pgmg_fmg_interp_time: hipEvents around `reps` back-to-back passes) and its share of
            the 8 TB/s HBM peak under its byte model (8 B per fine point written + 8 B per coarse
            point read), alternated over `rounds` rounds with the `pgmg_prolong` op pass (the
            existing pass closest in shape: 16 B per fine interior point + 8 B per coarse one)
            timed the same way in the same process.  The bar: 0.9 x the op pass's share.
  tta_N_*   time to accuracy on the analytic problem, f regenerated (flags 0) or streamed
            (PGMG_FLAG_STORED_RHS): wall and device ms of fmg(2) and its rel_error; the V solve
            from zero's rel_error per cycle, the first cycle count k whose rel_error is at most
            fmg's (none when fmg lands below the error the V solve converges to: then the first
            within 2 x that converged error), and the wall ms of that solve (k cycles, a check
            per cycle) and of pgmg_vcycle(k) in one call; device ms of fmg(2) on contexts of the
            level-1 size and of the tail top's size (the shares of the call spent below level 0 /
            below the tail top).
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


def step_interp(a):
    import torch
    import _pkgload
    pg = _pkgload.load()
    n, reps = a.n, a.reps
    nc = (n - 1) // 2 + 1
    fine = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
    coarse = torch.ones((nc, nc), dtype=torch.float64, device="cuda:0")

    def op_pass():
        for _ in range(2):
            pg.ops.prolong(coarse, fine, mode=pg.PGMG_PROLONG_REFERENCE)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pg.ops.prolong(coarse, fine, mode=pg.PGMG_PROLONG_REFERENCE)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    op_ms, cub_ms, cub_bytes = [], [], 0.0
    with pg.Solver(n) as s:
        s.set_problem()
        s.fmg(2)            # the levels hold a smooth solution, the chain is allocated
        s.sync()
        for _ in range(a.rounds):
            op_ms.append(op_pass())
            ms, cub_bytes = s.fmg_interp_time(reps)
            cub_ms.append(ms)
    opb = 16.0 * (n - 2) ** 2 + 8.0 * (nc - 2) ** 2
    op_share = opb / (statistics.median(op_ms) * 1e-3) / PEAK
    share = cub_bytes / (statistics.median(cub_ms) * 1e-3) / PEAK
    return {"n": n,
            "op_prolong": {"ms": spread(op_ms), "bytes": opb, "share_of_peak": round(op_share, 4)},
            "interp_cubic": {"ms": spread(cub_ms), "bytes": cub_bytes,
                             "share_of_peak": round(share, 4)},
            "share_ratio_to_op": round(share / op_share, 4), "bar": 0.9}


def step_tta(a):
    import _pkgload
    pg = _pkgload.load()
    n = a.n
    flags = pg.PGMG_FLAG_STORED_RHS if a.stored else 0
    out = {"n": n, "stored_f": bool(a.stored)}
    with pg.Solver(n, flags=flags) as s:
        _, tail_top = s.levels()
        # the V solve from zero: rel_error per cycle
        s.set_problem()
        info = s.solve(cycle="V", rtol=1e-30, max_cycles=a.max_cycles, check_every=1, error=True)
        vhist = [rel for _, _, rel in info.history]
        # fmg(2), warm (allocates the chain), then its error
        s.set_problem()
        s.fmg(2)
        s.sync()
        sw0 = s.stats()[0]
        fmg_err = s.monitor(error=True).rel_error
        k = next((c for c, rel in enumerate(vhist) if rel <= fmg_err), None)
        out.update({"fmg_rel_error": fmg_err, "fmg_sweeps": sw0, "v_rel_error_by_cycle": vhist,
                    "v_cycles_to_match": k})
        # the V solve converges to the discretisation error, fmg may land below it: then no
        # cycle count matches, and the comparison is with the first one within 2 x the V
        # solve's converged error
        k2 = next(c for c, rel in enumerate(vhist) if rel <= 2.0 * vhist[-1])
        out.update({"v_converged_rel_error": vhist[-1], "v_cycles_to_2x_converged": k2})
        if k is None:
            out["note"] = (f"the V solve did not reach fmg's error in {a.max_cycles} cycles; timed "
                           "against the cycles to 2 x its converged error")
            k = k2
        out["v_cycles_timed"] = k

        def run_fmg():
            s.fmg(2)
            s.sync()

        def run_solve():
            s.solve(cycle="V", rtol=1e-30, max_cycles=k, check_every=1)

        def run_vk():
            s.vcycle(k)
            s.sync()

        t = {"fmg": [], "v_solve_k": [], "vcycle_k_one_call": []}
        dev = []
        for rnd in range(a.rounds + 1):           # round 0 warms every shape up
            for key, call in (("fmg", run_fmg), ("v_solve_k", run_solve), ("vcycle_k_one_call", run_vk)):
                s.set_problem()
                s.sync()
                t0 = time.perf_counter()
                call()
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    t[key].append(ms)
                    if key == "fmg":
                        dev.append(s.last_elapsed_ms())
        out["wall_ms"] = {key: spread(v) for key, v in t.items()}
        out["fmg_device_ms"] = spread(dev)
    # the part of the call below level 0 / below the tail top: fmg(2) of the smaller contexts
    below = {}
    for name, m in (("below_level0", (n - 1) // 2 + 1), ("below_tail_top", tail_top)):
        with pg.Solver(m, flags=flags) as s:
            ms = []
            for rnd in range(a.rounds + 1):
                s.set_problem()
                s.fmg(2)
                s.sync()
                if rnd:
                    ms.append(s.last_elapsed_ms())
            below[name] = {"n": m, "device_ms": spread(ms),
                           "share_of_fmg": round(statistics.median(ms) / statistics.median(dev), 4)}
    out["parts"] = below
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16385)
    ap.add_argument("--sizes", default="4097,16385")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-cycles", type=int, default=20)
    ap.add_argument("--stored", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fmg" / "probe.json"))
    ap.add_argument("--step", choices=["interp", "tta"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"interp": step_interp, "tta": step_tta}[a.step](a)))
        return 0
    res = {"reps": a.reps, "rounds": a.rounds, "dtype": "f64", "peak_bytes_per_s": PEAK}
    steps = [("interp", "interp", a.n, 0)]
    for n in (int(x) for x in a.sizes.split(",")):
        for stored in (0, 1):
            steps.append((f"tta_{n}_{'stored' if stored else 'analytic'}_f", "tta", n, stored))
    for name, step, n, stored in steps:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--step", step,
               "--n", str(n), "--reps", str(a.reps), "--rounds", str(a.rounds),
               "--max-cycles", str(a.max_cycles), "--stored", str(stored)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"step {name} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}",
                  file=sys.stderr)
            return 1
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
    txt = json.dumps(res, indent=1)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(txt + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
