#!/usr/bin/env python3
"""The launch sequence of a fixed call series, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 scripts/launch_sequence.py
    python3 scripts/launch_sequence.py --parse DIR > sequence.txt

Without arguments: a V / carry / W / F / long (converging: the early-exit checks fire) /
in-stream-decision / unfused / fp32 / device-bound call series at N = 513, one result line
(solution hash, statistics) per step; PGMG_LIB picks the build.  --parse DIR: kernel name, grid
and workgroup of every launch of the kernel trace under DIR, in dispatch order.  Two builds
that launch the same kernels the same way give equal files (profiles/fused_split/)."""
import csv
import os
import pathlib
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(d):
    rows = []
    for p in sorted(pathlib.Path(d).rglob("*kernel_trace.csv")):
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"],
                             r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                             r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]))
    rows.sort()
    for r in rows:
        print(*r[1:])


def series():
    sys.path.insert(0, ROOT)
    import numpy as np
    import _pkgload

    pg = _pkgload.load()
    N = 513
    with pg.Solver(N) as s:
        s.set_problem()
        s.vcycle(3)
        s.vcycle(1)
        s.vcycle(1)
        print("carry", s.carry_info(), flush=True)
        print("V", s.solution_hash(), s.stats_detail(), flush=True)
        s.wcycle(2)
        print("W", s.solution_hash(), s.stats_detail(), flush=True)
        s.fcycle(2)
        print("F", s.solution_hash(), s.stats_detail(), flush=True)
        # a long call: the levels converge and the early-exit checks fire (decision kernels,
        # rare paths, fix-ups)
        s.vcycle(40)
        print("V40", s.solution_hash(), s.stats_detail(), flush=True)
    for name, fl in (("exact", pg.PGMG_FLAG_EXACT_DIST),
                     ("exact-noctile", pg.PGMG_FLAG_EXACT_DIST | pg.PGMG_FLAG_NO_CTILE),
                     ("exact-nocross", pg.PGMG_FLAG_EXACT_DIST | pg.PGMG_FLAG_NO_CROSS),
                     ("unfused", pg.PGMG_FLAG_UNFUSED)):
        with pg.Solver(N, flags=fl) as s:
            s.set_problem()
            s.vcycle(30)
            print(name, "V30", s.solution_hash(), s.stats_detail(), flush=True)
            s.fcycle(3)
            print(name, "F3", s.solution_hash(), s.stats_detail(), flush=True)
    with pg.Solver(N, dtype="f32") as s:
        s.set_problem()
        s.vcycle(12)
        print("f32 V12", s.solution_hash(), s.stats_detail(), flush=True)
    with pg.Solver(N) as s, pg.DeviceGrid(N, np.zeros((N, N))) as g:
        s.set_problem_device(g)
        print("bound", s.device_info(), flush=True)
        s.vcycle(2)
        s.vcycle(1)
        print("inplace", s.solution_hash(), s.stats_detail(), flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        series()
