#!/usr/bin/env python3
"""One named scenario through each branch of the fused level and the cross-cycle loop
(csrc/pgmg_cycle.hip), for comparing two builds of the library launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 scripts/cycle_paths.py run NAME
    python3 scripts/cycle_paths.py parse DIR      # the launch sequence of the trace under DIR
    python3 scripts/cycle_paths.py list

run NAME prints the solution hash and the statistics after every call; PGMG_LIB picks the
build.  parse prints one line per launch (kernel, grid, workgroup, LDS bytes) in dispatch
order per host thread (the ranks of a loopback scenario are threads, whose launches interleave
differently from run to run), the threads ordered by their sequence's checksum; the last line
is "launches N sha256 H" over all of it.  Two builds that launch the same kernels the same way
print equal text for both commands.  Every grid is cross-fused (cross_min_n = 9)."""
import csv
import ctypes
import hashlib
import os
import pathlib
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(s, tag):
    print(tag, s.solution_hash(), s.stats_detail(), "carry", s.carry_info(), "spec", s.dist_info(),
          flush=True)


def _v_calls(pg, tag, calls=(1, 1, 4, 1), N=1025, **cfg):
    with pg.Solver(N, **cfg) as s:
        s.set_problem()
        for i, k in enumerate(calls):
            s.vcycle(k)
            _report(s, f"{tag} call {i} ({k})")


def _rare(pg):
    # test_cross_rare_paths_fire_and_match_oracle's problem and sweep, coarser in eps and from
    # higher up (the residual norms grow with N)
    import numpy as np
    rng = np.random.default_rng(3)
    N = 1025
    phi0 = rng.uniform(-1, 1, (N, N))
    f = rng.uniform(-1, 1, (N, N)) * 1e-3
    for a in (phi0, f):
        a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = 0.0
    for k in range(26, -5, -1):
        eps = 10 ** (k / 2.0)
        with pg.Solver(N, eps=eps) as s:
            s.set_problem(phi0, f)
            s.vcycle(6)
            _report(s, f"rare eps=1e{k / 2.0}")


def _w(pg):
    with pg.Solver(513) as s:
        s.set_problem()
        for i in range(3):   # (a call's visits are planned from the call before)
            s.wcycle(3)
            _report(s, f"W call {i}")
            print("visit modes", s.spec_visit_modes(), flush=True)


def _f(pg, **cfg):
    with pg.Solver(1025, **cfg) as s:
        s.set_problem()
        s.fcycle(3)
        _report(s, "F3")


def _device(pg, staged):
    N = 1025
    hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    raw = ctypes.c_void_p()
    with pg.Solver(N) as s:
        if staged:   # a device pointer the library did not allocate
            assert hip.hipMalloc(ctypes.byref(raw), ctypes.c_size_t(N * N * 8)) == 0
            assert hip.hipMemset(raw, 0, ctypes.c_size_t(N * N * 8)) == 0
            assert hip.hipDeviceSynchronize() == 0
            phi = raw.value
        else:
            import numpy as np
            phi = pg.DeviceGrid(N, np.zeros((N, N)))
        s.set_problem_device(phi)
        print("bound, in place", s.device_info(), flush=True)
        for k in (1, 3):
            s.vcycle(k)
            _report(s, f"device call ({k})")
    if staged:
        hip.hipFree(raw)
    else:
        phi.close()


def _strips(pg, world, **cfg):
    hub = pg.LoopbackHub(world)
    out, err = [None] * world, [None] * world

    def work(r):
        try:
            with pg.Solver(1025, hub=hub, rank=r, gather_n=65, **cfg) as s:
                s.set_problem()
                s.vcycle(4)
                out[r] = (s.solution_hash(root=-1), s.stats_detail(), s.dist_info())
        except Exception as e:
            err[r] = e

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    hub.close()
    for e in err:
        if e is not None:
            raise e
    for r, o in enumerate(out):
        print("rank", r, *o, flush=True)


def _fmg_bc(pg):
    import numpy as np
    N = 1025
    rng = np.random.default_rng(5)
    phi0 = np.zeros((N, N))
    phi0[0, :], phi0[-1, :] = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    phi0[:, 0], phi0[:, -1] = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    f = rng.uniform(-1, 1, (N, N))
    with pg.Solver(N) as s:
        s.set_problem(phi0, f)
        s.fmg(nu=2, damp=0.5, boundary="keep")
        _report(s, "fmg_bc")


def scenarios(pg):
    return {
        "v": lambda: _v_calls(pg, "V"),
        "v_nocarry": lambda: _v_calls(pg, "V no carry", flags=pg.PGMG_FLAG_NO_CARRY),
        "v_exact": lambda: _v_calls(pg, "V exact", flags=pg.PGMG_FLAG_EXACT_DIST),
        "rare": lambda: _rare(pg),
        "ctile": lambda: _v_calls(pg, "V tail 9", tail_n=9),
        "ctile_off": lambda: _v_calls(pg, "V tail 9 no tiles", tail_n=9, flags=pg.PGMG_FLAG_NO_CTILE),
        "w": lambda: _w(pg),
        "f": lambda: _f(pg),
        "f_nopin": lambda: _f(pg, flags=pg.PGMG_FLAG_NO_PIN),
        "device_inplace": lambda: _device(pg, False),
        "device_staged": lambda: _device(pg, True),
        "f32": lambda: _v_calls(pg, "V f32", calls=(3,), dtype="f32"),
        "strips2": lambda: _strips(pg, 2),
        "strips3": lambda: _strips(pg, 3),
        "strips2_exact": lambda: _strips(pg, 2, flags=pg.PGMG_FLAG_EXACT_DIST),
        "fmg_bc": lambda: _fmg_bc(pg),
    }


def parse(d):
    threads = {}
    for p in sorted(pathlib.Path(d).rglob("*kernel_trace.csv")):
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                lds = r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", "?"))
                threads.setdefault(r.get("Thread_Id", "0"), []).append(
                    (int(r["Dispatch_Id"]), " ".join((
                        r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                        r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], lds))))
    seqs = []
    for rows in threads.values():
        text = "\n".join(line for _, line in sorted(rows))
        seqs.append((hashlib.sha256(text.encode()).hexdigest(), text))
    seqs.sort()
    total = hashlib.sha256()
    n = 0
    for k, (h, text) in enumerate(seqs):
        print(f"# thread {k}: {text.count(chr(10)) + 1} launches sha256 {h}")
        print(text)
        total.update(h.encode())
        n += text.count("\n") + 1
    print(f"launches {n} sha256 {total.hexdigest()}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "parse":
        return parse(sys.argv[2])
    sys.path.insert(0, ROOT)
    import _pkgload
    pg = _pkgload.load()
    table = scenarios(pg)
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in table:
        with pg.config_overrides(cross_min_n=9):
            table[sys.argv[2]]()
        print("done", flush=True)
        return
    print("\n".join(table) if sys.argv[1:] == ["list"] else __doc__)


if __name__ == "__main__":
    main()
