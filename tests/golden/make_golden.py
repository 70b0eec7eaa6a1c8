#!/usr/bin/env python3
"""Generate the golden fixtures in tests/golden/ from the REFERENCE's own CPU multigrid.

Run in the build container only (needs /root/reference and `make -C oracle ref`):

    python tests/golden/make_golden.py [--big] [--params-only] [--problem-only] [--special-only]

The reference (2_part_MG/MultiGrid.hpp + Smoother.hpp + DynamicGridUtils.hpp) is compiled
unmodified by oracle/Makefile into oracle/_ref/ref_harness; this script only runs it and
stores inputs/outputs as data:

  cycles.json        per-cycle relerr / residual norm / centre value / FNV-64 hash of phi /
                     cumulative sweep and early-exit counts, for V, W and F cycles
  cycles_params.json the same rows for runs with the W-cycle's alpha and the recursion floor
                     N_coarse off the reference's defaults (PARAM_CASES): ref_harness passes
                     alpha to MultigridSolver's constructor (MultiGrid.hpp:22) and sets its
                     public member N_coarse (:19); each case records both.  coarse_iter is
                     the literal 10 in the reference (:61, :100) and cannot be varied here.
                     Provenance: every row is stdout of oracle/_ref/ref_harness, i.e. of the
                     reference's own unmodified MultigridSolver; recorded results, no code.
                     (--params-only regenerates this file alone, in about a second)
  cycles_problem.json the same rows with the problem's constants off the reference's defaults
                     (PROBLEM_CASES): ref_harness assigns the reference's globals a, p, q
                     (globals.cpp:2-4) before anything reads them and, for V and W, hands the
                     case's mesh width h to compute_rhs, compute_exact_solution, v_cycle /
                     w_cycle and compute_residual; each case records a, p, q and h (null:
                     a / (N - 1)).  A relerr that is not finite (p = 0: the exact solution is
                     0 everywhere) is stored as null.  Recorded results of the reference's own
                     unmodified code, as above.  (--problem-only regenerates this file alone)
  special_ops.npz    inputs made of IEEE special values (signed zeros, subnormals, +-1e308, NaN
                     and Inf seeds; SPECIAL_OP_INPUTS) and the reference's residual, restriction,
                     prolongation and smoother outputs on them, N = 17 and 33
  special_cycles.npz the reference's V- and W-cycles on the input families of
                     tests/special_values.py (SPECIAL_CASES): per cycle the cumulative sweep and
                     exit counts, the census of phi (-0, subnormal, Inf, NaN words) and its
                     canonical-NaN hash (special_values.canon_hash); the last cycle's full phi for
                     N = 17 and, V-cycles, N = 33.
                     Recorded inputs and outputs of the reference's own unmodified code
                     (ref_harness modes O and P).  (--special-only regenerates these two alone)
  phi_<K><N>_c<k>.npy  full phi vectors for small N (N <= 129)
  ops_N<N>.npz       seeded random inputs and the reference's residual, restriction,
                     prolongation and smoother outputs (op-level known-answer tests)
"""
import argparse
import json
import math
import os
import pathlib
import subprocess
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
HARNESS = REPO / "oracle" / "_ref" / "ref_harness"

# (kind, N, cycles, eps, dump_phi_at)
CASES = [
    ("V", 33, 30, 1e-7, [1, 3, 30]),
    ("V", 65, 3, 1e-7, [3]),
    ("V", 129, 30, 1e-7, [1, 30]),
    ("V", 257, 3, 1e-7, []),
    ("V", 513, 30, 1e-7, []),
    ("V", 1025, 3, 1e-7, []),
    ("V", 2049, 2, 1e-7, []),
    ("V", 4097, 43, 1e-7, []),    # BASELINE configs[1]: the bench times 3 + 40 cycles
    ("V", 129, 8, 1e3, [8]),     # every smoother exits after its first sweep
    ("V", 257, 5, 1.0, []),      # mixed early exits
    ("V", 65, 4, 0.0, [4]),      # never exits
    ("W", 33, 3, 1e-7, [3]),
    ("W", 129, 3, 1e-7, [3]),
    ("W", 513, 1, 1e-7, []),
    ("F", 33, 3, 1e-7, [3]),
    ("F", 129, 2, 1e-7, [2]),
    ("F", 1025, 1, 1e-7, []),
]
# Off the defaults: (kind, N, cycles, eps, alpha, n_coarse), N <= 257 and at most 4 cycles.
# eps from {1e-7, 1e-2, 1e-4, 1e3, 0.0}: checks that all fire, none, and a mix.
PARAM_CASES = [
    # W-cycles, alpha 1, 2, 4 and 15 (15: the largest the library accepts)
    ("W", 65, 3, 1e-7, 1, 5),
    ("W", 65, 3, 1e-7, 2, 5),
    ("W", 129, 3, 1e-4, 2, 5),
    ("W", 257, 3, 1e-2, 2, 5),
    ("W", 65, 3, 1e-7, 4, 5),
    ("W", 129, 3, 1e-4, 4, 5),
    ("W", 33, 4, 0.0, 4, 5),
    ("W", 257, 2, 1e3, 4, 5),
    ("W", 33, 2, 1e-7, 15, 5),
    ("W", 17, 2, 1e-2, 15, 5),
    # V and W with n_coarse 3, 9, 17 (W also combined with alpha)
    ("V", 65, 4, 1e-7, 3, 3),
    ("V", 257, 3, 1e3, 3, 3),
    ("V", 129, 3, 1e-2, 3, 9),
    ("V", 65, 3, 0.0, 3, 9),
    ("V", 129, 3, 1e-4, 3, 17),
    ("V", 257, 3, 1e-7, 3, 17),
    ("W", 65, 3, 1e-7, 3, 3),
    ("W", 65, 3, 1e-7, 2, 3),
    ("W", 129, 2, 0.0, 3, 3),
    ("W", 129, 3, 1e-4, 3, 9),
    ("W", 129, 3, 1e-4, 4, 9),
    ("W", 65, 3, 1e-2, 3, 17),
    ("W", 129, 3, 1e-7, 4, 17),
    ("W", 257, 2, 1e3, 2, 17),
    # a recursion floor that is no grid size (7, 8: the same cycle as 5; 100 at 257: as 65)
    ("V", 65, 3, 1e-7, 3, 7),
    ("W", 65, 2, 1e-7, 3, 8),
    ("V", 257, 2, 1e-7, 3, 100),
    # the whole tail one coarsest solve; one-level hierarchies larger than 5x5
    ("V", 129, 4, 1e-7, 3, 65),
    ("V", 129, 3, 1e-2, 3, 65),
    ("V", 33, 4, 1e-7, 3, 33),
    ("V", 33, 3, 1e-4, 3, 100),
    ("W", 33, 3, 1e3, 2, 33),
    # F-cycles: the chain starts from an n_coarse x n_coarse grid
    ("F", 65, 3, 1e-7, 3, 3),
    ("F", 33, 3, 1e3, 3, 3),
    ("F", 129, 2, 1e-4, 3, 9),
    ("F", 129, 2, 0.0, 3, 17),
]
# The problem's constants off the defaults: (kind, N, cycles, eps, a, p, q, h), N <= 129 and at
# most 3 cycles.  h None: a / (N - 1); "H1": 0.7 / (N - 1); "H2": 1 / N (V and W only: the
# F-cycle runs its own chain).  The sets P1 .. P10 (p = N - 2 in P8) and a = -2, each with V, W
# and F; sizes and eps from {1e-7, 1e-2, 1e-4} mixed by position.
PROBLEM_SETS = [
    ("P1", 1.0, 2.0, 3.0),        # asymmetric
    ("P2", 2.0, 1.0, 1.0),        # dyadic a != 1
    ("P3", 3.0, 2.0, 1.0),        # non-dyadic a: i * h rounds
    ("P4", 0.5, 3.0, 5.0),        # a < 1, higher modes
    ("P5", 1.0, 0.5, 1.5),        # non-integer: f and u are O(1) on column and row N - 1
    ("P6", 1.0, -1.0, 2.0),       # negative wave number
    ("P7", 1.0, 0.0, 1.0),        # f = 0
    ("P8", 1.0, None, 1.0),       # p = N - 2: the mode one undamped Jacobi sweep annihilates
    ("P9", 1000.0, 2.0, 2.0),     # f ~ 1e-5
    ("P10", 1e-3, 1.0, 1.0),      # f ~ 2e7
    ("neg", -2.0, 1.0, 2.0),      # h < 0, h * h > 0
]


def mesh_width(tag, N):
    return {None: None, "H1": 0.7 / (N - 1), "H2": 1.0 / N}[tag]


def _problem_cases():
    cases, i = [], 0
    for kind in ("V", "W", "F"):
        for _, a, p, q in PROBLEM_SETS:
            N = (33, 65, 129)[i % 3]
            eps = (1e-7, 1e-2, 1e-4)[(i // 3 + i) % 3]
            cases.append((kind, N, 3, eps, a, float(N - 2) if p is None else p, q, None))
            i += 1
    # the exit mixes tests/test_gpu_problem_params.py relies on, at N = 65 (its precision split,
    # V at N = 65 with p = 63, eps 1e-7, is the loop's P8 row for V)
    for kind, eps, a, p, q in (("V", 1e-7, 1.0, 2.0, 3.0), ("V", 1e-7, 0.5, 3.0, 5.0),
                               ("V", 1e-2, 1000.0, 2.0, 2.0)):
        cases.append((kind, 65, 3, eps, a, p, q, None))
    # the caller's mesh width, with the default problem, P1 and P5
    for kind in ("V", "W"):
        for tag in ("H1", "H2"):
            for j, (a, p, q) in enumerate(((1.0, 1.0, 1.0), (1.0, 2.0, 3.0), (1.0, 0.5, 1.5))):
                N = (65, 129, 33)[j]
                eps = (1e-7, 1e-4, 1e-2)[j]
                cases.append((kind, N, 3, eps, a, p, q, tag))
    cases.append(("V", 65, 3, 1e-7, 1.0, 1.0, 1.0, 1.0))     # h = 1: every check fires
    return cases


PROBLEM_CASES = _problem_cases()

# Full-size cases (python make_golden.py --big: ~45 min on one core, <= 60 GB RSS).
# (kind, N, cycles, tool): tool "ref" = the compiled reference (oracle/_ref/ref_harness,
# whose leak reclaimer keeps its RSS at ~9 grids); "port" = oracle/mg_cpu_exec_port, our C
# restatement, pinned bit for bit to the reference up to N = 16385 by the cases above and
# used at N = 32769, where the reference needs more host memory than the build container
# has.  Kind G = FMG start + W-cycles (BASELINE config 5): cycle 1 an F-cycle, then W.
BIG = [("V", 16385, 30, "ref"),     # every cycle count the bench can time (warmup + steps)
       ("F", 16385, 22, "ref"),     # bench.py --cycle F: warmup 2 + steps 20
       ("G", 16385, 2, "ref"),
       ("V", 32769, 6, "port"),     # BASELINE config 4's grid (the bench times 1 + 5 cycles)
       ("G", 32769, 2, "port")]     # BASELINE config 5's grid
PORT = REPO / "oracle" / "mg_cpu_exec_port"


def parse(line):
    t = line.split()
    d = {t[i]: t[i + 1] for i in range(0, len(t) - 1, 2)}
    return {
        "cycle": int(d["cycle"]),
        "relerr": float(d["relerr"]),
        "res": float(d["res"]),
        "center": float(d["center"]),
        "hash": d["hash"],
        "sweeps": int(d["sweeps"]),
        "exits": int(d["exits"]),
    }


def big_case(kind, N, cycles, tool, ingest=None):
    """One BIG case: run the tool (or read its saved stdout, ingest/<kind><N>.txt, produced by
    exactly `<tool> <kind> <N> <cycles> 1e-7`)."""
    exe = HARNESS if tool == "ref" else PORT
    if ingest:
        path = pathlib.Path(ingest) / f"{kind}{N}.txt"
        out = path.read_text() if path.exists() else ""
        if sum(l.startswith("cycle") for l in out.splitlines()) < cycles:
            print(f"skipping {kind} {N}: {path} incomplete")
            return None
    else:
        out = subprocess.run([str(exe), kind, str(N), str(cycles), "1e-7"],
                             check=True, capture_output=True, text=True).stdout
    rows = [parse(l) for l in out.splitlines() if l.startswith("cycle")]
    assert len(rows) == cycles, (kind, N, len(rows))
    src = ("oracle/_ref/ref_harness (the reference's MultigridSolver)" if tool == "ref"
           else "oracle/mg_cpu_exec_port (C restatement)")
    return {"kind": kind, "N": N, "eps": 1e-7, "cycles": rows, "source": src}


def run_case(kind, N, cycles, eps, dumps, tmp):
    rows = []
    # one run for the stats; phi dumps need a run per dump point (harness dumps the last cycle)
    out = subprocess.run([str(HARNESS), kind, str(N), str(cycles), repr(eps)],
                         check=True, capture_output=True, text=True).stdout
    rows = [parse(l) for l in out.splitlines() if l.startswith("cycle")]
    for k in dumps:
        path = os.path.join(tmp, "phi.bin")
        subprocess.run([str(HARNESS), kind, str(N), str(k), repr(eps), path],
                       check=True, capture_output=True)
        phi = np.fromfile(path, dtype="<f8").reshape(N, N)
        tag = "" if eps == 1e-7 else f"_eps{eps:g}"
        np.save(HERE / f"phi_{kind}{N}_c{k}{tag}.npy", phi)
    return {"kind": kind, "N": N, "eps": eps, "cycles": rows}


def run_param_case(kind, N, cycles, eps, alpha, n_coarse):
    assert N <= 257 and cycles <= 4
    out = subprocess.run([str(HARNESS), kind, str(N), str(cycles), repr(eps), "-", str(alpha),
                          str(n_coarse)], check=True, capture_output=True, text=True).stdout
    rows = [parse(l) for l in out.splitlines() if l.startswith("cycle")]
    assert len(rows) == cycles, (kind, N, alpha, n_coarse, len(rows))
    return {"kind": kind, "N": N, "eps": eps, "alpha": alpha, "n_coarse": n_coarse,
            "cycles": rows}


def write_params():
    res = [run_param_case(*c) for c in PARAM_CASES]
    jpath = HERE / "cycles_params.json"
    jpath.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {len(res)} cases to {jpath}")


def run_problem_case(kind, N, cycles, eps, a, p, q, h):
    assert N <= 129 and cycles <= 3 and kind in "VWF"
    hv = mesh_width(h, N) if h is None or isinstance(h, str) else h
    assert hv is None or kind != "F", "the F-cycle runs its own chain of mesh widths"
    out = subprocess.run([str(HARNESS), kind, str(N), str(cycles), repr(eps), "-", "3", "5",
                          repr(a), repr(p), repr(q), "-" if hv is None else repr(hv)],
                         check=True, capture_output=True, text=True).stdout
    rows = [parse(l) for l in out.splitlines() if l.startswith("cycle")]
    assert len(rows) == cycles, (kind, N, a, p, q, h, len(rows))
    for r in rows:
        if not math.isfinite(r["relerr"]):
            r["relerr"] = None
    return {"kind": kind, "N": N, "eps": eps, "a": a, "p": p, "q": q, "h": hv, "cycles": rows}


def write_problem():
    res = [run_problem_case(*c) for c in PROBLEM_CASES]
    jpath = HERE / "cycles_problem.json"
    jpath.write_text(json.dumps(res, indent=1, allow_nan=False) + "\n")
    print(f"wrote {len(res)} cases to {jpath}")


def make_ops(N, seed, tmp):
    rng = np.random.default_rng(seed)
    Nc = (N - 1) // 2 + 1
    h = 1.0 / (N - 1)
    x = rng.uniform(-1.0, 1.0, (N, N))
    f = rng.uniform(-1.0, 1.0, (N, N))
    e = rng.uniform(-1.0, 1.0, (Nc, Nc))
    for a in (x, f, e):   # Dirichlet boundary 0
        a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = 0.0
    eps = 1e-7
    pin = os.path.join(tmp, "in.bin")
    pout = os.path.join(tmp, "out.bin")
    np.concatenate([x.ravel(), f.ravel(), e.ravel()]).astype("<f8").tofile(pin)
    subprocess.run([str(HARNESS), "O", str(N), repr(h), repr(eps), pin, pout], check=True)
    o = np.fromfile(pout, dtype="<f8")
    L, Lc = N * N, Nc * Nc
    parts = np.split(o, np.cumsum([L, Lc, L, L]))
    np.savez(HERE / f"ops_N{N}.npz", N=N, h=h, eps=eps, x=x, f=f, e=e,
             residual=parts[0].reshape(N, N), restrict=parts[1].reshape(Nc, Nc),
             prolong=parts[2].reshape(N, N), smooth1=parts[3].reshape(N, N),
             smooth10=parts[4].reshape(N, N))


# Special values: the cases are special_values.reference_cases(), 2 cycles each.
SPECIAL_CYCLES = 2


def special_op_inputs(N, which):
    """x, f (N x N) and e (Nc x Nc) of one of the three special op inputs."""
    rng = np.random.default_rng(9000 + N + 100 * ("sparse", "big", "seed").index(which))
    Nc = (N - 1) // 2 + 1

    def one(n):
        if which == "sparse":   # +-0, a few point sources and subnormals
            a = np.where(rng.random((n, n)) < 0.5, 0.0, -0.0)
            k = rng.random((n, n))
            a = np.where(k < 0.04, rng.choice([1.0, -2.5, 0.375], (n, n)), a)
            a = np.where((k >= 0.04) & (k < 0.12),
                         rng.choice([5e-324, -5e-324, 3e-310, -1.5e-308, 2.2e-308], (n, n)), a)
            return a
        if which == "big":      # sums of four overflow, differences cancel
            return rng.uniform(-1.0, 1.0, (n, n)) * 1e308
        a = rng.uniform(-1.0, 1.0, (n, n))
        return a
    x, f, e = one(N), one(N), one(Nc)
    if which == "seed":
        x[N // 3, 2 * N // 3] = np.nan
        x[N - 2, 1] = -np.inf
        f[2 * N // 3, N // 3] = np.inf
        e[Nc // 2, Nc // 2] = np.nan
        e[1, Nc - 2] = np.inf
    return x, f, e


def write_special():
    import sys
    sys.path.insert(0, str(REPO / "tests"))
    sys.path.insert(0, str(REPO / "oracle"))
    import special_values as sv
    ops, cyc = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for N in (17, 33):
            Nc, h, eps = (N - 1) // 2 + 1, 1.0 / (N - 1), 1e-7
            for which in ("sparse", "big", "seed"):
                x, f, e = special_op_inputs(N, which)
                np.concatenate([x.ravel(), f.ravel(), e.ravel()]).astype("<f8").tofile(pin)
                subprocess.run([str(HARNESS), "O", str(N), repr(h), repr(eps), pin, pout],
                               check=True)
                o = np.fromfile(pout, dtype="<f8")
                L, Lc = N * N, Nc * Nc
                parts = np.split(o, np.cumsum([L, Lc, L, L]))
                t = f"N{N}_{which}_"
                ops.update({t + "x": x, t + "f": f, t + "e": e,
                            t + "residual": parts[0].reshape(N, N),
                            t + "restrict": parts[1].reshape(Nc, Nc),
                            t + "prolong": parts[2].reshape(N, N),
                            t + "smooth1": parts[3].reshape(N, N),
                            t + "smooth10": parts[4].reshape(N, N)})
        for kind, N, fam, nc, alpha, eps in sv.reference_cases():
            phi0, f = sv.family(fam, N)
            f = sv.analytic_f(N) if f is None else f
            np.concatenate([phi0.ravel(), f.ravel()]).astype("<f8").tofile(pin)
            out = subprocess.run([str(HARNESS), "P", kind, str(N), str(SPECIAL_CYCLES), repr(eps),
                                  str(alpha), str(nc), "-", pin, pout],
                                 check=True, capture_output=True, text=True).stdout
            rows = [l.split() for l in out.splitlines() if l.startswith("cycle")]
            assert len(rows) == SPECIAL_CYCLES, (kind, N, fam, out)
            phi = np.fromfile(pout, dtype="<f8").reshape(SPECIAL_CYCLES, N, N)
            t = f"{kind}_{N}_{fam}_nc{nc}_a{alpha}_eps{eps:g}_"
            cyc[t + "sweeps"] = np.array([int(r[3]) for r in rows], dtype=np.int64)
            cyc[t + "exits"] = np.array([int(r[5]) for r in rows], dtype=np.int64)
            cyc[t + "census"] = np.array([[sv.census(p)[k] for k in ("nz", "sub", "inf", "nan")]
                                          for p in phi], dtype=np.int64)
            cyc[t + "hash"] = np.array([int(sv.canon_hash(p), 16) for p in phi], dtype=np.uint64)
            if N == 17 or (N == 33 and kind == "V"):    # full arrays: the last cycle's phi
                cyc[t + "phi"] = phi[-1]
    np.savez_compressed(HERE / "special_ops.npz", **ops)
    np.savez_compressed(HERE / "special_cycles.npz", **cyc)
    print(f"wrote {len(ops) // 8} op cases and {len(sv.reference_cases())} cycle cases to "
          "special_*.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also run the full-size BIG cases")
    ap.add_argument("--ingest", metavar="DIR",
                    help="with --big: read the BIG cases' stdout from DIR/<kind><N>.txt")
    ap.add_argument("--big-only", action="store_true", help="skip the small cases")
    ap.add_argument("--params-only", action="store_true",
                    help="write cycles_params.json only (PARAM_CASES)")
    ap.add_argument("--problem-only", action="store_true",
                    help="write cycles_problem.json only (PROBLEM_CASES)")
    ap.add_argument("--special-only", action="store_true",
                    help="write special_ops.npz and special_cycles.npz only")
    args = ap.parse_args()
    if not HARNESS.exists():
        raise SystemExit("build the reference harness first: make -C oracle ref")
    if args.special_only:
        write_special()
        return
    if not args.params_only:
        write_problem()
    if args.problem_only:
        return
    write_params()
    if args.params_only:
        return
    prev = []
    jpath = HERE / "cycles.json"
    if jpath.exists():
        prev = json.loads(jpath.read_text())
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        if not args.big_only:
            res = [run_case(*c, tmp) for c in CASES]
            for N, seed in ((17, 1), (33, 12345), (65, 7)):
                make_ops(N, seed, tmp)
    if args.big or args.big_only:
        res += [r for r in (big_case(*c, ingest=args.ingest) for c in BIG) if r is not None]
    keys = {(r["kind"], r["N"], r["eps"]) for r in res}
    res += [r for r in prev if (r["kind"], r["N"], r["eps"]) not in keys]
    res.sort(key=lambda r: (r["kind"], r["N"], r["eps"]))
    jpath.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {len(res)} cases to {jpath}")


if __name__ == "__main__":
    main()
