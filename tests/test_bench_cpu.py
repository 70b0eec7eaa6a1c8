"""CPU: bench.py's launcher (`--gpus N` without a launcher starts N ranks itself; a mismatch
between --gpus and the world size, or too few devices, exits non-zero).  VERDICT r03 #1: the
driver's 8-GPU scaling run must measure what it claims."""
import json
import os
import subprocess
import sys

from conftest import ROOT

BENCH = str(ROOT / "bench.py")
OFF = ["--cpu-baseline", "off", "--pmc", "off", "--trace", "off"]


def _env(**kw):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PGMG_BENCH_SOLO", "PGMG_BENCH_TRANSPORT",
              "PGMG_BENCH_LAUNCH_STUB"):
        e.pop(k, None)
    e.update(kw)
    return e


def test_gpus_n_launches_n_ranks():
    # --n: an abbreviation of the launcher's own options (--nnodes, ...), forwarded as --N
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--n", "4097"] + OFF,
                       capture_output=True, text=True, timeout=300,
                       env=_env(PGMG_BENCH_LAUNCH_STUB="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert sorted(x["stub_rank"] for x in lines) == [0, 1]
    assert all(x["world"] == 2 for x in lines)
    assert sorted(x["local_rank"] for x in lines) == [0, 1]
    assert all(x["n"] == 4097 for x in lines)


def test_gpus_mismatch_with_world_size_fails():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + OFF, capture_output=True,
                       text=True, timeout=120,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_gpus_more_than_devices_fails():
    """No GPU in this container: --gpus 2 without a harness transport exits 2 with a message
    instead of timing one GPU and printing n_gpus: 1."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + OFF, capture_output=True,
                       text=True, timeout=300, env=_env())
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "needs 2 GPUs" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_options_listed():
    """The options the driver's runs and DESIGN.md name exist (a rename would silently fall
    back to argparse's prefix matching or fail only on the GPU box)."""
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True,
                       timeout=120, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--big-grid", "--other-configs", "--cycle",
                "--save-profiles", "--trace", "--pmc", "--cpu-baseline", "--ops", "--full",
                "--dump-outputs"):
        assert opt in r.stdout, opt


def test_plain_run_turns_every_leg_off(monkeypatch):
    """Without --full none of the study's legs runs and one repetition is timed; with it each
    leg follows its own option and five are."""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.reps == 1 and a.steps == 7 and a.dump_outputs == ""
    assert all(getattr(a, leg) == "off" for leg in bench.FULL_LEGS)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--pmc", "off", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.reps == 5 and a.pmc == "off" and a.dump_outputs == "d"
    assert all(getattr(a, leg) == "auto" for leg in bench.FULL_LEGS if leg != "pmc")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--reps", "3"])
    assert bench.parse().reps == 3


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: a small phi whole, a large one as the same seeded sample every time
    (float64, within the size limit), and the sweep counts."""
    import numpy as np
    bench = _bench()

    class S:
        def __init__(self, n):
            self.phi = np.arange(n * n, dtype=np.float64).reshape(n, n)

        def solution(self):
            return self.phi

        def stats(self):
            return 123, 4

    bench.dump_outputs(S(33), tmp_path / "a")
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["phi.npy", "stats.npy"]
    got = np.load(tmp_path / "a" / "phi.npy")
    assert got.dtype == np.float64 and np.array_equal(got, np.arange(33 * 33, dtype=np.float64))
    assert np.load(tmp_path / "a" / "stats.npy").tolist() == [123.0, 4.0]
    n = 2600   # 54 MB of float64: above the limit
    assert n * n * 8 > bench.DUMP_MAX_BYTES
    big = S(n)
    bench.dump_outputs(big, tmp_path / "b")
    bench.dump_outputs(big, tmp_path / "c")
    b, c = np.load(tmp_path / "b" / "phi_sample.npy"), np.load(tmp_path / "c" / "phi_sample.npy")
    assert b.dtype == np.float64 and b.nbytes == bench.DUMP_MAX_BYTES and np.array_equal(b, c)
    # the stub's phi holds its own flat index: sorted indices inside the grid, spread over it
    assert np.all(np.diff(b) >= 0) and b[0] >= 0 and b[-1] < n * n and b[-1] - b[0] > 0.99 * n * n
    assert not (tmp_path / "b" / "phi.npy").exists()


def test_op_cases_build_and_match_kernel_names():
    """bench.py's per-op study table builds (every case callable) and each case's trace-key
    matcher picks the kernels that call launches (bench.kernel_key form: no spaces) -- a stub library on the CPU,
    no GPU."""
    import importlib
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")

    class Ops:
        def __getattr__(self, name):
            return lambda *a, **k: None

    class PG:
        ops = Ops()
        PGMG_PROLONG_SYMMETRIC, PGMG_PROLONG_REFERENCE = 1, 0

    cases, keep = bench.op_cases(PG(), 33, device="cpu")
    assert len(cases) == 8 and len(keep) == 6
    for _, call, nbytes, keys, sweeps, passes in cases:
        call()
        assert nbytes > 0 and callable(keys) and 1 <= passes <= max(1, sweeps)
    names = {
        0: "k_op_sweep_ip<16,true,true>", 1: "k_op_sweep2_ip<8,true,true>",
        2: "k_op_sweep2_ip<8,true,true>", 3: "k_op_sweep<16,true,false,true>",
        4: "k_op_residual<16>", 5: "k_op_restrict<8>", 6: "k_op_prolong<1>", 7: "k_op_prolong<0>",
    }
    for i, k in names.items():
        assert cases[i][3](k), (i, k)
    assert not cases[0][3]("k_op_sweep2_ip<8,true,true>")
    assert not cases[1][3]("k_op_sweep_ip<16,true,true>")
    assert cases[2][3]("k_op_sweep_ip<16,true,true>")
    # the in-place passes' deferred-edge scatter is part of their cost
    for i in (0, 1, 2):
        assert cases[i][3]("k_op_defer_scatter")
    assert not cases[3][3]("k_op_defer_scatter")


def _bench():
    import importlib
    sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_fractions_physical_on_a_stub_line():
    """The roofline rows and the per-op rows bench.py prints, built from stub measurements
    shaped like a real N = 16385 run (the library's pass info, a trace and live PMC of this
    build): every frac* field at or below the copy ceiling (0.79), the paired sweep's rate
    only as sweep_equiv_frac, every traffic_source naming this build; and the checker flags a
    mis-charged kernel and a traffic figure from another build."""
    bench = _bench()
    n = 16383.0 ** 2
    build = "live rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this build; libpgmg.so sha256:0123456789abcdef"
    key = "k_postpre_lds<double,false,true,2>"
    leg = {"passes": [(1, 0, 0.0), (3, 18, 1.02), (4, 1, 1.06), (5, 1, 1.1)],
           "passes_reps": {1: [], 3: [1.03, 1.02, 1.02], 4: [1.06, 1.06, 1.06], 5: [1.1, 1.1, 1.1]},
           "info": {3: ("pgmg::k_postpre_lds<double, false, true, 2>", 16 * n + 16 * n / 4),
                    4: ("pgmg::k_postpre_lds<double, false, true, 130>", 16 * n + 16 * n / 4),
                    5: ("pgmg::k_postpre_lds<double, false, true, 258>", 16 * n + 16 * n / 4)},
           "bytes": {1: 16 * n, 3: 16 * n, 4: 16 * n, 5: 16 * n}, "gen": True}
    pmc = {key: 1.078 * (16 * n + 16 * n / 4)}
    trace = {key: (95, 1.06, 1.036, 19)}
    rows = bench.roofline_rows(leg, pmc, build, trace, "trace")
    assert [r["symbol"] for r in rows] == [key, "k_postpre_lds<double,false,true,258>",
                                           "k_postpre_lds<double,false,true,130>"]
    assert rows[0]["traffic_ratio"] == 1.078 and rows[1]["traffic"] is None
    ops = []
    for name, nbytes, sweeps, passes, ms in (("v=1", 48 * n, 2, 1, 1.38), ("v=100", 2424 * n, 101, 51, 70.6),
                                             ("residual", 24 * n, 0, 1, 1.35)):
        ops.append(bench.op_row(name, nbytes, lambda k: k.startswith("k_op"), sweeps, passes, ms,
                                {"k_op_sweep2_ip<8,true,true,256>": (153, 1.32, None, None)},
                                {"k_op_sweep2_ip<8,true,true,256>": 1.05 * 24 * n}, build))
    assert ops[0]["sweep_equiv_frac"] > 1.0 and ops[0]["frac"] < 0.79
    line = {"roofline": rows[0], "roofline_other": rows[1:], "ops": {"table": ops}}
    assert bench.implausible_fracs(line) == []
    bad = {"roofline": dict(rows[0], frac=0.9158),
           "x": {"traffic_source": "profiles/pmc_fine.json (another build: unrecorded)"}}
    found = bench.implausible_fracs(bad)
    assert len(found) == 2, found


def test_rank_split_summary():
    """--gpus N's per-rank compute / RCCL split: compute = device time
    minus the time inside collective groups, median and max over ranks."""
    bench = _bench()
    allr = [(0.40, 0.05, 11.0), (0.42, 0.09, 11.0), (0.41, 0.02, 11.0), (0.45, 0.10, 11.0)]
    d = bench.rank_split_summary(allr, 0.0085, 20)
    assert d["compute_ms"]["per_rank"] == [0.35, 0.33, 0.39, 0.35]
    assert d["compute_ms"]["max"] == 0.39 and d["rccl_ms"]["max"] == 0.1
    assert d["rccl_ms"]["median"] == 0.07 and d["groups_per_cycle"] == 11.0
    assert d["instrumented_ms_per_step"] == 0.425


def test_levels_table_maps_launch_grids():
    """The levels table tells the coarse levels apart by their launch grid (fused_grid, the
    restated fused_geometry) and charges each pass its algorithmic bytes."""
    bench = _bench()
    g8193, g4097 = bench.fused_grid(8193), bench.fused_grid(4097)
    assert g8193 != g4097
    grid = {"trace": {("k_pre<double,true,false,2>", g8193): [145000, 147000],
                      ("k_post<double,false,2,true>", g8193): [251000],
                      ("k_postpre_lds<double,false,true,2>", 123): [1020000] * 19,
                      ("k_op_residual<16>", 5): [1300000]},
            "pmc": {("k_pre<double,true,false,2>", g8193): {"FETCH_SIZE": [330000.0], "WRITE_SIZE": [33000.0]}}}
    rows = bench.levels_table(16385, grid, {"k_postpre_lds<double,false,true,2>": 5.37e9})
    assert [(r["N"], r["pass"]) for r in rows] == [(16385, "k_postpre_lds"), (8193, "k_post"), (8193, "k_pre")]
    pre = rows[2]
    alg = 8 * 8191.0 ** 2 + 8 * 4095.0 ** 2
    assert pre["us"] == 146.0 and pre["alg_gbps"] == round(alg / 146.0 * 1e-3, 1)
    assert pre["traffic_ratio"] == round((2 * 330000 + 33000) * 1024 / alg, 3)
