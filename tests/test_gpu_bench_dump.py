"""GPU: a plain `bench.py --dump-outputs DIR` run writes what its timed call computed.

One small run (N = 257, 1 warmup + 3 timed V-cycles, no --full): the line carries the headline
fields with `full` false and none of the study's legs, and DIR/phi.npy is, bit for bit, the
oracle's phi after 1 + 3 V-cycles from phi0 = 0 (EXACT, like tests/test_gpu_parity.py), with
the oracle's sweep count in DIR/stats.npy.
"""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bitwise

pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_the_timed_result(oracle_mod, tmp_path):
    N, warm, steps = 257, 1, 3
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--n", str(N),
                        "--steps", str(steps), "--warmup", str(warm),
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == steps and d["repetitions"]["count"] == 1
    assert d["unit"] == "V-cycles/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1) < 1e-3
    assert d["roofline"] is None and d["parity"] is None and d["cpu_baseline"] is None
    for leg in ("other_configs", "dropin", "ops", "fast_mode", "general_rhs", "levels"):
        assert leg not in d, leg
    ref, o = oracle_mod.run_cycles("V", N, warm + steps)
    got = np.load(tmp_path / "out" / "phi.npy")
    assert got.dtype == np.float64
    assert_bitwise(got.reshape(N, N), ref, "bench.py --dump-outputs phi")
    assert np.load(tmp_path / "out" / "stats.npy")[0] == o.sweeps
