"""CPU: the batch entries (include/pgmg.h "Batched small problems") without a GPU: what they refuse
(PGMG_ERR_ARG before any HIP call -- on a machine without a GPU a HIP call would fail with
PGMG_ERR_HIP instead), the ctypes mirrors of their two structs, and the input conditions of the
model for the batches tests/test_gpu_batch.py runs.
"""
import ctypes as C
import math
import subprocess
from importlib import import_module

import pytest

import batch_model
import solve_rule
from conftest import ROOT

DUMMY = C.c_void_p(0x1000)   # never dereferenced: every call here fails before a launch


@pytest.fixture(scope="module")
def capi(pgmg):
    return import_module("pgmg_amd._capi")


def _cfg(pgmg, capi, N=17, **kw):
    cfg = capi.PgmgBatchConfig()
    assert pgmg.load().pgmg_batch_config_default(C.byref(cfg), N) == 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _opts(pgmg, capi, **kw):
    o = capi.PgmgSolveOpts()
    assert pgmg.load().pgmg_solve_opts_default(C.byref(o)) == 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_batch_config_defaults(pgmg, capi):
    cfg = _cfg(pgmg, capi, 33)
    assert (cfg.N, cfg.v1, cfg.v2, cfg.coarse_iter, cfg.n_coarse, cfg.alpha) == (33, 1, 1, 10, 5, 3)
    assert cfg.eps == 1e-7 and cfg.h == 1.0 / 32 and cfg.precision == capi.PGMG_PRECISION_FP64
    assert pgmg.load().pgmg_batch_config_default(None, 33) == capi.PGMG_ERR_ARG


BAD_CFG = [dict(N=3), dict(N=7), dict(N=129), dict(N=64), dict(alpha=0), dict(alpha=16),
           dict(n_coarse=2), dict(coarse_iter=-1), dict(v1=-1), dict(v2=64), dict(h=0.0),
           dict(h=math.inf), dict(h=math.nan), dict(precision=2)]


@pytest.mark.parametrize("bad", BAD_CFG, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_config_rejected_by_every_entry(pgmg, capi, bad):
    lib = pgmg.load()
    cfg = _cfg(pgmg, capi, **bad)
    o = _opts(pgmg, capi)
    ms = C.c_double()
    assert lib.pgmg_batch_cycle(C.byref(cfg), capi.PGMG_CYCLE_V, 1, DUMMY, DUMMY, 4, None, None,
                                None) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_solve(C.byref(cfg), C.byref(o), 0.5, DUMMY, DUMMY, 4, None,
                                None) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), capi.PGMG_CYCLE_V, 1, 4, 1,
                               C.byref(ms)) == capi.PGMG_ERR_ARG
    assert lib.pgmg_last_error()


def test_cycle_arguments_rejected(pgmg, capi):
    lib = pgmg.load()
    cfg = _cfg(pgmg, capi)
    V, W, F = capi.PGMG_CYCLE_V, capi.PGMG_CYCLE_W, capi.PGMG_CYCLE_F

    def call(cfgp=C.byref(cfg), cycle=V, n=1, phi=DUMMY, f=DUMMY, B=4):
        return lib.pgmg_batch_cycle(cfgp, cycle, n, phi, f, B, None, None, None)

    assert call(cfgp=None) == capi.PGMG_ERR_ARG
    assert call(phi=None) == capi.PGMG_ERR_ARG
    assert call(f=None) == capi.PGMG_ERR_ARG
    assert call(B=0) == capi.PGMG_ERR_ARG
    assert call(B=-3) == capi.PGMG_ERR_ARG
    assert call(B=2 ** 31) == capi.PGMG_ERR_ARG
    assert call(cycle=F) == capi.PGMG_ERR_ARG
    assert call(cycle=7) == capi.PGMG_ERR_ARG
    assert call(n=-1) == capi.PGMG_ERR_ARG
    assert call(cycle=W, n=-1) == capi.PGMG_ERR_ARG


def test_solve_arguments_rejected(pgmg, capi):
    lib = pgmg.load()
    cfg = _cfg(pgmg, capi)
    good = _opts(pgmg, capi)

    def call(cfgp=C.byref(cfg), o=good, omega=0.5, phi=DUMMY, f=DUMMY, B=4, out=None):
        return lib.pgmg_batch_solve(cfgp, C.byref(o) if o is not None else None, omega, phi, f, B,
                                    C.byref(out) if out is not None else None, None)

    assert call(cfgp=None) == capi.PGMG_ERR_ARG
    assert call(o=None) == capi.PGMG_ERR_ARG
    assert call(phi=None) == capi.PGMG_ERR_ARG
    assert call(f=None) == capi.PGMG_ERR_ARG
    assert call(B=0) == capi.PGMG_ERR_ARG
    for omega in (-0.1, 1.5, math.nan, math.inf, -math.inf):
        assert call(omega=omega) == capi.PGMG_ERR_ARG, omega
    # pgmg_solve's option rule (tests/test_solve_cpu.py pins it on pgmg_stop.h)
    for bad in (dict(max_cycles=-1), dict(check_every=0), dict(stall_checks=0), dict(rtol=-1.0),
                dict(rtol=math.nan), dict(atol=-1.0), dict(atol=math.inf), dict(stall_ratio=-0.5),
                dict(stall_ratio=math.nan), dict(cycle=9), dict(monitor=8)):
        assert call(o=_opts(pgmg, capi, **bad)) == capi.PGMG_ERR_ARG, bad
    assert call(o=_opts(pgmg, capi, cycle=capi.PGMG_CYCLE_F)) == capi.PGMG_ERR_ARG
    assert call(o=_opts(pgmg, capi, monitor=capi.PGMG_MON_RESIDUAL | capi.PGMG_MON_ERROR)) \
        == capi.PGMG_ERR_ARG
    out = capi.PgmgBatchOut()
    out.history_cap = -1
    assert call(out=out) == capi.PGMG_ERR_ARG


def test_time_arguments_rejected(pgmg, capi):
    lib = pgmg.load()
    cfg = _cfg(pgmg, capi)
    ms = C.c_double()
    V = capi.PGMG_CYCLE_V
    assert lib.pgmg_batch_time(None, V, 1, 4, 1, C.byref(ms)) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), V, 1, 4, 1, None) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), V, 1, 0, 1, C.byref(ms)) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), V, 1, 4, 0, C.byref(ms)) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), V, -1, 4, 1, C.byref(ms)) == capi.PGMG_ERR_ARG
    assert lib.pgmg_batch_time(C.byref(cfg), capi.PGMG_CYCLE_F, 1, 4, 1,
                               C.byref(ms)) == capi.PGMG_ERR_ARG


def test_valid_call_fails_loudly_without_gpu(pgmg, capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = pgmg.load()
    cfg = _cfg(pgmg, capi)
    o = _opts(pgmg, capi)
    ms = C.c_double()
    assert lib.pgmg_batch_cycle(C.byref(cfg), capi.PGMG_CYCLE_V, 1, DUMMY, DUMMY, 4, None, None,
                                None) == capi.PGMG_ERR_HIP
    assert lib.pgmg_last_error()
    assert lib.pgmg_batch_solve(C.byref(cfg), C.byref(o), 0.5, DUMMY, DUMMY, 4, None,
                                None) == capi.PGMG_ERR_HIP
    rc = lib.pgmg_batch_time(C.byref(cfg), capi.PGMG_CYCLE_V, 1, 4, 1, C.byref(ms))
    assert rc in (capi.PGMG_ERR_HIP, capi.PGMG_ERR_NOMEM)
    with pytest.raises(pgmg.PgmgError):
        pgmg.BatchSolver(17).time(4)


def test_python_wrapper_refuses_other_arrays(pgmg):
    import numpy as np
    import torch
    bs = pgmg.BatchSolver(9)
    with pytest.raises(pgmg.PgmgError):
        bs.cycle(np.zeros((2, 9, 9)), np.zeros((2, 9, 9)))
    with pytest.raises(pgmg.PgmgError):   # host tensors
        bs.cycle(torch.zeros((2, 9, 9), dtype=torch.float64), torch.zeros((2, 9, 9), dtype=torch.float64))
    with pytest.raises(ValueError):
        pgmg.BatchSolver(9, dtype="f16")
    with pytest.raises(TypeError):
        pgmg.BatchSolver(9, tail_n=9)


@pytest.mark.parametrize("cname,pyname", [("pgmg_batch_config", "PgmgBatchConfig"),
                                          ("pgmg_batch_out", "PgmgBatchOut")])
def test_batch_struct_layout(pgmg, capi, tmp_path, cname, pyname):
    """The ctypes mirror agrees with the C struct: size and every field offset."""
    cls = getattr(capi, pyname)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    body = "".join(f'printf("%zu ", offsetof({cname}, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgmg.h"\n'
                   f'int main(void){{printf("%zu ", sizeof({cname}));{body}return 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want


@pytest.mark.parametrize("name", sorted(batch_model.SOLVE_CASES))
def test_model_conditions_of_the_gpu_batches(oracle_mod, name):
    """Every decision of the stop rule on these batches is taken with a relative margin of at
    least 1e-9, far above the 9e-13 by which the device's summation order may move a norm; and a
    batch is mixed: at least three different cycle counts, a stop at check 0, and (in the batches
    whose smoother can reach the target) the cycle cap."""
    c = batch_model.solve_case(name)
    assert solve_rule.norm_tol(65) < 1e-12
    margins = [m.margin for m in c.models]
    print(name, [(m.cycles, solve_rule.REASON[m.reason]) for m in c.models], min(margins))
    assert min(margins) >= 1e-9, margins
    assert len({m.cycles for m in c.models}) >= 3
    assert [m.cycles for m in c.models[-2:]] == [0, 0]
    assert all(m.reason == solve_rule.CONVERGED and m.checks == 1 for m in c.models[-2:])
    assert c.models[-1].norms == [0.0]


def test_model_batches_cover_every_stop_reason(oracle_mod):
    reasons = {n: {m.reason for m in batch_model.solve_case(n).models} for n in batch_model.SOLVE_CASES}
    assert solve_rule.MAX_CYCLES in reasons["damped17"] and solve_rule.MAX_CYCLES in reasons["damped65"]
    assert solve_rule.STALLED in reasons["stall17"] and solve_rule.STALLED in reasons["stall65"]
    for n in ("damped65", "damped17"):
        plain = [m.cycles for m in batch_model.solve_case(n).models[0:8:2]]
        scaled = [m.cycles for m in batch_model.solve_case(n).models[1:8:2]]
        assert all(9 <= k <= 11 for k in plain), plain
        assert max(scaled) < min(plain)
