"""GPU: pgmg_damp_grid (include/pgmg.h: one damping pass on caller-owned arrays) -- the
level-general launch of the damping pass, which pgmg_fmg_damped runs on every level of its
pyramid -- bitwise against tests/damp_model.py.

The sizes are those at which the kernel takes another shape: 5 (the smallest: one workgroup,
wave 0 holds two column pairs, waves 1 .. 3 none), 9, 65 (two bands, the second holding the
boundary row 64 alone), 129 (three bands), 513 (one full tile of 512 columns), 1025 (two tiles x
17 bands: deferred rows and columns).  h = 2^l / (N - 1), l = 0 and 3: a coarse level carries a
larger h.  x has a random, non-zero boundary; f is oracle.rhs_mt64.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import damp_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 65, 129, 513, 1025]


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _state(N):
    import oracle
    rng = np.random.default_rng(1000 + N)
    x = rng.standard_normal((N, N))          # the boundary too
    f = np.array(oracle.rhs_mt64(N))
    for a in (x, f):
        a.setflags(write=False)
    return x, f


def _edges(a):
    return np.concatenate([a[0, :], a[-1, :], a[:, 0], a[:, -1]])


@pytest.mark.parametrize("N", SIZES)
def test_damp_grid_bitwise(pgmg, N):
    import torch
    x, f = _state(N)
    ft = _t(f)
    for l in (0, 3):
        h = 2.0 ** l / (N - 1)
        with pgmg.Solver(N, h0=h) as s:
            s.set_problem(x, f)
            mon = s.monitor().res_norm
        for omega in (0.5, 1.0):
            what = f"damp_grid N={N} l={l} omega={omega}"
            want, model_norm = damp_model.damp(x, f, h, omega)
            xt = _t(x)
            got_norm = pgmg.ops.damp(xt, ft, h, omega)
            got = xt.cpu().numpy()
            print(f"{what}: norm {got_norm!r} (monitor {mon!r}, oracle {model_norm!r})")
            assert_bitwise(got, want, what)
            assert np.array_equal(bits(_edges(got)), bits(_edges(x))), what + ": boundary written"
            assert got_norm == mon, (what, got_norm, mon)
            # the asynchronous form (no norm): the same array after a sync
            xa = _t(x)
            assert pgmg.ops.damp(xa, ft, h, omega, norm=False) is None
            torch.cuda.synchronize()
            assert_bitwise(xa.cpu().numpy(), want, what + " async")
            # two passes back to back = the model applied twice
            want2, _ = damp_model.damp(want, f, h, omega)
            pgmg.ops.damp(xa, ft, h, omega, norm=False)
            torch.cuda.synchronize()
            assert_bitwise(xa.cpu().numpy(), want2, what + " twice")
    assert pgmg.load().pgmg_ops_release(None) == pgmg.PGMG_OK


def test_damp_grid_errors_touch_nothing(pgmg):
    N = 33
    x, f = _state(N)
    xt, ft = _t(x), _t(f)
    lib = pgmg.load()
    h = 1.0 / (N - 1)
    out = C.c_double(-1.0)
    px, pf = C.c_void_p(xt.data_ptr()), C.c_void_p(ft.data_ptr())
    for bad_n in (-1, 0, 3, 4, 6, 7, 32, 34, 100):
        assert lib.pgmg_damp_grid(px, pf, bad_n, h, 0.5, C.byref(out), None) == pgmg.PGMG_ERR_ARG, bad_n
    for bad in (0.0, -0.5, 1.5, math.nan, math.inf):
        assert lib.pgmg_damp_grid(px, pf, N, h, bad, C.byref(out), None) == pgmg.PGMG_ERR_ARG, bad
        assert lib.pgmg_damp_grid(px, pf, N, h, bad, None, None) == pgmg.PGMG_ERR_ARG, bad
    for bad_h in (0.0, -1.0, math.nan, math.inf):
        assert lib.pgmg_damp_grid(px, pf, N, bad_h, 0.5, None, None) == pgmg.PGMG_ERR_ARG, bad_h
    assert lib.pgmg_damp_grid(None, pf, N, h, 0.5, None, None) == pgmg.PGMG_ERR_ARG
    assert lib.pgmg_damp_grid(px, None, N, h, 0.5, None, None) == pgmg.PGMG_ERR_ARG
    import torch
    torch.cuda.synchronize()
    assert out.value == -1.0
    assert_bitwise(xt.cpu().numpy(), x, "x after refused calls")
    assert_bitwise(ft.cpu().numpy(), f, "f after refused calls")
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.damp(xt, ft, h, omega=0.0)
