"""GPU: pgmg_defect_grid and pgmg_correct_grid (include/pgmg.h: the two passes of
pgmg_solve_mixed on caller-owned arrays) bitwise against tests/mixed_model.py.

The sizes are those at which k_defect takes another shape: 5 (one workgroup, wave 0 holds two
column pairs, waves 1 .. 3 none), 9, 33, 129 (three bands) and 1025 (the first size with two
512-column tiles and several 64-row bands).  x and f are random with a non-zero frame; h =
1 / (N - 1) and 0.7 / (N - 1); scale 1, 2^-20 and 2^30.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import mixed_model
from conftest import assert_bitwise, bits
from special_values import ABI_F32_WORDS, assert_bitwise_nan, census

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 33, 129, 1025]
SCALES = [1.0, 2.0 ** -20, 2.0 ** 30]


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.tensor(a, dtype=torch.float32 if a.dtype == np.float32 else torch.float64,
                        device="cuda:0")


def _junk32(N):
    """an output array that holds no value a pass could leave by accident (a NaN pattern)"""
    import torch
    return torch.full((N, N), float("nan"), dtype=torch.float32, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _state(N):
    rng = np.random.default_rng(2000 + N)
    x = rng.standard_normal((N, N))          # the frame too
    f = rng.standard_normal((N, N)) * (N - 1) ** 2
    e = rng.standard_normal((N, N)).astype(np.float32)
    x[0, N // 2] = -0.0                      # a frame word whose sign a rewrite would lose
    x[N // 2, N - 1] = -0.0
    for a in (x, f, e):
        a.setflags(write=False)
    return x, f, e


def _frame(a):
    return np.concatenate([a[0, :], a[-1, :], a[:, 0], a[:, -1]])


@pytest.mark.parametrize("N", SIZES)
def test_defect_bitwise(pgmg, N):
    import torch
    x, f, _ = _state(N)
    xt, ft = _t(x), _t(f)
    for h in (1.0 / (N - 1), 0.7 / (N - 1)):
        with pgmg.Solver(N, h0=h) as s:
            s.set_problem(x, f)
            mon = s.monitor().res_norm
        for scale in SCALES:
            what = f"defect N={N} h={h!r} scale={scale!r}"
            want, model_norm = mixed_model.defect(x, f, h, scale)
            gt = _junk32(N)
            got_norm = pgmg.ops.defect(xt, ft, h, gt, scale)
            got = gt.cpu().numpy()
            print(f"{what}: norm {got_norm!r} (monitor {mon!r}, oracle {model_norm!r})")
            assert got.dtype == np.float32
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
            assert not _frame(got).view(np.uint32).any(), what + ": the frame is not +0"
            assert got_norm == mon, (what, got_norm, mon)
            assert abs(got_norm - model_norm) <= N * N * 2.0 ** -52 * model_norm, what
            # the asynchronous form (no norm): the same array after a sync
            ga = _junk32(N)
            assert pgmg.ops.defect(xt, ft, h, ga, scale, norm=False) is None
            torch.cuda.synchronize()
            assert np.array_equal(ga.cpu().numpy().view(np.uint32), want.view(np.uint32)), what + " async"
    assert_bitwise(xt.cpu().numpy(), x, "x after the defect passes")
    assert_bitwise(ft.cpu().numpy(), f, "f after the defect passes")
    assert pgmg.load().pgmg_ops_release(None) == pgmg.PGMG_OK


@pytest.mark.parametrize("N", SIZES)
def test_correct_bitwise(pgmg, N):
    import torch
    x, _, e = _state(N)
    et = _t(e)
    for t in (1.0, 2.0 ** 20, 2.0 ** -30):
        what = f"correct N={N} t={t!r}"
        want = mixed_model.correct(x, e, t)
        xt = _t(x)
        pgmg.ops.correct(xt, et, t)
        torch.cuda.synchronize()
        got = xt.cpu().numpy()
        assert_bitwise(got, want, what)
        assert np.array_equal(bits(_frame(got)), bits(_frame(x))), what + ": the frame was written"
        # twice = the model applied twice
        pgmg.ops.correct(xt, et, t)
        torch.cuda.synchronize()
        assert_bitwise(xt.cpu().numpy(), mixed_model.correct(want, e, t), what + " twice")
    assert np.array_equal(et.cpu().numpy().view(np.uint32), e.view(np.uint32)), "e was written"


def _special(N):
    """x, f (float64) and e (float32) that hold +-0, subnormals, +-Inf, NaN and words fp32 cannot
    hold, frame included"""
    w = np.array(ABI_F32_WORDS + (5e-324, -5e-324, 1e300, -1e300, float("inf"), float("-inf")))
    k = np.arange(N * N)
    f = w[k % len(w)].reshape(N, N).copy()
    x = np.zeros((N, N))
    x[N // 3, N // 2] = np.inf
    x[2 * N // 3, N // 4] = np.nan
    x[N // 2, 1:5] = (-0.0, 5e-324, 1e-310, -2.5e-308)
    we = np.array([1e-40, -1e-45, 3e38, -0.0, 0.0, np.inf, -np.inf, np.nan, 0.1, -7.0], dtype=np.float32)
    e = we[k % len(we)].reshape(N, N).copy()
    return x, f, e


def test_defect_special_values(pgmg):
    N = 33
    x, f, _ = _special(N)
    h = 1.0 / (N - 1)
    with pgmg.Solver(N) as s:
        s.set_problem(x, f)
        mon = s.monitor().res_norm
    for scale in (1.0, 2.0 ** 30, 2.0 ** -100):
        want, model_norm = mixed_model.defect(x, f, h, scale)
        c = census(want)
        assert c["nan"] >= 1 and c["inf"] >= 1 and c["nz"] >= 1, c
        if scale == 1.0:
            assert c["sub"] >= 1, c   # (a subnormal fp32 result)
        gt = _junk32(N)
        got_norm = pgmg.ops.defect(_t(x), _t(f), h, gt, scale)
        assert_bitwise_nan(gt.cpu().numpy(), want, f"defect special scale={scale!r}")
        assert math.isnan(model_norm) and math.isnan(got_norm) and math.isnan(mon)
    # finite inputs whose product overflows fp32, with a finite norm
    rng = np.random.default_rng(7)
    ff = rng.standard_normal((N, N)) * 1e30
    ff[5, 5], ff[6, 6], ff[7, 7] = 1e-45, -1e-46, -0.0
    xf = np.zeros((N, N))
    want, model_norm = mixed_model.defect(xf, ff, h, 2.0 ** 30)
    c = census(want)
    assert c["inf"] >= 100 and c["nan"] == 0 and c["nz"] >= 1, c
    gt = _junk32(N)
    got_norm = pgmg.ops.defect(_t(xf), _t(ff), h, gt, 2.0 ** 30)
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert math.isfinite(got_norm) and abs(got_norm - model_norm) <= N * N * 2.0 ** -52 * model_norm


def test_correct_special_values(pgmg):
    import torch
    N = 33
    _, x, e = _special(N)     # (the word table as x: its frame holds every special word too)
    for t in (1.0, 2.0 ** -20, 2.0 ** 100):
        want = mixed_model.correct(x, e, t)
        c = census(want[1:-1, 1:-1])
        assert c["nan"] >= 1 and c["inf"] >= 1 and c["sub"] + c["nz"] >= 1, c
        xt = _t(x)
        pgmg.ops.correct(xt, _t(e), t)
        torch.cuda.synchronize()
        got = xt.cpu().numpy()
        assert_bitwise_nan(got, want, f"correct special t={t!r}")
        assert np.array_equal(bits(_frame(got)), bits(_frame(x))), "the frame's bits (NaN payloads too)"


def test_errors_enqueue_nothing(pgmg):
    import torch
    ARG = pgmg.PGMG_ERR_ARG
    N = 33
    x, f, e = _state(N)
    xt, ft, et, gt = _t(x), _t(f), _t(e), _junk32(N)
    lib = pgmg.load()
    h = 1.0 / (N - 1)
    out = C.c_double(-1.0)
    px, pf, pe, pg = (C.c_void_p(t.data_ptr()) for t in (xt, ft, et, gt))
    host = np.zeros((N, N), dtype=np.float32)
    for bad_n in (-1, 0, 3, 4, 6, 7, 32, 34, 100):
        assert lib.pgmg_defect_grid(px, pf, pg, bad_n, h, 1.0, C.byref(out), None) == ARG, bad_n
        assert lib.pgmg_correct_grid(px, pe, bad_n, 1.0, None) == ARG, bad_n
    for bad_h in (0.0, math.nan, math.inf, -math.inf):
        assert lib.pgmg_defect_grid(px, pf, pg, N, bad_h, 1.0, None, None) == ARG, bad_h
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.pgmg_defect_grid(px, pf, pg, N, h, bad, C.byref(out), None) == ARG, bad
        assert lib.pgmg_correct_grid(px, pe, N, bad, None) == ARG, bad
    assert lib.pgmg_defect_grid(None, pf, pg, N, h, 1.0, None, None) == ARG
    assert lib.pgmg_defect_grid(px, None, pg, N, h, 1.0, None, None) == ARG
    assert lib.pgmg_defect_grid(px, pf, None, N, h, 1.0, None, None) == ARG
    assert lib.pgmg_correct_grid(None, pe, N, 1.0, None) == ARG
    assert lib.pgmg_correct_grid(px, None, N, 1.0, None) == ARG
    # g that is host memory, that is x or f, or that ends inside f; e inside x
    assert lib.pgmg_defect_grid(px, pf, host.ctypes.data_as(C.c_void_p), N, h, 1.0, None, None) == ARG
    assert lib.pgmg_defect_grid(px, pf, px, N, h, 1.0, None, None) == ARG
    assert lib.pgmg_defect_grid(px, pf, pf, N, h, 1.0, None, None) == ARG
    assert lib.pgmg_defect_grid(px, pf, C.c_void_p(ft.data_ptr() + 8 * N * N - 4), N, h, 1.0, None, None) == ARG
    assert lib.pgmg_correct_grid(px, px, N, 1.0, None) == ARG
    assert lib.pgmg_correct_grid(px, C.c_void_p(xt.data_ptr() + 4 * N * N), N, 1.0, None) == ARG
    torch.cuda.synchronize()
    assert out.value == -1.0
    assert_bitwise(xt.cpu().numpy(), x, "x after refused calls")
    assert_bitwise(ft.cpu().numpy(), f, "f after refused calls")
    assert np.isnan(gt.cpu().numpy()).all(), "g after refused calls"
    # a negative h is legal (a < 0 contexts): the same g as h > 0
    want, _ = mixed_model.defect(x, f, h, 1.0)
    pgmg.ops.defect(xt, ft, -h, gt, norm=False)
    torch.cuda.synchronize()
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.correct(xt, et, scale=0.0)
