"""GPU: pgmg_extrap_grid (include/pgmg.h: the extrapolation of pgmg_solve_extrap on caller-owned
arrays) bitwise against tests/extrap_model.extrapolate.

k_extrap_add has k_interp_cubic's launch geometry (256 coarse columns per workgroup in x, bands
of 4 .. 32 coarse rows), so the sizes Nf are its boundaries: 17 (Nc = 9, the smallest legal size
but one: dominated by the one-sided formulas; 9 itself, Nc = 5, where every interior odd line
is one-sided, rides along), 33, 129 and 257 (more than one wave: lanes 0 and 63 load their halo
columns), 513 (Nc - 1 = 256: exactly one workgroup of coarse columns), 1025 (two workgroups in x,
128 bands).  The arrays have the odd pitch Nf, so every fine pair is an unaligned 16-byte access.
Fine and coarse are random with non-zero, different frames.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import extrap_model
import special_values as sv
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [9, 17, 33, 129, 257, 513, 1025]


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _edges(a):
    return np.concatenate([a[0, :], a[-1, :], a[:, 0], a[:, -1]])


@functools.lru_cache(maxsize=None)
def _state(Nf):
    """(fine, coarse, the model's result), read-only"""
    Nc = (Nf + 1) // 2
    rng = np.random.default_rng(4000 + Nf)
    fine, coarse = rng.standard_normal((Nf, Nf)), rng.standard_normal((Nc, Nc))
    want = extrap_model.extrapolate(fine, coarse)
    for a in (fine, coarse, want):
        a.setflags(write=False)
    return fine, coarse, want


@pytest.mark.parametrize("Nf", SIZES)
def test_extrapolate_bitwise(pgmg, Nf):
    import torch
    fine, coarse, want = _state(Nf)
    ft, ct = _t(fine), _t(coarse)
    pgmg.ops.extrapolate(ft, ct)
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert_bitwise(got, want, f"extrapolate Nf={Nf}")
    assert np.array_equal(bits(_edges(got)), bits(_edges(fine))), "frame written"
    assert_bitwise(ct.cpu().numpy(), coarse, "coarse is only read")
    # a second call works on the result of the first (every difference from the fine of before)
    pgmg.ops.extrapolate(ft, ct)
    torch.cuda.synchronize()
    assert_bitwise(ft.cpu().numpy(), extrap_model.extrapolate(want, coarse), f"twice Nf={Nf}")
    pgmg.ops.release()


def _special(Nf):
    Nc = (Nf + 1) // 2
    rng = np.random.default_rng(77)
    fine, coarse = rng.standard_normal((Nf, Nf)), rng.standard_normal((Nc, Nc))
    # the frame: -0, +0, a subnormal, Inf and NaN; none may change, none is computed with
    fine[0, 2], fine[0, 3], fine[-1, 5], fine[6, 0], fine[7, -1] = -0.0, 0.0, 5e-324, np.inf, np.nan
    fine[0, 0], fine[-1, -1] = -0.0, -np.inf
    # a patch where fine and coarse agree: D = +0 there, and phi + 0 keeps phi's words
    fine[8:20, 8:20] = 0.0
    coarse[4:10, 4:10] = 0.0
    fine[10, 10], fine[11, 11], fine[12, 13] = -0.0, 1e-310, -5e-324
    # subnormal differences (their third is subnormal too)
    fine[30, 30], coarse[15, 15] = 3e-310, 1e-310
    fine[30, 34], coarse[15, 17] = 0.0, 5e-324
    # non-finite words: Inf - Inf and 0 * Inf inside the interpolation
    fine[40, 40] = np.inf
    coarse[24, 24] = -np.inf
    fine[50, 20] = np.nan
    fine[45, 51] = np.inf          # an odd point: no D reads it, Inf + finite stays Inf
    # the one-sided corner
    coarse[0, 0], coarse[Nc - 1, Nc - 2] = 1e308, -1e308
    return fine, coarse


def test_special_values(pgmg):
    """+-0, subnormals, +-Inf and NaN: NaN exactly where the model has it, every other word
    bitwise the model's; then a grid of -0.0 (its interior becomes +0, its frame stays -0) and a
    subnormal-scale pair."""
    import torch
    Nf = 65
    fine, coarse = _special(Nf)
    want = extrap_model.extrapolate(fine, coarse)
    c = sv.census(want)
    print("census of the model's result:", c)
    assert c["nz"] >= 2 and c["sub"] >= 3 and c["inf"] >= 3 and 1 <= c["nan"] <= 0.25 * want.size, c
    ft = _t(fine)
    pgmg.ops.extrapolate(ft, _t(coarse))
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    sv.assert_bitwise_nan(got, want, "special words")
    nn = ~np.isnan(_edges(fine))
    assert np.array_equal(bits(_edges(got))[nn], bits(_edges(fine))[nn]), "frame written"
    assert np.array_equal(np.isnan(_edges(got)), np.isnan(_edges(fine)))
    for fine, coarse, what in (
            (np.full((Nf, Nf), -0.0), np.full((33, 33), -0.0), "negative zeros"),
            (_state(Nf)[0] * 1e-310, _state(Nf)[1] * 1e-310, "subnormal scale")):
        want = extrap_model.extrapolate(fine, coarse)
        ft = _t(fine)
        pgmg.ops.extrapolate(ft, _t(coarse))
        torch.cuda.synchronize()
        assert_bitwise(ft.cpu().numpy(), want, what)
    assert sv.census(want)["sub"] >= 1000
    pgmg.ops.release()


def test_two_streams_then_release(pgmg):
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    fa, ca, wa = _state(257)
    fb, cb, wb = _state(129)
    ta, tca, tb, tcb = _t(fa), _t(ca), _t(fb), _t(cb)
    torch.cuda.synchronize()
    pgmg.ops.extrapolate(ta, tca, stream=sa.cuda_stream)
    pgmg.ops.extrapolate(tb, tcb, stream=sb.cuda_stream)
    pgmg.ops.release(sa.cuda_stream)
    pgmg.ops.release(sb.cuda_stream)
    assert_bitwise(ta.cpu().numpy(), wa, "stream a")
    assert_bitwise(tb.cpu().numpy(), wb, "stream b")
    # a set released and used again allocates a fresh one
    tb2 = _t(fb)
    torch.cuda.synchronize()
    pgmg.ops.extrapolate(tb2, tcb, stream=sb.cuda_stream)
    pgmg.ops.release(sb.cuda_stream)
    assert_bitwise(tb2.cpu().numpy(), wb, "stream b again")


def test_argument_errors_touch_nothing(pgmg):
    import torch
    fine, coarse, _ = _state(33)
    ft, ct = _t(fine), _t(coarse)
    lib = pgmg.load()
    pf, pc = C.c_void_p(ft.data_ptr()), C.c_void_p(ct.data_ptr())
    for bad in (-1, 0, 3, 5, 7, 8, 10, 16, 32, 34, 100):
        assert lib.pgmg_extrap_grid(pf, pc, bad, None) == pgmg.PGMG_ERR_ARG, bad
    assert lib.pgmg_extrap_grid(None, pc, 33, None) == pgmg.PGMG_ERR_ARG
    assert lib.pgmg_extrap_grid(pf, None, 33, None) == pgmg.PGMG_ERR_ARG
    torch.cuda.synchronize()
    assert_bitwise(ft.cpu().numpy(), fine, "fine after refused calls")
    assert_bitwise(ct.cpu().numpy(), coarse, "coarse after refused calls")
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.extrapolate(_t(np.zeros((5, 5))), _t(np.zeros((3, 3))))
