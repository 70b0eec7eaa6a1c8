"""GPU: pgmg_vorticity_stage_grid (include/pgmg.h "Runge-Kutta vorticity transport", on
caller-owned arrays) through ops.vorticity_stage, bitwise against tests/vort_rk_model.stage on
random psi, omega and saved omega with non-zero frames.

k_vort_stage is k_vort_step with a third input stream, on the same decomposition grad_grid(N), so
the sizes are test_gpu_vorticity_grid.py's, for its reasons: 5 (one band; every interior point
touches the frame), 9 (two bands of rows), 17, 65, 129 (64 pairs: exactly one wave), 257 (a second
wave: lanes 0 and 63 load their halo), 1025 (two column tiles).  The arrays have the odd pitch N, so
every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import vort_model
import vort_rk_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 17, 65, 129, 257, 1025]
CANARY = 1234.5
PAIRS = ((0.5, 0.5), (0.75, 0.25), (vort_rk_model.K3, vort_rk_model.B3))


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _field(N, which):
    """which = 0: psi; 1: omega, +-0 and subnormals on its frame; 2: the saved omega"""
    a = np.random.default_rng(9300 + 10 * N + which).standard_normal((N, N))
    if which == 1:
        a[0, 0], a[0, 2], a[-1, 1], a[2, 0], a[1, -1], a[-1, -1] = -0.0, -0.0, 0.0, 5e-324, -1e-310, 0.0
    a.setflags(write=False)
    return a


def _guarded(a):
    """a device copy of `a` inside a larger buffer of canaries: (the N x N view, the buffer)"""
    import torch
    n = a.size
    buf = torch.full((n + 64,), CANARY, dtype=torch.float64, device="cuda:0")
    view = buf[32:32 + n].view(a.shape)
    view.copy_(_t(a))
    return view, buf


def _guards_intact(buf, what):
    b = buf.cpu().numpy()
    assert np.all(b[:32] == CANARY) and np.all(b[-32:] == CANARY), what + ": a word beside the array changed"


def _same_bits(a, b):
    return bits(np.array([a]))[0] == bits(np.array([b]))[0]


@pytest.mark.parametrize("N", SIZES)
def test_stage_bitwise(pgmg, N):
    """out against the model for the three coefficient pairs of orders 2 and 3, h positive and
    negative, nu = 0; the frame of out is omega's words; vmax exactly ops.vorticity_step's; a call
    without vmax gives the same out; (0, 1) gives ops.vorticity_step's numbers; the inputs are only
    read; the words beside the arrays stay."""
    import torch
    psi, w, w0 = _field(N, 0), _field(N, 1), _field(N, 2)
    (pt, pb), (wt, wb), (zt, zb) = _guarded(psi), _guarded(w), _guarded(w0)
    ot, ob = _guarded(np.full((N, N), np.nan))
    et = _t(np.zeros((N, N)))
    cases = ((1.0 / (N - 1), 1e-3, 0.01), (-2.0 / (N - 1), 0.25, 0.0), (0.7 / (N - 1), 1e-5, 3.0))
    for (h, dt, nu), (a, b) in zip(cases, PAIRS):
        want, wmax = vort_rk_model.stage(psi, w, w0, h, dt, nu, a, b)
        what = f"N={N} h={h} dt={dt} nu={nu} a={a} b={b}"
        ot.fill_(np.nan)
        torch.cuda.synchronize()
        out, vmax = pgmg.ops.vorticity_stage(pt, wt, zt, ot, h, dt, nu, a, b, vmax=True)
        assert out is ot
        assert_bitwise(ot.cpu().numpy(), want, "stage " + what)
        emax = pgmg.ops.vorticity_step(pt, wt, et, h, dt, nu, vmax=True)[1]
        print(f"{what}: vmax {vmax!r} step's {emax!r} model {wmax!r}")
        assert _same_bits(vmax, emax) and _same_bits(vmax, wmax), (what, vmax, emax, wmax)
        ot.fill_(np.nan)
        torch.cuda.synchronize()
        pgmg.ops.vorticity_stage(pt, wt, zt, ot, h, dt, nu, a, b)   # asynchronous
        torch.cuda.synchronize()
        assert_bitwise(ot.cpu().numpy(), want, "stage without vmax " + what)
        # (0, 1): 0 * W0 + 1 * e, the Euler pass's numbers (only the sign of a zero could differ)
        pgmg.ops.vorticity_stage(pt, wt, zt, ot, h, dt, nu, 0.0, 1.0)
        torch.cuda.synchronize()
        euler = et.cpu().numpy()
        assert_bitwise(euler, vort_model.step(psi, w, h, dt, nu)[0], "the Euler pass " + what)
        assert np.array_equal(ot.cpu().numpy(), euler), "(0, 1) " + what
    keep = np.ones((N, N), dtype=bool)
    keep[1:-1, 1:-1] = False
    assert np.array_equal(bits(ot.cpu().numpy())[keep], bits(w)[keep])
    for t, a, name in ((pt, psi, "psi"), (wt, w, "omega"), (zt, w0, "omega0")):
        assert_bitwise(t.cpu().numpy(), a, name + " is only read")
    for buf, name in ((pb, "psi"), (wb, "omega"), (zb, "omega0"), (ob, "out")):
        _guards_intact(buf, f"{name} N={N}")
    pgmg.ops.release()


@pytest.mark.parametrize("N", [9, 257])
def test_saved_field_may_be_omega(pgmg, N):
    """d_w0 == d_w: out = a * w + b * e."""
    import torch
    psi, w = _field(N, 0), _field(N, 1)
    h, dt, nu = 1.0 / (N - 1), 1e-3, 0.01
    pt, wt, ot = _t(psi), _t(w), _t(np.zeros((N, N)))
    want, wmax = vort_rk_model.stage(psi, w, w, h, dt, nu, 0.75, 0.25)
    vmax = pgmg.ops.vorticity_stage(pt, wt, wt, ot, h, dt, nu, 0.75, 0.25, vmax=True)[1]
    assert_bitwise(ot.cpu().numpy(), want, f"w0 is w, N={N}")
    assert _same_bits(vmax, wmax)
    assert_bitwise(wt.cpu().numpy(), w, "omega is only read")
    pgmg.ops.release()


def test_stage_special_values(pgmg):
    """NaN and Inf in the saved omega (and in psi and omega): out NaN exactly where the model has
    it and bitwise elsewhere; a NaN on the saved omega's frame reaches nothing."""
    N, h, dt, nu = 65, 1.0 / 64, 1e-3, 0.01
    a, b = vort_rk_model.K3, vort_rk_model.B3
    psi, w, w0 = np.array(_field(N, 0)), np.array(_field(N, 1)), np.array(_field(N, 2))
    w0[7, 9], w0[33, 1], w0[63, 63], w0[40, 2] = np.nan, np.inf, -np.inf, 1e308
    w0[0, :] = w0[-1, :] = np.nan
    w0[:, 0] = w0[:, -1] = np.nan
    want, wmax = vort_rk_model.stage(psi, w, w0, h, dt, nu, a, b)
    assert np.isnan(want).sum() == 1 and np.isinf(want).sum() == 2
    out, vmax = pgmg.ops.vorticity_stage(_t(psi), _t(w), _t(w0), _t(np.zeros((N, N))), h, dt, nu, a, b,
                                         vmax=True)
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isfinite(wmax) and _same_bits(vmax, wmax)
    # an Inf in W0 times a = 0 is a NaN, as in the model
    want = vort_rk_model.stage(psi, w, w0, h, dt, nu, 0.0, 1.0)[0]
    got = pgmg.ops.vorticity_stage(_t(psi), _t(w), _t(w0), _t(np.zeros((N, N))), h, dt, nu, 0.0, 1.0)
    got = got.cpu().numpy()
    assert np.isnan(want).sum() == 3 and np.array_equal(np.isnan(got), np.isnan(want))
    psi[10, 10], psi[30, 0] = np.nan, np.inf
    w[20, 20], w[0, 5], w[50, 3] = np.nan, np.nan, -np.inf
    want, wmax = vort_rk_model.stage(psi, w, w0, h, dt, nu, a, b)
    out, vmax = pgmg.ops.vorticity_stage(_t(psi), _t(w), _t(w0), _t(np.zeros((N, N))), h, dt, nu, a, b,
                                         vmax=True)
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and 1 <= np.isnan(want).sum() < 64
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isinf(wmax) and _same_bits(vmax, wmax)
    pgmg.ops.release()


def test_streams(pgmg):
    import torch
    sa = torch.cuda.Stream()
    N, h, dt, nu = 257, 1.0 / 256, 1e-3, 0.01
    psi, w, w0 = _field(N, 0), _field(N, 1), _field(N, 2)
    pt, wt, zt, ot = _t(psi), _t(w), _t(w0), _t(np.zeros((N, N)))
    torch.cuda.synchronize()
    walls = (1.0, -2.0, 0.5, 3.0)
    ww = vort_model.wall(psi, w, h, walls)
    want, wmax = vort_rk_model.stage(psi, ww, w0, h, dt, nu, 0.5, 0.5)
    pgmg.ops.wall_vorticity(pt, wt, h, walls, stream=sa.cuda_stream)
    vmax = pgmg.ops.vorticity_stage(pt, wt, zt, ot, h, dt, nu, 0.5, 0.5, vmax=True,
                                    stream=sa.cuda_stream)[1]
    assert _same_bits(vmax, wmax)
    pgmg.ops.release(sa.cuda_stream)
    assert_bitwise(ot.cpu().numpy(), want, "wall then stage on a stream")
    pgmg.ops.release()


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    keep = [np.random.default_rng(k).standard_normal((N, N)) for k in range(4)]
    pt, wt, zt, ot = (_t(a) for a in keep)
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pp, pw, pz, po = (C.c_void_p(t.data_ptr()) for t in (pt, wt, zt, ot))
    m = C.c_double(-7.0)
    host = np.zeros((N, N))
    ph = host.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def stage(psi=pp, w=pw, w0=pz, out=po, N=N, h=h, dt=1e-3, nu=0.01, a=0.75, b=0.25, vmax=True):
        return lib.pgmg_vorticity_stage_grid(psi, w, w0, out, N, h, dt, nu, a, b,
                                             C.byref(m) if vmax else None, None)

    for bad in (0, 3, 4, 6, 10, 32, 34):
        assert stage(N=bad) == ARG, bad
    for bad in (0.0, -0.0, nan, inf):
        assert stage(h=bad) == ARG, bad
    for bad in (0.0, -1e-3, nan, inf):
        assert stage(dt=bad) == ARG, bad
    for bad in (-1e-9, nan, inf):
        assert stage(nu=bad) == ARG, bad
    for bad in (nan, inf, -inf):
        assert stage(a=bad) == ARG and stage(b=bad) == ARG, bad
    assert stage(psi=None) == ARG and stage(w=None) == ARG and stage(w0=None) == ARG
    assert stage(out=None) == ARG
    assert stage(out=pp) == ARG and stage(out=pw) == ARG and stage(out=pz) == ARG
    assert stage(out=C.c_void_p(zt.data_ptr() + 8 * (N * N - 1))) == ARG   # one element shared
    assert stage(out=ph) == ARG                                            # not device memory
    assert not host.any()
    torch.cuda.synchronize()
    assert m.value == -7.0
    for t, a, name in zip((pt, wt, zt, ot), keep, ("psi", "omega", "omega0", "out")):
        assert_bitwise(t.cpu().numpy(), a, name + " after refused calls")
    assert stage() == pgmg.PGMG_OK and stage(vmax=False) == pgmg.PGMG_OK and stage(w0=pw) == pgmg.PGMG_OK
    assert stage(a=-1.5, b=0.0) == pgmg.PGMG_OK                            # finite is all that is asked
    with pytest.raises(pgmg.PgmgError):
        z = _t(np.zeros((6, 6)))
        pgmg.ops.vorticity_stage(z, z, z, _t(np.zeros((6, 6))), 0.2, 1e-3, 0.0, 0.5, 0.5)
    pgmg.ops.release()
