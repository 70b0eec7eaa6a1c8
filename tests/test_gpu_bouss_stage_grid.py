"""GPU: pgmg_boussinesq_stage_grid (include/pgmg.h "Runge-Kutta buoyancy-driven flow", on
caller-owned arrays) through ops.boussinesq_stage, bitwise against tests/bouss_rk_model.stage on
random psi, w, T and saved w and T with non-zero frames.

k_bouss_stage is k_bouss_step with two more input streams, on the same decomposition grad_grid(N):
N = 5 (fewer rows than rows in flight; every interior point touches the frame), 9 (two bands, the
second of one row), 17, 33, 129 (64 pairs: exactly one wave), 257 (a second wave: lanes 0 and 63
load their halo), 513 (one full tile of 256 pairs), 1025 (two column tiles).  The arrays have the
odd pitch N, so every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bouss_model
import bouss_rk_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 17, 33, 129, 257, 513, 1025]
CANARY = 1234.5
PAIRS = ((0.5, 0.5), (0.75, 0.25), (bouss_rk_model.K3, bouss_rk_model.B3))
NAMES = ("psi", "w", "T", "w0", "T0")


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _field(N, which):
    """which = 0: psi; 1: w and 2: T, +-0 and subnormals on their frames; 3, 4: the saved w and T"""
    a = np.random.default_rng(9700 + 10 * N + which).standard_normal((N, N))
    if which == 1:
        a[0, 0], a[0, 2], a[-1, 1], a[2, 0], a[1, -1], a[-1, -1] = -0.0, -0.0, 0.0, 5e-324, -1e-310, 0.0
    if which == 2:
        a[0, 1], a[-1, 2], a[-1, 0], a[1, 0], a[2, -1], a[0, -1] = -0.0, 5e-324, -0.0, -0.0, 0.0, -1e-310
    a.setflags(write=False)
    return a


def _fields(N):
    return tuple(_field(N, k) for k in range(5))


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
    """Both outputs against the model for the three coefficient pairs of orders 2 and 3, h positive
    and negative, nu = kappa = 0, bx != 0; the frames of the outputs are w's and T's words; vmax
    exactly ops.boussinesq_step's; a call without vmax gives the same outputs; (0, 1) gives
    ops.boussinesq_step's numbers; the inputs are only read; the words beside the arrays stay."""
    import torch
    host = _fields(N)
    psi, w, T, w0, T0 = host
    dev = [_guarded(a) for a in host]
    pt, wt, Tt, w0t, T0t = (d[0] for d in dev)
    (owt, owb), (ott, otb) = _guarded(np.full((N, N), np.nan)), _guarded(np.full((N, N), np.nan))
    ewt, ett = _t(np.zeros((N, N))), _t(np.zeros((N, N)))
    cases = ((1.0 / (N - 1), 1e-3, 0.01, 0.02, (0.0, 20.0)), (-2.0 / (N - 1), 0.25, 0.0, 0.0, (-3.5, 2.25)),
             (0.7 / (N - 1), 1e-5, 3.0, 0.5, (1.5, 0.0)))
    for (h, dt, nu, kappa, buoy), (a, b) in zip(cases, PAIRS):
        wantw, wantt, wmax = bouss_rk_model.stage(psi, w, T, w0, T0, h, dt, nu, kappa, buoy, a, b)
        what = f"N={N} h={h} dt={dt} nu={nu} kappa={kappa} buoy={buoy} a={a} b={b}"
        owt.fill_(np.nan)
        ott.fill_(np.nan)
        torch.cuda.synchronize()
        ow, ot, vmax = pgmg.ops.boussinesq_stage(pt, wt, Tt, w0t, T0t, owt, ott, h, dt, nu, kappa, buoy,
                                                 a, b, vmax=True)
        assert ow is owt and ot is ott
        assert_bitwise(owt.cpu().numpy(), wantw, "stage w " + what)
        assert_bitwise(ott.cpu().numpy(), wantt, "stage T " + what)
        emax = pgmg.ops.boussinesq_step(pt, wt, Tt, ewt, ett, h, dt, nu, kappa, buoy, vmax=True)[2]
        print(f"{what}: vmax {vmax!r} step's {emax!r} model {wmax!r}")
        assert _same_bits(vmax, emax) and _same_bits(vmax, wmax), (what, vmax, emax, wmax)
        owt.fill_(np.nan)
        ott.fill_(np.nan)
        torch.cuda.synchronize()
        pgmg.ops.boussinesq_stage(pt, wt, Tt, w0t, T0t, owt, ott, h, dt, nu, kappa, buoy, a, b)   # asynchronous
        torch.cuda.synchronize()
        assert_bitwise(owt.cpu().numpy(), wantw, "stage w without vmax " + what)
        assert_bitwise(ott.cpu().numpy(), wantt, "stage T without vmax " + what)
        # (0, 1): 0 * W0 + 1 * e, the Euler pass's numbers (only the sign of a zero could differ)
        pgmg.ops.boussinesq_stage(pt, wt, Tt, w0t, T0t, owt, ott, h, dt, nu, kappa, buoy, 0.0, 1.0)
        torch.cuda.synchronize()
        ew, et = ewt.cpu().numpy(), ett.cpu().numpy()
        mw, mt, _ = bouss_model.step(psi, w, T, h, dt, nu, kappa, buoy)
        assert_bitwise(ew, mw, "the Euler pass w " + what)
        assert_bitwise(et, mt, "the Euler pass T " + what)
        assert np.array_equal(owt.cpu().numpy(), ew), "(0, 1) w " + what
        assert np.array_equal(ott.cpu().numpy(), et), "(0, 1) T " + what
    keep = np.ones((N, N), dtype=bool)
    keep[1:-1, 1:-1] = False
    assert np.array_equal(bits(owt.cpu().numpy())[keep], bits(w)[keep])
    assert np.array_equal(bits(ott.cpu().numpy())[keep], bits(T)[keep])
    for (t, buf), a, name in zip(dev, host, NAMES):
        assert_bitwise(t.cpu().numpy(), a, name + " is only read")
        _guards_intact(buf, f"{name} N={N}")
    _guards_intact(owb, f"wout N={N}")
    _guards_intact(otb, f"Tout N={N}")
    pgmg.ops.release()


@pytest.mark.parametrize("N", [9, 257])
def test_saved_fields_may_be_w_and_T(pgmg, N):
    """d_w0 == d_w and d_T0 == d_T: the outputs are a * w + b * ew and a * T + b * et."""
    psi, w, T = _field(N, 0), _field(N, 1), _field(N, 2)
    h, dt, nu, kappa, buoy = 1.0 / (N - 1), 1e-3, 0.01, 0.02, (0.0, 20.0)
    pt, wt, Tt, owt, ott = _t(psi), _t(w), _t(T), _t(np.zeros((N, N))), _t(np.zeros((N, N)))
    wantw, wantt, wmax = bouss_rk_model.stage(psi, w, T, w, T, h, dt, nu, kappa, buoy, 0.75, 0.25)
    vmax = pgmg.ops.boussinesq_stage(pt, wt, Tt, wt, Tt, owt, ott, h, dt, nu, kappa, buoy, 0.75, 0.25,
                                     vmax=True)[2]
    assert_bitwise(owt.cpu().numpy(), wantw, f"w0 is w, N={N}")
    assert_bitwise(ott.cpu().numpy(), wantt, f"T0 is T, N={N}")
    assert _same_bits(vmax, wmax)
    assert_bitwise(wt.cpu().numpy(), w, "w is only read")
    assert_bitwise(Tt.cpu().numpy(), T, "T is only read")
    pgmg.ops.release()


def _nan_equal_bits(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok]), what


def test_stage_special_values(pgmg):
    """NaN and Inf at interior points of the saved w and T touch only their own word of their own
    output; NaN frames of the saved fields reach nothing; NaN and Inf in psi, w and T spread as in
    the model."""
    N, h, dt, nu, kappa, buoy = 65, 1.0 / 64, 1e-3, 0.01, 0.02, (0.5, 20.0)
    a, b = bouss_rk_model.K3, bouss_rk_model.B3
    psi, w, T, w0, T0 = (np.array(f) for f in _fields(N))
    clean = bouss_rk_model.stage(psi, w, T, w0, T0, h, dt, nu, kappa, buoy, a, b)
    w0[7, 9], w0[33, 1], w0[63, 63], w0[40, 2] = np.nan, np.inf, -np.inf, 1e308
    T0[8, 9], T0[1, 33], T0[63, 1], T0[2, 40] = np.nan, -np.inf, np.inf, -1e308
    for Z in (w0, T0):
        Z[0, :] = Z[-1, :] = np.nan
        Z[:, 0] = Z[:, -1] = np.nan
    wantw, wantt, wmax = bouss_rk_model.stage(psi, w, T, w0, T0, h, dt, nu, kappa, buoy, a, b)
    for want, was, at in ((wantw, clean[0], [(7, 9), (33, 1), (63, 63), (40, 2)]),
                          (wantt, clean[1], [(8, 9), (1, 33), (63, 1), (2, 40)])):
        assert np.isnan(want).sum() == 1 and np.isinf(want).sum() == 2
        differs = bits(want) != bits(was)
        assert sorted(zip(*np.nonzero(differs))) == sorted(at)   # only their own words
    zeros = lambda: _t(np.zeros((N, N)))
    ow, ot, vmax = pgmg.ops.boussinesq_stage(_t(psi), _t(w), _t(T), _t(w0), _t(T0), zeros(), zeros(), h,
                                             dt, nu, kappa, buoy, a, b, vmax=True)
    _nan_equal_bits(ow.cpu().numpy(), wantw, "w")
    _nan_equal_bits(ot.cpu().numpy(), wantt, "T")
    assert np.isfinite(wmax) and _same_bits(vmax, wmax)
    # an Inf in a saved field times a = 0 is a NaN, as in the model
    wantw, wantt, _ = bouss_rk_model.stage(psi, w, T, w0, T0, h, dt, nu, kappa, buoy, 0.0, 1.0)
    ow, ot = pgmg.ops.boussinesq_stage(_t(psi), _t(w), _t(T), _t(w0), _t(T0), zeros(), zeros(), h, dt, nu,
                                       kappa, buoy, 0.0, 1.0)
    assert np.isnan(wantw).sum() == 3 and np.isnan(wantt).sum() == 3
    _nan_equal_bits(ow.cpu().numpy(), wantw, "w, a = 0")
    _nan_equal_bits(ot.cpu().numpy(), wantt, "T, a = 0")
    psi[10, 10], psi[30, 0] = np.nan, np.inf
    w[20, 20], w[0, 5], w[50, 3] = np.nan, np.nan, -np.inf
    T[25, 40], T[5, 0], T[3, 50] = np.nan, np.nan, np.inf
    wantw, wantt, wmax = bouss_rk_model.stage(psi, w, T, w0, T0, h, dt, nu, kappa, buoy, a, b)
    ow, ot, vmax = pgmg.ops.boussinesq_stage(_t(psi), _t(w), _t(T), _t(w0), _t(T0), zeros(), zeros(), h,
                                             dt, nu, kappa, buoy, a, b, vmax=True)
    assert 1 <= np.isnan(wantw).sum() < 64 and 1 <= np.isnan(wantt).sum() < 64
    _nan_equal_bits(ow.cpu().numpy(), wantw, "w, special inputs")
    _nan_equal_bits(ot.cpu().numpy(), wantt, "T, special inputs")
    assert np.isinf(wmax) and _same_bits(vmax, wmax)
    pgmg.ops.release()


def test_streams(pgmg):
    import torch
    sa = torch.cuda.Stream()
    N, h, dt, nu, kappa, buoy = 257, 1.0 / 256, 1e-3, 0.01, 0.02, (0.0, 20.0)
    psi, w, T, w0, T0 = _fields(N)
    pt, wt, Tt, w0t, T0t = (_t(a) for a in (psi, w, T, w0, T0))
    owt, ott = _t(np.zeros((N, N))), _t(np.zeros((N, N)))
    torch.cuda.synchronize()
    walls = (1.0, -2.0, 0.5, 3.0)
    import vort_model
    ww = vort_model.wall(psi, w, h, walls)
    Tw = bouss_model.wall_scalar(T, 5)
    wantw, wantt, wmax = bouss_rk_model.stage(psi, ww, Tw, w0, T0, h, dt, nu, kappa, buoy, 0.5, 0.5)
    pgmg.ops.wall_vorticity(pt, wt, h, walls, stream=sa.cuda_stream)
    pgmg.ops.wall_scalar(Tt, 5, stream=sa.cuda_stream)
    vmax = pgmg.ops.boussinesq_stage(pt, wt, Tt, w0t, T0t, owt, ott, h, dt, nu, kappa, buoy, 0.5, 0.5,
                                     vmax=True, stream=sa.cuda_stream)[2]
    assert _same_bits(vmax, wmax)
    pgmg.ops.release(sa.cuda_stream)
    assert_bitwise(owt.cpu().numpy(), wantw, "walls then stage on a stream: w")
    assert_bitwise(ott.cpu().numpy(), wantt, "walls then stage on a stream: T")
    pgmg.ops.release()


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    keep = [np.random.default_rng(k).standard_normal((N, N)) for k in range(7)]
    ts = [_t(a) for a in keep]
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pp, pw, pT, pw0, pT0, pow_, pot = (C.c_void_p(t.data_ptr()) for t in ts)
    m = C.c_double(-7.0)
    host = np.zeros((N, N))
    ph = host.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    good = (C.c_double * 2)(0.0, 20.0)

    def stage(psi=pp, w=pw, T=pT, w0=pw0, T0=pT0, wout=pow_, tout=pot, N=N, h=h, dt=1e-3, nu=0.01,
              kappa=0.02, buoy=good, a=0.75, b=0.25, vmax=True):
        return lib.pgmg_boussinesq_stage_grid(psi, w, T, w0, T0, wout, tout, N, h, dt, nu, kappa, buoy, a,
                                              b, C.byref(m) if vmax else None, None)

    for bad in (0, 3, 4, 6, 10, 32, 34):
        assert stage(N=bad) == ARG, bad
    for bad in (0.0, -0.0, nan, inf):
        assert stage(h=bad) == ARG, bad
    for bad in (0.0, -1e-3, nan, inf):
        assert stage(dt=bad) == ARG, bad
    for bad in (-1e-9, nan, inf):
        assert stage(nu=bad) == ARG and stage(kappa=bad) == ARG, bad
    assert stage(buoy=None) == ARG
    for k in range(2):
        for bad in (nan, inf, -inf):
            v = [0.0, 20.0]
            v[k] = bad
            assert stage(buoy=(C.c_double * 2)(*v)) == ARG, (k, bad)
    for bad in (nan, inf, -inf):
        assert stage(a=bad) == ARG and stage(b=bad) == ARG, bad
    for name in ("psi", "w", "T", "w0", "T0", "wout", "tout"):
        assert stage(**{name: None}) == ARG, name
    for out in ("wout", "tout"):
        for q in (pp, pw, pT, pw0, pT0):
            assert stage(**{out: q}) == ARG
        # one element shared with an input
        assert stage(**{out: C.c_void_p(ts[3].data_ptr() + 8 * (N * N - 1))}) == ARG
        assert stage(**{out: ph}) == ARG                                   # not device memory
    assert stage(wout=pot) == ARG and stage(tout=pow_) == ARG              # the outputs overlap
    assert stage(tout=C.c_void_p(ts[5].data_ptr() + 8 * (N * N - 1))) == ARG
    assert not host.any()
    torch.cuda.synchronize()
    assert m.value == -7.0
    for t, a, name in zip(ts, keep, NAMES + ("wout", "Tout")):
        assert_bitwise(t.cpu().numpy(), a, name + " after refused calls")
    assert stage() == pgmg.PGMG_OK and stage(vmax=False) == pgmg.PGMG_OK
    assert stage(w0=pw, T0=pT) == pgmg.PGMG_OK
    assert stage(a=-1.5, b=0.0) == pgmg.PGMG_OK                            # finite is all that is asked
    with pytest.raises(pgmg.PgmgError):
        z = _t(np.zeros((6, 6)))
        pgmg.ops.boussinesq_stage(z, z, z, z, z, _t(np.zeros((6, 6))), _t(np.zeros((6, 6))), 0.2, 1e-3, 0.0,
                                  0.0, (0.0, 1.0), 0.5, 0.5)
    pgmg.ops.release()
