"""GPU: pgmg_boussinesq_grid and pgmg_wall_scalar_grid (include/pgmg.h "Buoyancy-driven flow", on
caller-owned arrays) through ops.boussinesq_step and ops.wall_scalar, bitwise against
tests/bouss_model.py on random psi, w and T with non-zero frames.

k_bouss_step has k_vort_step's shape and decomposition grad_grid(N), so the sizes are those of
tests/test_gpu_vorticity_grid.py, for its reasons: 5 (one band; every interior point touches the
frame), 9 (two bands of rows, 8 + 1), 17, 65, 129 (64 pairs: exactly one wave), 257 (a second wave:
lanes 0 and 63 load their halo), 1025 (two column tiles).  The arrays have the odd pitch N, so
every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bouss_model
import vort_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 17, 65, 129, 257, 1025]
CANARY = 1234.5
# (h as a multiple of 1 / (N - 1), dt, nu, kappa, buoy): h positive and negative, nu = 0, kappa =
# 0, and the three buoyancies
CASES = [(1.0, 1e-3, 0.01, 0.02, (0.0, 710.0)), (-2.0, 0.25, 0.0, 0.7, (-3.5, 2.25)),
         (0.7, 1e-5, 3.0, 0.0, (0.0, 0.0))]


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _field(N, which):
    """which = 0: psi; 1: w; 2: T -- the last two with +-0 and subnormals on their frames"""
    a = np.random.default_rng(9300 + 10 * N + which).standard_normal((N, N))
    if which == 1:
        a[0, 0], a[0, 2], a[-1, 1], a[2, 0], a[1, -1], a[-1, -1] = -0.0, -0.0, 0.0, 5e-324, -1e-310, 0.0
    if which == 2:
        a[0, 1], a[0, -1], a[-1, 3], a[1, 0], a[3, -1], a[-1, 0] = -0.0, -0.0, 5e-324, -0.0, 0.0, -1e-310
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
def test_step_bitwise(pgmg, N):
    """Both outputs against the model for every case of CASES; their frames are the words of w and
    of T (+-0 and subnormals carried); vmax exactly the model's maximum; a call without vmax gives
    the same outputs; T_out is also the device's own ops.vorticity_step of T with kappa; psi, w
    and T are only read; the words beside all five arrays stay."""
    import torch
    psi, w, T = _field(N, 0), _field(N, 1), _field(N, 2)
    (pt, pb), (wt, wb), (tt, tb) = _guarded(psi), _guarded(w), _guarded(T)
    nan = np.full((N, N), np.nan)
    (wo, wob), (to, tob) = _guarded(nan), _guarded(nan)
    vo = _t(nan)
    keep = np.ones((N, N), dtype=bool)
    keep[1:-1, 1:-1] = False
    for hm, dt, nu, kappa, buoy in CASES:
        h = hm / (N - 1)
        want_w, want_t, wmax = bouss_model.step(psi, w, T, h, dt, nu, kappa, buoy)
        what = f"N={N} h={h} dt={dt} nu={nu} kappa={kappa} buoy={buoy}"
        for o in (wo, to):
            o.fill_(np.nan)
        torch.cuda.synchronize()
        a, b, vmax = pgmg.ops.boussinesq_step(pt, wt, tt, wo, to, h, dt, nu, kappa, buoy, vmax=True)
        assert a is wo and b is to
        assert_bitwise(wo.cpu().numpy(), want_w, "w_out " + what)
        assert_bitwise(to.cpu().numpy(), want_t, "T_out " + what)
        print(f"{what}: vmax {vmax!r} model {wmax!r}")
        assert _same_bits(vmax, wmax), (what, vmax, wmax)
        for o in (wo, to):
            o.fill_(np.nan)
        torch.cuda.synchronize()
        pgmg.ops.boussinesq_step(pt, wt, tt, wo, to, h, dt, nu, kappa, buoy)   # asynchronous
        pgmg.ops.vorticity_step(pt, tt, vo, h, dt, kappa)
        torch.cuda.synchronize()
        assert_bitwise(wo.cpu().numpy(), want_w, "w_out without vmax " + what)
        assert_bitwise(to.cpu().numpy(), want_t, "T_out without vmax " + what)
        assert_bitwise(to.cpu().numpy(), vo.cpu().numpy(), "T_out against ops.vorticity_step " + what)
        assert np.array_equal(bits(want_w)[keep], bits(w)[keep])
        assert np.array_equal(bits(want_t)[keep], bits(T)[keep])
    for t, a, name in ((pt, psi, "psi"), (wt, w, "w"), (tt, T, "T")):
        assert_bitwise(t.cpu().numpy(), a, name + " is only read")
    for b, name in ((pb, "psi"), (wb, "w"), (tb, "T"), (wob, "w_out"), (tob, "T_out")):
        _guards_intact(b, f"{name} N={N}")
    pgmg.ops.release()


def test_step_special_values(pgmg):
    """NaN, +-Inf, -0.0 and subnormals in psi, w and T at interior points, beside the frame and on
    it: the outputs are NaN exactly where the model's are and bitwise elsewhere; vmax skips the
    NaN terms as the model's fmax does."""
    N, h, dt, nu, kappa, buoy = 65, 1.0 / 64, 1e-3, 0.01, 0.02, (-3.5, 2.25)
    psi, w, T = (np.array(_field(N, k)) for k in range(3))
    psi[10, 10], psi[30, 0], psi[40, 41], psi[1, 7] = np.nan, np.inf, 1e300, -0.0
    w[20, 20], w[0, 5], w[50, 3], w[1, 1], w[33, 34] = np.nan, np.nan, -np.inf, 5e-324, -0.0
    T[25, 45], T[5, 0], T[63, 63], T[-1, 9], T[12, 1], T[44, 20] = np.nan, np.nan, np.inf, -np.inf, -1e-310, -0.0
    zeros = np.zeros((N, N))

    def run(psi, w, T):
        wo, to, vmax = pgmg.ops.boussinesq_step(_t(psi), _t(w), _t(T), _t(zeros), _t(zeros), h, dt, nu,
                                                kappa, buoy, vmax=True)
        return wo.cpu().numpy(), to.cpu().numpy(), vmax

    want_w, want_t, wmax = bouss_model.step(psi, w, T, h, dt, nu, kappa, buoy)
    got_w, got_t, vmax = run(psi, w, T)
    for got, want, name in ((got_w, want_w, "w_out"), (got_t, want_t, "T_out")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert 1 <= np.isnan(want).sum() < 64, name
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok]), name
    assert np.isinf(wmax) and _same_bits(vmax, wmax)
    psi[30, 0], psi[40, 41] = 0.0, 1.0
    wmax = bouss_model.step(psi, w, T, h, dt, nu, kappa, buoy)[2]
    assert np.isfinite(wmax) and _same_bits(run(psi, w, T)[2], wmax)
    assert run(np.full((N, N), np.nan), w, T)[2] == 0.0
    pgmg.ops.release()


@pytest.mark.parametrize("N", [5, 9, 129, 1025])
def test_wall_scalar_bitwise(pgmg, N):
    """All 16 masks against the model: the set walls as the formula gives them; the corners, the
    clear walls and the interior keep their bits; the words beside the array stay."""
    import torch
    T = _field(N, 2)
    tt, tb = _guarded(T)
    inner = np.zeros((N, N), dtype=bool)
    inner[1:-1, 1:-1] = True
    walls = {1: (0, slice(1, -1)), 2: (-1, slice(1, -1)), 4: (slice(1, -1), 0), 8: (slice(1, -1), -1)}
    for mask in range(16):
        want = bouss_model.wall_scalar(T, mask)
        tt.copy_(_t(T))
        torch.cuda.synchronize()
        assert pgmg.ops.wall_scalar(tt, mask) is tt
        torch.cuda.synchronize()
        got = tt.cpu().numpy()
        assert_bitwise(got, want, f"wall_scalar N={N} mask={mask}")
        assert np.array_equal(bits(got)[inner], bits(T)[inner]), "the interior"
        for j, i in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert bits(got)[j, i] == bits(T)[j, i], "a corner was written"
        for bit, where in walls.items():
            if not mask & bit:
                assert np.array_equal(bits(got)[where], bits(T)[where]), (mask, bit)
            else:
                assert not np.array_equal(bits(got)[where], bits(T)[where]), (mask, bit)
    _guards_intact(tb, f"T N={N}")
    tt.copy_(_t(T))
    assert pgmg.ops.wall_scalar(tt, ("left", "top")) is tt
    torch.cuda.synchronize()
    assert_bitwise(tt.cpu().numpy(), bouss_model.wall_scalar(T, 2 | 4), "walls by name")


def test_streams(pgmg):
    """Two streams used concurrently, each with its own arrays and a different case, give the bits
    one stream gives (the model's): the per-stream scratch sets do not mix."""
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    N = 257
    psi, w, T = _field(N, 0), _field(N, 1), _field(N, 2)
    runs = []
    for s, (hm, dt, nu, kappa, buoy) in ((sa, CASES[0]), (sb, CASES[1])):
        runs.append(dict(s=s, h=hm / (N - 1), dt=dt, nu=nu, kappa=kappa, buoy=buoy, pt=_t(psi), wt=_t(w),
                         tt=_t(T), wo=_t(np.zeros((N, N))), to=_t(np.zeros((N, N)))))
    torch.cuda.synchronize()
    for _ in range(2):   # interleaved: wall then step on each stream
        for r in runs:
            pgmg.ops.wall_scalar(r["tt"], 3, stream=r["s"].cuda_stream)
            pgmg.ops.boussinesq_step(r["pt"], r["wt"], r["tt"], r["wo"], r["to"], r["h"], r["dt"], r["nu"],
                                     r["kappa"], r["buoy"], stream=r["s"].cuda_stream)
    vm = [pgmg.ops.boussinesq_step(r["pt"], r["wt"], r["tt"], r["wo"], r["to"], r["h"], r["dt"], r["nu"],
                                   r["kappa"], r["buoy"], vmax=True, stream=r["s"].cuda_stream)[2]
          for r in runs]
    torch.cuda.synchronize()
    Tw = bouss_model.wall_scalar(T, 3)
    for r, m in zip(runs, vm):
        want_w, want_t, wmax = bouss_model.step(psi, w, Tw, r["h"], r["dt"], r["nu"], r["kappa"], r["buoy"])
        assert_bitwise(r["wo"].cpu().numpy(), want_w, "w_out on a stream")
        assert_bitwise(r["to"].cpu().numpy(), want_t, "T_out on a stream")
        assert _same_bits(m, wmax)
        pgmg.ops.release(r["s"].cuda_stream)
    pgmg.ops.release()


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    keep = [np.random.default_rng(k).standard_normal((N, N)) for k in range(3)]
    keep += [np.full((N, N), np.nan), np.full((N, N), np.nan)]
    pt, wt, tt, wo, to = (_t(a) for a in keep)
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pp, pw, pT, pwo, pto = (C.c_void_p(t.data_ptr()) for t in (pt, wt, tt, wo, to))
    m = C.c_double(-7.0)
    host = np.zeros((N, N))
    ph = host.ctypes.data_as(C.c_void_p)
    good = (C.c_double * 2)(0.0, 710.0)

    def step(psi=pp, w=pw, T=pT, wout=pwo, tout=pto, N=N, h=h, dt=1e-3, nu=0.01, kappa=0.02, buoy=good,
             vmax=True):
        return lib.pgmg_boussinesq_grid(psi, w, T, wout, tout, N, h, dt, nu, kappa, buoy,
                                        C.byref(m) if vmax else None, None)

    def wall(T=pwo, N=N, mask=15):
        return lib.pgmg_wall_scalar_grid(T, N, mask, None)

    for bad in (0, 3, 4, 6, 10, 32, 34):
        assert step(N=bad) == ARG and wall(N=bad) == ARG, bad
    for bad in (0.0, -0.0, float("nan"), float("inf")):
        assert step(h=bad) == ARG, bad
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        assert step(dt=bad) == ARG, bad
    for bad in (-1e-9, float("nan"), float("inf")):
        assert step(nu=bad) == ARG and step(kappa=bad) == ARG, bad
    assert step(buoy=None) == ARG
    for k in range(2):
        for bad in (float("nan"), float("inf"), -float("inf")):
            b = [0.0, 710.0]
            b[k] = bad
            assert step(buoy=(C.c_double * 2)(*b)) == ARG, (k, bad)
    for name in ("psi", "w", "T", "wout", "tout"):
        assert step(**{name: None}) == ARG, name
    for name in ("wout", "tout"):
        for other in (pp, pw, pT):
            assert step(**{name: other}) == ARG, name                         # an output on an input
        assert step(**{name: C.c_void_p(pt.data_ptr() + 8 * (N * N - 1))}) == ARG   # one element shared
        assert step(**{name: ph}) == ARG                                      # not device memory
    assert step(wout=pto) == ARG and step(tout=pwo) == ARG                    # the outputs overlap
    for bad in (16, 17, 32, 255, 2 ** 31):
        assert wall(mask=bad) == ARG, bad
    assert wall(T=None) == ARG and wall(T=ph) == ARG
    assert not host.any()
    torch.cuda.synchronize()
    assert m.value == -7.0
    for t, a, name in zip((pt, wt, tt, wo, to), keep, ("psi", "w", "T", "w_out", "T_out")):
        assert_bitwise(t.cpu().numpy(), a, name + " after refused calls")
    assert step() == pgmg.PGMG_OK and step(vmax=False) == pgmg.PGMG_OK and wall(mask=0) == pgmg.PGMG_OK
    assert wall() == pgmg.PGMG_OK
    with pytest.raises(pgmg.PgmgError):
        z = [_t(np.zeros((6, 6))) for _ in range(5)]
        pgmg.ops.boussinesq_step(*z, 0.2, 1e-3, 0.0, 0.0, (0.0, 1.0))
    with pytest.raises(ValueError):
        pgmg.ops.wall_scalar(tt, ("north",))
    for bad in (2 ** 32 + 1, -1):          # not an unsigned 32-bit mask: never truncated to one
        with pytest.raises(ValueError):
            pgmg.ops.wall_scalar(tt, bad)
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.wall_scalar(tt, 16)
    assert_bitwise(tt.cpu().numpy(), keep[2], "T after refused masks")
    pgmg.ops.release()
