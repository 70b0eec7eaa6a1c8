"""GPU: pgmg_vorticity_grid and pgmg_wall_vorticity_grid (include/pgmg.h "Vorticity transport", on
caller-owned arrays) through ops.vorticity_step and ops.wall_vorticity, bitwise against
tests/vort_model.py on random psi and omega with non-zero frames.

k_vort_step has k_gradient's shape and decomposition grad_grid(N): a lane owns a column pair, a
wave 128 columns, a workgroup 512 (tiles = ceil((N - 1) / 2 / 256)), bands of 8 rows below N =
4097.  The sizes: 5 (one band; every interior point touches the frame), 9 (TWO_BANDS: the smallest
N with two bands of rows, 8 + 1), 17, 65, 129 (64 pairs: exactly one wave), 257 (a second wave:
lanes 0 and 63 load their halo), 1025 (TWO_TILES: the smallest N with two column tiles, 512 pairs).
The arrays have the odd pitch N, so every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import vort_model
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

TWO_BANDS, TWO_TILES = 9, 1025
SIZES = [5, TWO_BANDS, 17, 65, 129, 257, TWO_TILES]
CANARY = 1234.5
WALLS = (1.0, -2.0, 0.5, 3.0)


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _field(N, which):
    a = np.random.default_rng(8100 + 10 * N + which).standard_normal((N, N))
    if which == 1:   # omega: +-0 and subnormals on the frame, a -0.0 in a corner
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


def test_the_named_sizes(pgmg):
    """TWO_BANDS and TWO_TILES are what the decomposition says they are: grad_grid(N)'s rule
    (csrc/pgmg_gradient.hip), restated."""
    def grid(N):
        tiles = ((N - 1) // 2 + 255) // 256
        band = 64
        while band > 8 and tiles * ((N + band - 1) // band) < 1024:
            band //= 2
        return tiles, (N + band - 1) // band
    assert grid(5) == (1, 1) and grid(TWO_BANDS) == (1, 2)
    assert grid((TWO_TILES + 1) // 2)[0] == 1 and grid(TWO_TILES)[0] == 2


@pytest.mark.parametrize("N", SIZES)
def test_step_bitwise(pgmg, N):
    """out against the model for h positive and negative, nu = 0 and dt large and small; the frame
    of out is omega's words (+-0 and subnormals carried); vmax exactly the model's maximum; a call
    without vmax gives the same out; psi and omega are only read; the words beside the arrays
    stay."""
    import torch
    psi, w = _field(N, 0), _field(N, 1)
    (pt, pb), (wt, wb) = _guarded(psi), _guarded(w)
    ot, ob = _guarded(np.full((N, N), np.nan))
    for h, dt, nu in ((1.0 / (N - 1), 1e-3, 0.01), (-2.0 / (N - 1), 0.25, 0.0), (0.7 / (N - 1), 1e-5, 3.0)):
        want, wmax = vort_model.step(psi, w, h, dt, nu)
        what = f"N={N} h={h} dt={dt} nu={nu}"
        ot.fill_(np.nan)
        torch.cuda.synchronize()
        out, vmax = pgmg.ops.vorticity_step(pt, wt, ot, h, dt, nu, vmax=True)
        assert out is ot
        assert_bitwise(ot.cpu().numpy(), want, "step " + what)
        print(f"{what}: vmax {vmax!r} model {wmax!r}")
        assert _same_bits(vmax, wmax), (what, vmax, wmax)
        ot.fill_(np.nan)
        torch.cuda.synchronize()
        pgmg.ops.vorticity_step(pt, wt, ot, h, dt, nu)   # asynchronous
        torch.cuda.synchronize()
        assert_bitwise(ot.cpu().numpy(), want, "step without vmax " + what)
    keep = np.ones((N, N), dtype=bool)
    keep[1:-1, 1:-1] = False
    assert np.array_equal(bits(want)[keep], bits(w)[keep])
    assert_bitwise(pt.cpu().numpy(), psi, "psi is only read")
    assert_bitwise(wt.cpu().numpy(), w, "omega is only read")
    for b, name in ((pb, "psi"), (wb, "omega"), (ob, "out")):
        _guards_intact(b, f"{name} N={N}")
    pgmg.ops.release()


def test_step_special_values(pgmg):
    """NaN and Inf in psi and omega: out NaN exactly where the model has it and bitwise elsewhere;
    vmax skips the NaN terms as the model's fmax does."""
    import torch
    N, h, dt, nu = 65, 1.0 / 64, 1e-3, 0.01
    psi, w = np.array(_field(N, 0)), np.array(_field(N, 1))
    psi[10, 10], psi[30, 0], psi[40, 41] = np.nan, np.inf, 1e300
    w[20, 20], w[0, 5], w[50, 3] = np.nan, np.nan, -np.inf
    want, wmax = vort_model.step(psi, w, h, dt, nu)
    out, vmax = pgmg.ops.vorticity_step(_t(psi), _t(w), _t(np.zeros((N, N))), h, dt, nu, vmax=True)
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and 1 <= np.isnan(want).sum() < 64
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isinf(wmax) and _same_bits(vmax, wmax)
    psi[30, 0], psi[40, 41] = 0.0, 1.0
    want, wmax = vort_model.step(psi, w, h, dt, nu)
    vmax = pgmg.ops.vorticity_step(_t(psi), _t(w), _t(np.zeros((N, N))), h, dt, nu, vmax=True)[1]
    assert np.isfinite(wmax) and _same_bits(vmax, wmax)
    allnan = np.full((N, N), np.nan)
    assert pgmg.ops.vorticity_step(_t(allnan), _t(w), _t(np.zeros((N, N))), h, dt, nu, vmax=True)[1] == 0.0
    pgmg.ops.release()


@pytest.mark.parametrize("N", SIZES)
def test_wall_bitwise(pgmg, N):
    """Both modes, h positive and negative, against the model: the frame as the formulas give it,
    the corners +0.0, the interior of omega and all of psi untouched."""
    import torch
    psi, w = _field(N, 0), _field(N, 1)
    (pt, pb), (wt, wb) = _guarded(psi), _guarded(w)
    for h in (1.0 / (N - 1), -2.0 / (N - 1)):
        for free in (False, True):
            want = vort_model.wall(psi, w, h, WALLS, free)
            wt.copy_(_t(w))
            torch.cuda.synchronize()
            assert pgmg.ops.wall_vorticity(pt, wt, h, WALLS, free=free) is wt
            torch.cuda.synchronize()
            got = wt.cpu().numpy()
            assert_bitwise(got, want, f"wall N={N} h={h} free={free}")
            corners = np.array([got[0, 0], got[0, -1], got[-1, 0], got[-1, -1]])
            assert not bits(corners).any(), "the corners are +0.0"
    assert_bitwise(pt.cpu().numpy(), psi, "psi is only read")
    for b, name in ((pb, "psi"), (wb, "omega")):
        _guards_intact(b, f"{name} N={N}")


def test_streams(pgmg):
    import torch
    sa = torch.cuda.Stream()
    N, h, dt, nu = 257, 1.0 / 256, 1e-3, 0.01
    psi, w = _field(N, 0), _field(N, 1)
    pt, wt, ot = _t(psi), _t(w), _t(np.zeros((N, N)))
    torch.cuda.synchronize()
    ww = vort_model.wall(psi, w, h, WALLS)
    want, wmax = vort_model.step(psi, ww, h, dt, nu)
    pgmg.ops.wall_vorticity(pt, wt, h, WALLS, stream=sa.cuda_stream)
    vmax = pgmg.ops.vorticity_step(pt, wt, ot, h, dt, nu, vmax=True, stream=sa.cuda_stream)[1]
    assert _same_bits(vmax, wmax)
    pgmg.ops.release(sa.cuda_stream)
    assert_bitwise(ot.cpu().numpy(), want, "wall then step on a stream")
    pgmg.ops.release()


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    keep = [np.random.default_rng(k).standard_normal((N, N)) for k in range(3)]
    pt, wt, ot = (_t(a) for a in keep)
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pp, pw, po = (C.c_void_p(t.data_ptr()) for t in (pt, wt, ot))
    m = C.c_double(-7.0)
    host = np.zeros((N, N))
    ph = host.ctypes.data_as(C.c_void_p)
    good = (C.c_double * 4)(*WALLS)

    def step(psi=pp, w=pw, out=po, N=N, h=h, dt=1e-3, nu=0.01, vmax=True):
        return lib.pgmg_vorticity_grid(psi, w, out, N, h, dt, nu, C.byref(m) if vmax else None, None)

    def wall(psi=pp, w=pw, N=N, h=h, mode=0, walls=good):
        return lib.pgmg_wall_vorticity_grid(psi, w, N, h, mode, walls, None)

    for call in (step, wall):
        for bad in (0, 3, 4, 6, 10, 32, 34):
            assert call(N=bad) == ARG, bad
        for bad in (0.0, -0.0, float("nan"), float("inf")):
            assert call(h=bad) == ARG, bad
        assert call(psi=None) == ARG and call(w=None) == ARG
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        assert step(dt=bad) == ARG, bad
    for bad in (-1e-9, float("nan"), float("inf")):
        assert step(nu=bad) == ARG, bad
    assert step(out=None) == ARG
    assert step(out=pp) == ARG and step(out=pw) == ARG
    assert step(out=C.c_void_p(pt.data_ptr() + 8 * (N * N - 1))) == ARG   # one element shared
    assert step(out=ph) == ARG                                            # not device memory
    for bad in (-1, 2, 7):
        assert wall(mode=bad) == ARG, bad
    assert wall(walls=None) == ARG
    for k in range(4):
        for bad in (float("nan"), float("inf")):
            ws = list(WALLS)
            ws[k] = bad
            assert wall(walls=(C.c_double * 4)(*ws)) == ARG and wall(walls=(C.c_double * 4)(*ws), mode=1) == ARG
    assert wall(w=pp) == ARG                                              # in place on psi
    assert wall(w=ph) == ARG
    assert not host.any()
    torch.cuda.synchronize()
    assert m.value == -7.0
    for t, a, name in zip((pt, wt, ot), keep, ("psi", "omega", "out")):
        assert_bitwise(t.cpu().numpy(), a, name + " after refused calls")
    assert step() == pgmg.PGMG_OK and wall() == pgmg.PGMG_OK and step(vmax=False) == pgmg.PGMG_OK
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.vorticity_step(_t(np.zeros((6, 6))), _t(np.zeros((6, 6))), _t(np.zeros((6, 6))), 0.2, 1e-3, 0.0)
    pgmg.ops.release()
