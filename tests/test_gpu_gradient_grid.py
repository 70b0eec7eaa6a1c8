"""GPU: pgmg_gradient_grid (include/pgmg.h "Gradient of the solution", on caller-owned arrays)
through ops.gradient, bitwise against tests/grad_model.gradient.

k_gradient gives a lane a column pair, a wave 128 columns and a workgroup 512, and marches bands
of 8 .. 64 rows.  The sizes: 5 (every point one-sided at order 4; one wave, two lanes), 9, 17, 33
and 65 (one wave, partly filled: the last pair's lane has inactive lanes to its right), 129 (one
wave exactly: 64 pairs), 257 (two waves: lanes 0 and 63 load their halo pairs), 513 (256 pairs:
exactly one workgroup in x), 1025 (two workgroups in x, 129 bands).  The arrays have the odd pitch
N, so every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grad_model
import special_values as sv
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 17, 33, 65, 129, 257, 513, 1025]
ORDERS = [2, 4]
SCALES = [1.0, -1.0, 0.37]


def _hs(N):
    return [1.0 / (N - 1), 0.7 / (N - 1), -2.0 / (N - 1)]


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _phi(N):
    a = np.random.default_rng(5000 + N).standard_normal((N, N))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(N, order, h, scale):
    gx, gy = grad_model.gradient(_phi(N), h, order, scale)
    gx.setflags(write=False)
    gy.setflags(write=False)
    return gx, gy, grad_model.norm(gx, gy)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", SIZES)
def test_gradient_bitwise(pgmg, N, order):
    import torch
    pt = _t(_phi(N))
    gx, gy = torch.empty_like(pt), torch.empty_like(pt)
    for h in _hs(N):
        for scale in SCALES:
            wx, wy, wn = _want(N, order, h, scale)
            gx.fill_(np.nan)
            gy.fill_(np.nan)
            torch.cuda.synchronize()
            _, _, n = pgmg.ops.gradient(pt, h, gx, gy, order=order, scale=scale, norm=True)
            what = f"N={N} order={order} h={h} scale={scale}"
            assert_bitwise(gx.cpu().numpy(), wx, "gx " + what)
            assert_bitwise(gy.cpu().numpy(), wy, "gy " + what)
            print(f"{what}: norm {n!r} model {wn!r}")
            assert abs(n - wn) <= N * N * 2.0 ** -52 * wn, (what, n, wn)
    assert_bitwise(pt.cpu().numpy(), _phi(N), "phi is only read")
    pgmg.ops.release()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [5, 65, 257])
def test_one_component_and_async(pgmg, N, order):
    """gx=None or gy=None: the other component has the same bits and the norm is its own; without
    a norm the call is asynchronous and allocates its outputs."""
    import torch
    h, scale = 0.7 / (N - 1), 0.37
    wx, wy, _ = _want(N, order, h, scale)
    pt = _t(_phi(N))
    g = torch.empty_like(pt)
    a, b, n = pgmg.ops.gradient(pt, h, gx=g, order=order, scale=scale, norm=True)
    assert a is g and b is None
    assert_bitwise(g.cpu().numpy(), wx, "gx alone")
    assert abs(n - grad_model.norm(wx, None)) <= N * N * 2.0 ** -52 * n
    a, b, n = pgmg.ops.gradient(pt, h, gy=g, order=order, scale=scale, norm=True)
    assert a is None and b is g
    assert_bitwise(g.cpu().numpy(), wy, "gy alone")
    assert abs(n - grad_model.norm(None, wy)) <= N * N * 2.0 ** -52 * n
    gx, gy = pgmg.ops.gradient(pt, h, order=order, scale=scale)
    torch.cuda.synchronize()
    assert_bitwise(gx.cpu().numpy(), wx, "gx, no norm")
    assert_bitwise(gy.cpu().numpy(), wy, "gy, no norm")
    pgmg.ops.release()


def _special(N=65):
    a = np.random.default_rng(78).standard_normal((N, N))
    # the frame: -0, +0, a subnormal, Inf and NaN
    a[0, 2], a[0, 3], a[-1, 5], a[6, 0], a[7, -1] = -0.0, 0.0, 5e-324, np.inf, np.nan
    a[0, 0], a[-1, -1], a[-1, 30], a[40, 0] = -0.0, -np.inf, np.inf, 1e-310
    # a patch of zeros of both signs with period 4: differences of +0 and -0
    a[8:20, 8:20] = 0.0
    a[8:20, 10:20:4] = a[8:20, 11:20:4] = -0.0
    a[10:20:4, 8:20] = -0.0
    # a patch at the subnormal scale: subnormal differences, subnormal results
    a[24:34, 40:56] = _phi(65)[24:34, 40:56] * 1e-310
    # Inf - Inf inside a stencil (two apart along x, then along y), a lone Inf, a NaN
    a[44, 20], a[44, 22] = np.inf, np.inf
    a[50, 40], a[52, 40] = -np.inf, -np.inf
    a[58, 10] = np.inf
    a[36, 60] = np.nan
    # overflow inside the one-sided corner formulas
    a[1, 1], a[-2, -2] = 1e308, -1e308
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("order", ORDERS)
def test_special_values(pgmg, order):
    """+-0, subnormals, +-Inf and NaN in the frame and the interior: NaN exactly where the model
    has it, every other word bitwise the model's; then a grid of -0.0 and a subnormal-scale one."""
    import torch
    N = 65
    phi = _special(N)
    for h, scale in ((1.0 / 64, 1.0), (-2.0 / 64, 0.37), (0.7 / 64, -1.0)):
        wx, wy = grad_model.gradient(phi, h, order, scale)
        for w in (wx, wy):
            c = sv.census(w)
            print(f"order {order} h {h} scale {scale}: census of the model's result {c}")
            assert c["nz"] >= 1 and c["sub"] >= 1 and 1 <= c["nan"] <= 0.25 * w.size, c
            assert np.count_nonzero(w == np.inf) >= 1 and np.count_nonzero(w == -np.inf) >= 1
        pt = _t(phi)
        gx, gy = pgmg.ops.gradient(pt, h, order=order, scale=scale)
        torch.cuda.synchronize()
        sv.assert_bitwise_nan(gx.cpu().numpy(), wx, "gx special words")
        sv.assert_bitwise_nan(gy.cpu().numpy(), wy, "gy special words")
        sv.assert_bitwise_nan(pt.cpu().numpy(), np.array(phi), "phi is only read")
    for phi, what in ((np.full((N, N), -0.0), "negative zeros"),
                      (_phi(N) * 1e-310, "subnormal scale")):
        for scale in (1.0, -1.0):
            wx, wy = grad_model.gradient(phi, 1.0 / 64, order, scale)
            gx, gy = pgmg.ops.gradient(_t(phi), 1.0 / 64, order=order, scale=scale)
            torch.cuda.synchronize()
            assert_bitwise(gx.cpu().numpy(), wx, f"gx {what} scale {scale}")
            assert_bitwise(gy.cpu().numpy(), wy, f"gy {what} scale {scale}")
    assert sv.census(wx)["sub"] >= 1000
    pgmg.ops.release()


def test_norm_same_bits_twice_and_on_two_streams(pgmg):
    import torch
    N, order, h = 257, 4, 1.0 / 256
    pt = _t(_phi(N))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    norms = [pgmg.ops.gradient(pt, h, order=order, norm=True)[2] for _ in range(2)]
    norms.append(pgmg.ops.gradient(pt, h, order=order, norm=True, stream=sa.cuda_stream)[2])
    norms.append(pgmg.ops.gradient(pt, h, order=order, norm=True, stream=sb.cuda_stream)[2])
    print(norms)
    assert len({bits(np.array([n]))[0] for n in norms}) == 1, norms
    for s in (None, sa.cuda_stream, sb.cuda_stream):
        pgmg.ops.release(s)


def test_two_streams_then_release(pgmg):
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    Na, Nb = 257, 129
    ha, hb = 1.0 / (Na - 1), 0.7 / (Nb - 1)
    pa, pb = _t(_phi(Na)), _t(_phi(Nb))
    torch.cuda.synchronize()
    ax, ay = pgmg.ops.gradient(pa, ha, order=4, stream=sa.cuda_stream)
    bx, by = pgmg.ops.gradient(pb, hb, order=2, scale=-1.0, stream=sb.cuda_stream)
    pgmg.ops.release(sa.cuda_stream)
    pgmg.ops.release(sb.cuda_stream)
    assert_bitwise(ax.cpu().numpy(), _want(Na, 4, ha, 1.0)[0], "stream a gx")
    assert_bitwise(ay.cpu().numpy(), _want(Na, 4, ha, 1.0)[1], "stream a gy")
    assert_bitwise(bx.cpu().numpy(), _want(Nb, 2, hb, -1.0)[0], "stream b gx")
    assert_bitwise(by.cpu().numpy(), _want(Nb, 2, hb, -1.0)[1], "stream b gy")
    # a set released and used again allocates a fresh one
    bx, by, n = pgmg.ops.gradient(pb, hb, order=2, scale=-1.0, stream=sb.cuda_stream, norm=True)
    pgmg.ops.release(sb.cuda_stream)
    assert_bitwise(by.cpu().numpy(), _want(Nb, 2, hb, -1.0)[1], "stream b again")
    wn = _want(Nb, 2, hb, -1.0)[2]
    assert abs(n - wn) <= Nb * Nb * 2.0 ** -52 * wn


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    phi = _phi(N)
    keep = np.random.default_rng(1).standard_normal((N, N))
    pt, gx, gy = _t(phi), _t(keep), _t(keep)
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pp, px, py = (C.c_void_p(t.data_ptr()) for t in (pt, gx, gy))
    n = C.c_double(-7.0)

    def call(phi=pp, gx=px, gy=py, N=N, h=h, order=4, scale=1.0):
        return lib.pgmg_gradient_grid(phi, gx, gy, N, h, order, scale, C.byref(n), None)

    assert call() == pgmg.PGMG_OK
    gx.copy_(_t(keep))
    gy.copy_(_t(keep))
    torch.cuda.synchronize()
    n.value = -7.0
    for bad in (0, 3, 4, 6, 10, 32, 34):
        assert call(N=bad) == ARG, bad
    for bad in (1, 3, 6):
        assert call(order=bad) == ARG, bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(scale=bad) == ARG, bad
    for bad in (0.0, -0.0, float("nan"), float("inf")):
        assert call(h=bad) == ARG, bad
    assert call(phi=None) == ARG
    assert call(gx=None, gy=None) == ARG
    assert call(gy=px) == ARG                                    # the same array twice
    assert call(gy=C.c_void_p(gx.data_ptr() + 8 * (N * N - 1))) == ARG   # one element shared
    assert call(gx=pp) == ARG and call(gy=pp, gx=None) == ARG    # an output that is phi
    host = np.zeros((N, N))
    assert call(gx=host.ctypes.data_as(C.c_void_p)) == ARG       # not device memory
    assert not host.any()
    torch.cuda.synchronize()
    assert n.value == -7.0
    assert_bitwise(pt.cpu().numpy(), phi, "phi after refused calls")
    assert_bitwise(gx.cpu().numpy(), keep, "gx after refused calls")
    assert_bitwise(gy.cpu().numpy(), keep, "gy after refused calls")
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.gradient(_t(np.zeros((6, 6))), 0.2)
    pgmg.ops.release()
