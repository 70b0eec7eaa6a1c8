"""GPU: pgmg_divergence_grid and pgmg_gradient_add_grid (include/pgmg.h "Projection", on
caller-owned arrays) through ops.divergence and ops.gradient_add, bitwise against
tests/proj_model.py.

Both kernels have k_gradient's shape: a lane owns a column pair, a wave 128 columns, a workgroup
512, bands of 8 .. 64 rows.  The sizes: 5 (every column and row one-sided at order 4), 9, 17, 33
(several 8-row bands), 129 (64 pairs: exactly one wave), 257 (a second wave: lanes 0 and 63 load
their halo pairs), 513 (256 pairs: one full workgroup tile), 1025 (two tiles in x).  Every input
is also given transposed, which swaps the stencil that meets each edge.  The arrays have the odd
pitch N, so every pair is an unaligned 16-byte access.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import proj_model
import special_values as sv
from conftest import assert_bitwise, bits

pytestmark = pytest.mark.gpu

SIZES = [5, 9, 17, 33, 129, 257, 513, 1025]
ORDERS = [2, 4]
SCALES = [1.0, -1.0, 0.37]
CANARY = 1234.5


def _hs(N):
    return [0.7 / (N - 1), -2.0 / (N - 1)]


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _field(N, which, transposed=False):
    a = np.random.default_rng(7000 + 10 * N + which).standard_normal((N, N))
    if transposed:
        a = np.ascontiguousarray(a.T)
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


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", SIZES)
def test_divergence_bitwise(pgmg, N, order):
    """out against the model for every h and scale, plain and transposed inputs; the norm within
    N^2 2^-52 of the model's; a norm-only call gives the same norm bit for bit and writes
    nothing; the words beside out, u and v stay."""
    import torch
    for tr in (False, True):
        u, v = _field(N, 0, tr), _field(N, 1, tr)
        (ut, ub), (vt, vb) = _guarded(u), _guarded(v)
        ot, ob = _guarded(np.full((N, N), np.nan))
        for h in _hs(N):
            for scale in SCALES:
                want = proj_model.divergence(u, v, h, order, scale)
                wn = proj_model.norm(want)
                ot.fill_(np.nan)
                torch.cuda.synchronize()
                out, n = pgmg.ops.divergence(ut, vt, h, ot, order=order, scale=scale, norm=True)
                what = f"N={N} order={order} h={h} scale={scale} transposed={tr}"
                assert out is ot
                assert_bitwise(ot.cpu().numpy(), want, "divergence " + what)
                print(f"{what}: norm {n!r} model {wn!r}")
                assert abs(n - wn) <= N * N * 2.0 ** -52 * wn, (what, n, wn)
                ot.fill_(CANARY)
                torch.cuda.synchronize()
                none, n2 = pgmg.ops.divergence(ut, vt, h, None, order=order, scale=scale, norm=True)
                assert none is None and bits(np.array([n2]))[0] == bits(np.array([n]))[0], (what, n, n2)
                assert np.all(ot.cpu().numpy() == CANARY), what + ": a norm-only call wrote"
                got = pgmg.ops.divergence(ut, vt, h, order=order, scale=scale)   # asynchronous
                torch.cuda.synchronize()
                assert_bitwise(got.cpu().numpy(), want, "allocated out " + what)
        assert_bitwise(ut.cpu().numpy(), u, "u is only read")
        assert_bitwise(vt.cpu().numpy(), v, "v is only read")
        for b, name in ((ub, "u"), (vb, "v"), (ob, "out")):
            _guards_intact(b, f"{name} N={N} order={order}")
    pgmg.ops.release()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", SIZES)
def test_gradient_add_bitwise(pgmg, N, order):
    """u += gx, v += gy in place against the model; u=None or v=None leaves the other array's
    words as they were; phi is only read; the words beside u, v and phi stay."""
    import torch
    for tr in (False, True):
        u, v, phi = _field(N, 0, tr), _field(N, 1, tr), _field(N, 2, tr)
        (ut, ub), (vt, vb), (pt, pb) = _guarded(u), _guarded(v), _guarded(phi)
        for h in _hs(N):
            for scale in SCALES:
                wu, wv = proj_model.gradient_add(phi, h, u, v, order, scale)
                what = f"N={N} order={order} h={h} scale={scale} transposed={tr}"
                ut.copy_(_t(u))
                vt.copy_(_t(v))
                torch.cuda.synchronize()
                pgmg.ops.gradient_add(pt, h, ut, vt, order=order, scale=scale)
                torch.cuda.synchronize()
                assert_bitwise(ut.cpu().numpy(), wu, "u " + what)
                assert_bitwise(vt.cpu().numpy(), wv, "v " + what)
        # one component alone (the last h and scale): the other array keeps its words
        ut.copy_(_t(u))
        vt.copy_(_t(v))
        torch.cuda.synchronize()
        pgmg.ops.gradient_add(pt, h, u=ut, order=order, scale=scale)
        torch.cuda.synchronize()
        assert_bitwise(ut.cpu().numpy(), wu, "u alone")
        assert_bitwise(vt.cpu().numpy(), v, "v with v=None")
        ut.copy_(_t(u))
        torch.cuda.synchronize()
        pgmg.ops.gradient_add(pt, h, v=vt, order=order, scale=scale)
        torch.cuda.synchronize()
        assert_bitwise(vt.cpu().numpy(), wv, "v alone")
        assert_bitwise(ut.cpu().numpy(), u, "u with u=None")
        assert_bitwise(pt.cpu().numpy(), phi, "phi is only read")
        for b, name in ((ub, "u"), (vb, "v"), (pb, "phi")):
            _guards_intact(b, f"{name} N={N} order={order}")
    pgmg.ops.release()


def test_gradient_add_padded_phi(pgmg):
    """pitch_phi > N (the context passes its padded level-0 grid): the same bits."""
    import torch
    N, P, order, h, scale = 257, 272, 4, 0.7 / 256, -1.0
    u, v, phi = _field(N, 0), _field(N, 1), _field(N, 2)
    wu, wv = proj_model.gradient_add(phi, h, u, v, order, scale)
    pad = torch.full((N, P), np.nan, dtype=torch.float64, device="cuda:0")
    pad[:, :N] = _t(phi)
    ut, vt = _t(u), _t(v)
    torch.cuda.synchronize()
    lib = pgmg.load()
    rc = lib.pgmg_gradient_add_grid(C.c_void_p(pad.data_ptr()), P, C.c_void_p(ut.data_ptr()),
                                    C.c_void_p(vt.data_ptr()), N, h, order, scale, None)
    assert rc == pgmg.PGMG_OK
    torch.cuda.synchronize()
    assert_bitwise(ut.cpu().numpy(), wu, "u from a padded phi")
    assert_bitwise(vt.cpu().numpy(), wv, "v from a padded phi")


def _special(N=65, seed=78):
    """tests/test_gpu_gradient_grid.py's fixture: +-0, subnormals, +-Inf and NaN in the frame and
    the interior"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N, N))
    a[0, 2], a[0, 3], a[-1, 5], a[6, 0], a[7, -1] = -0.0, 0.0, 5e-324, np.inf, np.nan
    a[0, 0], a[-1, -1], a[-1, 30], a[40, 0] = -0.0, -np.inf, np.inf, 1e-310
    a[8:20, 8:20] = 0.0
    a[8:20, 10:20:4] = a[8:20, 11:20:4] = -0.0
    a[10:20:4, 8:20] = -0.0
    a[24:34, 40:56] = rng.standard_normal((10, 16)) * 1e-310
    a[44, 20], a[44, 22] = np.inf, np.inf
    a[50, 40], a[52, 40] = -np.inf, -np.inf
    a[58, 10] = np.inf
    a[36, 60] = np.nan
    a[1, 1], a[-2, -2] = 1e308, -1e308
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("order", ORDERS)
def test_special_values(pgmg, order):
    """NaN exactly where the model has it, every other word bitwise the model's."""
    import torch
    N = 65
    u, v, phi = _special(N, 78), _special(N, 79), _special(N, 80)
    for h, scale in ((1.0 / 64, 1.0), (-2.0 / 64, 0.37), (0.7 / 64, -1.0)):
        want = proj_model.divergence(u, v, h, order, scale)
        c = sv.census(want)
        print(f"order {order} h {h} scale {scale}: census of the model's divergence {c}")
        assert c["sub"] >= 1 and 1 <= c["nan"] <= 0.25 * want.size, c
        assert np.count_nonzero(want == np.inf) >= 1 and np.count_nonzero(want == -np.inf) >= 1
        ut, vt = _t(u), _t(v)
        got = pgmg.ops.divergence(ut, vt, h, order=order, scale=scale)
        torch.cuda.synchronize()
        sv.assert_bitwise_nan(got.cpu().numpy(), want, "divergence special words")
        wu, wv = proj_model.gradient_add(phi, h, u, v, order, scale)
        pgmg.ops.gradient_add(_t(phi), h, ut, vt, order=order, scale=scale)
        torch.cuda.synchronize()
        sv.assert_bitwise_nan(ut.cpu().numpy(), wu, "u special words")
        sv.assert_bitwise_nan(vt.cpu().numpy(), wv, "v special words")
    for a, what in ((np.full((N, N), -0.0), "negative zeros"),
                    (_field(129, 0)[:N, :N] * 1e-310, "subnormal scale")):
        for scale in (1.0, -1.0):
            want = proj_model.divergence(a, a.T, 1.0 / 64, order, scale)
            got = pgmg.ops.divergence(_t(a), _t(a.T), 1.0 / 64, order=order, scale=scale)
            torch.cuda.synchronize()
            assert_bitwise(got.cpu().numpy(), want, f"divergence {what} scale {scale}")
    assert sv.census(want)["sub"] >= 1000
    pgmg.ops.release()


def test_streams_and_release(pgmg):
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    N, order, h = 257, 4, 0.7 / 256
    u, v, phi = _field(N, 0), _field(N, 1), _field(N, 2)
    ut, vt, pt = _t(u), _t(v), _t(phi)
    want = proj_model.divergence(u, v, h, order, 1.0)
    wu, wv = proj_model.gradient_add(phi, h, u, v, 2, -1.0)
    torch.cuda.synchronize()
    out, na = pgmg.ops.divergence(ut, vt, h, order=order, norm=True, stream=sa.cuda_stream)
    assert out is None
    outb = pgmg.ops.divergence(ut, vt, h, order=order, stream=sb.cuda_stream)
    n0 = pgmg.ops.divergence(ut, vt, h, order=order, norm=True)[1]
    assert bits(np.array([na]))[0] == bits(np.array([n0]))[0], (na, n0)
    pgmg.ops.release(sb.cuda_stream)
    assert_bitwise(outb.cpu().numpy(), want, "stream b")
    pgmg.ops.gradient_add(pt, h, ut, vt, order=2, scale=-1.0, stream=sa.cuda_stream)
    pgmg.ops.release(sa.cuda_stream)
    assert_bitwise(ut.cpu().numpy(), wu, "u on stream a")
    assert_bitwise(vt.cpu().numpy(), wv, "v on stream a")
    # a set released and used again allocates a fresh one
    n1 = pgmg.ops.divergence(_t(u), _t(v), h, order=order, norm=True, stream=sa.cuda_stream)[1]
    assert bits(np.array([n1]))[0] == bits(np.array([n0]))[0]
    for s in (None, sa.cuda_stream):
        pgmg.ops.release(s)


def test_argument_errors_touch_nothing(pgmg):
    import torch
    N = 33
    h = 1.0 / (N - 1)
    keep = [np.random.default_rng(k).standard_normal((N, N)) for k in range(4)]
    ut, vt, ot, pt = (_t(a) for a in keep)
    torch.cuda.synchronize()
    lib = pgmg.load()
    ARG = pgmg.PGMG_ERR_ARG
    pu, pv, po, pp = (C.c_void_p(t.data_ptr()) for t in (ut, vt, ot, pt))
    n = C.c_double(-7.0)
    host = np.zeros((N, N))
    ph = host.ctypes.data_as(C.c_void_p)

    def div(u=pu, v=pv, out=po, N=N, h=h, order=4, scale=1.0, norm=True):
        return lib.pgmg_divergence_grid(u, v, out, N, h, order, scale, C.byref(n) if norm else None,
                                        None)

    def add(phi=pp, pitch=N, u=pu, v=pv, N=N, h=h, order=4, scale=1.0):
        return lib.pgmg_gradient_add_grid(phi, pitch, u, v, N, h, order, scale, None)

    for call in (div, add):
        for bad in (0, 3, 4, 6, 10, 32, 34):
            assert call(N=bad) == ARG, bad
        for bad in (1, 3, 6):
            assert call(order=bad) == ARG, bad
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(scale=bad) == ARG, bad
        for bad in (0.0, -0.0, float("nan"), float("inf")):
            assert call(h=bad) == ARG, bad
    assert div(u=None) == ARG and div(v=None) == ARG
    assert div(out=None, norm=False) == ARG
    assert div(out=pu) == ARG and div(out=pv) == ARG
    assert div(out=C.c_void_p(ut.data_ptr() + 8 * (N * N - 1))) == ARG   # one element shared
    assert div(out=ph) == ARG                                            # not device memory
    assert add(phi=None) == ARG and add(pitch=N - 1) == ARG
    assert add(u=None, v=None) == ARG
    assert add(v=pu) == ARG                                              # the same array twice
    assert add(u=pp) == ARG and add(v=pp, u=None) == ARG                 # an output that is phi
    assert add(u=ph) == ARG
    assert not host.any()
    torch.cuda.synchronize()
    assert n.value == -7.0
    for t, a, name in zip((ut, vt, ot, pt), keep, ("u", "v", "out", "phi")):
        assert_bitwise(t.cpu().numpy(), a, name + " after refused calls")
    assert div() == pgmg.PGMG_OK and add() == pgmg.PGMG_OK
    with pytest.raises(pgmg.PgmgError):
        pgmg.ops.divergence(_t(np.zeros((6, 6))), _t(np.zeros((6, 6))), 0.2)
    pgmg.ops.release()
