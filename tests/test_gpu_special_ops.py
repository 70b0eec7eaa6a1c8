"""GPU: the op-level entries on IEEE special values, against the oracle (which
tests/test_oracle_special.py pins to the compiled reference on such words at N = 17 and 33).

Comparison: special_values.assert_bitwise_nan -- equal NaN masks, every other word bitwise equal,
so the sign of a zero, a subnormal and an Inf count.  Shapes: the ragged, several-tile ones of
tests/test_gpu_ops.py.  Four input classes, on and beside the places the kernels treat specially
(first / last interior row and column, both sides of the 512- and 480-column block edges, row-band
edges, the corners where a deferred row meets a deferred column, the caller's boundary):

  neg_zero  x = f = -0.0 everywhere: every norm is exactly 0 (a check fires at once with
            eps = 1e-7 and never with eps = 0), and -0 survives only where the reference keeps it
  sparse    +-0 and subnormals everywhere, a few point sources: every word of every tile edge is
            sign-of-zero sensitive
  big       +-(0.85 .. 1.7)e308 everywhere: sums overflow to +-Inf and Inf - Inf gives NaN in
            every tile; squares overflow, so no check fires
  seed      uniform(-1, 1) with NaN / +-Inf seeds at the special places (SEED_COLS x SEED_ROWS and
            the boundary): a NaN must spread exactly as the reference's does -- out of a discarded
            halo lane or a load past the grid it must not

The census of the ORACLE's result is asserted first (the class produced its special words).
"""
import ctypes as C

import numpy as np
import pytest

import damp_model
import special_values as sv

pytestmark = pytest.mark.gpu

SHAPES = [(5, 6), (9, 130), (129, 128), (257, 513), (64, 1030), (1031, 1537)]
CLASSES = ["neg_zero", "sparse", "big", "seed"]
# both sides of the single sweep's 512-column and the paired pass's 480-column block edges
SEED_COLS = (1, 2, 479, 480, 481, 511, 512, 513, 959, 960, 961, 1023, 1024, 1025)
# first / last interior rows and both sides of the power-of-two rows a band can end at
SEED_ROWS = (1, 2, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512)


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _one(rng, cls, H, W):
    if cls == "neg_zero":
        return np.full((H, W), -0.0)
    if cls == "sparse":
        a = np.where(rng.random((H, W)) < 0.5, 0.0, -0.0)
        k = rng.random((H, W))
        a = np.where(k < 0.02, rng.choice([1.0, -2.5, 0.375], (H, W)), a)
        a = np.where((k >= 0.02) & (k < 0.10),
                     rng.choice([5e-324, -5e-324, 3e-310, -1.5e-308, 2.2e-308], (H, W)), a)
        a[H // 2, W // 2] = 1.0              # at least one point source, whatever the shape
        return a
    if cls == "big":                         # two neighbours of one sign overflow
        return rng.uniform(0.5, 1.0, (H, W)) * rng.choice([-1.7e308, 1.7e308], (H, W))
    a = rng.uniform(-1.0, 1.0, (H, W))
    words = (np.nan, np.inf, -np.inf)
    n = 0
    for r in SEED_ROWS + (H - 3, H - 2):
        for c in SEED_COLS + (W - 3, W - 2):
            # a diagonal subset, so that the seeds stay sparse: their spread is what is compared
            if 1 <= r < H - 1 and 1 <= c < W - 1 and (r + c) % 3 == 0:
                a[r, c] = words[n % 3]
                n += 1
    a[0, W // 2] = np.nan                      # the caller's boundary
    a[H // 2, W - 1] = -np.inf
    a[H - 1, 1] = np.inf
    return a


def _inputs(cls, H, W, salt=0):
    rng = np.random.default_rng(H * 7919 + W + 1000003 * CLASSES.index(cls) + salt)
    return _one(rng, cls, H, W), _one(rng, cls, H, W)


def _census_ok(cls, ref, what):
    c = sv.census(ref)
    if cls == "neg_zero":
        assert c["nz"] >= 1, (what, c)
    elif cls == "sparse":
        assert c["nz"] >= 1 and c["sub"] >= 1, (what, c)
    elif cls == "big":                       # (a small grid may have turned every Inf into NaN)
        assert c["inf"] + c["nan"] >= 1, (what, c)
    else:
        assert c["nan"] >= 1, (what, c)
    return c


def _orc_smooth(oracle_mod, x, f, h, num_iter, eps):
    H, W = x.shape
    o = oracle_mod.Oracle(eps=eps)
    work = np.zeros(H * W)
    return oracle_mod.lib().orc_jacobi_smooth(C.byref(o.c), oracle_mod._p(x), oracle_mod._p(f), W,
                                              H, h, num_iter, oracle_mod._p(work))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_jacobi_special(pgmg, oracle_mod, H, W, cls):
    """In place, v = 0, 1, 2, 5; eps = -1 (no checks), 0.0 (checks that never fire) and 1e-7;
    the ping-pong buffer full of NaN; the sweep count is the oracle's."""
    import torch
    x0, f = _inputs(cls, H, W)
    h = 1.0 / (max(H, W) - 1)
    ft = _t(f)
    counts = set()
    for v in (0, 1, 2, 5):
        for eps in (-1.0, 0.0, 1e-7):
            what = f"jacobi {cls} {H}x{W} v={v} eps={eps}"
            x = x0.copy()
            n_ref = _orc_smooth(oracle_mod, x, f, h, v, eps)
            if v == 5:
                _census_ok(cls, x, what)
            xt = _t(x0)
            tmp = torch.full_like(xt, float("nan"))
            n = pgmg.ops.jacobi(xt, ft, h, v, eps=eps, tmp=tmp)
            assert n == n_ref, (what, n, n_ref)
            sv.assert_bitwise_nan(xt.cpu().numpy(), x, what)
            counts.add((v, eps, n_ref))
    if cls == "neg_zero":
        # a norm of exactly 0 fires at once unless eps is 0 (or negative)
        assert (5, 1e-7, 1) in counts and (5, 0.0, 6) in counts and (5, -1.0, 6) in counts, counts
    else:
        # NaN and Inf norms never fire; neither do the point sources' norms
        assert (5, 1e-7, 6) in counts, counts


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_residual_special(pgmg, oracle_mod, H, W, cls):
    import torch
    x, f = _inputs(cls, H, W, salt=1)
    h = 1.0 / (max(H, W) - 1)
    want = np.full((H, W), 3.25)             # the boundary of r is untouched
    ref = np.zeros((H, W))
    oracle_mod.lib().orc_residual(oracle_mod._p(ref), oracle_mod._p(x), oracle_mod._p(f), W, H, h)
    want[1:-1, 1:-1] = ref[1:-1, 1:-1]
    _census_ok(cls, want, f"residual {cls} {H}x{W}")
    r = torch.full((H, W), 3.25, dtype=torch.float64, device="cuda:0")
    pgmg.ops.residual(r, _t(x), _t(f), h)
    torch.cuda.synchronize()
    sv.assert_bitwise_nan(r.cpu().numpy(), want, f"residual {cls} {H}x{W}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("Nf", [5, 9, 17, 129, 1025])
def test_restrict_special(pgmg, oracle_mod, Nf, cls):
    import torch
    fine, _ = _inputs(cls, Nf, Nf, salt=2)
    Nc = (Nf - 1) // 2 + 1
    want = np.full((Nc, Nc), -2.5)           # the coarse boundary is untouched
    ref = oracle_mod.restrict(fine)
    want[1:-1, 1:-1] = ref[1:-1, 1:-1]
    if Nf >= 129:
        _census_ok(cls, want, f"restrict {cls} {Nf}")
    c = torch.full((Nc, Nc), -2.5, dtype=torch.float64, device="cuda:0")
    pgmg.ops.restrict(_t(fine), c)
    torch.cuda.synchronize()
    sv.assert_bitwise_nan(c.cpu().numpy(), want, f"restrict {cls} {Nf}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("Nf", [5, 9, 17, 129, 1025])
def test_prolong_reference_special(pgmg, oracle_mod, Nf, cls):
    """fine += P coarse: -0 + -0 stays -0, -0 + +0 is +0, and the uncorrected fine row and
    column 1 keep the caller's words."""
    Nc = (Nf - 1) // 2 + 1
    fine, _ = _inputs(cls, Nf, Nf, salt=3)
    coarse, _ = _inputs(cls, Nc, Nc, salt=4)
    want = oracle_mod.prolong(fine, coarse)
    if Nf >= 17:
        _census_ok(cls, want, f"prolong {cls} {Nf}")
    ft = _t(fine)
    pgmg.ops.prolong(_t(coarse), ft, mode=pgmg.PGMG_PROLONG_REFERENCE)
    sv.assert_bitwise_nan(ft.cpu().numpy(), want, f"prolong {cls} {Nf}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("Nf,nt", [(5, 0), (17, 0), (17, 4), (129, 0), (1025, 0), (1025, 32),
                                   (513, 1000)])
def test_prolong_symmetric_special(pgmg, oracle_mod, Nf, nt, cls):
    Nc = (Nf - 1) // 2 + 1
    fine, _ = _inputs(cls, Nf, Nf, salt=5)
    coarse, _ = _inputs(cls, Nc, Nc, salt=6)
    want = oracle_mod.prolong_sym(fine, coarse, num_thread=nt if nt else None)
    if Nf >= 17:
        _census_ok(cls, want, f"prolong_sym {cls} {Nf}")
    ft = _t(fine)
    pgmg.ops.prolong(_t(coarse), ft, mode=pgmg.PGMG_PROLONG_SYMMETRIC, num_thread=nt)
    sv.assert_bitwise_nan(ft.cpu().numpy(), want, f"prolong_sym {cls} {Nf} nt={nt}")


def _norm_cases():
    n = 70001                                # several workgroups, not a multiple of anything
    rng = np.random.default_rng(11)
    base = rng.uniform(-1.0, 1.0, n)
    out = {"zeros": np.zeros(n), "neg_zeros": np.full(n, -0.0)}
    for name, word, into in (("one_subnormal", 5e-324, "zeros"), ("tiny_squares", 1e-170, "zeros"),
                             ("one_1e200", 1e200, "base"), ("all_1e200", 1e200, None),
                             ("one_nan", np.nan, "base"), ("last_nan", np.nan, "base"),
                             ("one_inf", -np.inf, "base"), ("inf_and_nan", np.inf, "base")):
        a = np.zeros(n) if into == "zeros" else base.copy() if into == "base" else np.full(n, word)
        a[n - 1 if name == "last_nan" else n // 3] = word
        if name == "inf_and_nan":
            a[5] = np.nan
        out[name] = a
    out["ordinary"] = base
    return out


@pytest.mark.parametrize("name", sorted(_norm_cases()))
def test_norm_special(pgmg, oracle_mod, name):
    """pgmg_norm equals the oracle's norm of the same array wherever that is 0, Inf or NaN (a
    subnormal's square underflows to 0, 1e200's overflows to Inf); otherwise within the existing
    tolerance (tests/test_gpu_parity.py: 1e-13 relative, the two summation orders)."""
    import math
    a = _norm_cases()[name]
    want = oracle_mod.norm(a)
    expect = {"zeros": 0.0, "neg_zeros": 0.0, "one_subnormal": 0.0, "tiny_squares": 0.0,
              "one_1e200": math.inf, "all_1e200": math.inf, "one_inf": math.inf,
              "one_nan": math.nan, "last_nan": math.nan, "inf_and_nan": math.nan}
    if name in expect:                       # the oracle's own value is what the case is about
        assert want == expect[name] or (math.isnan(want) and math.isnan(expect[name])), (name, want)
    got = pgmg.ops.norm(_t(a))
    print(f"norm {name}: got {got!r} want {want!r}")
    if math.isnan(want):
        assert math.isnan(got), (name, got)
    elif want == 0.0 or math.isinf(want):
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (name, got, want)
    else:
        assert abs(got - want) <= 1e-13 * want, (name, got, want)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("N", [5, 9, 129, 513, 1025])
def test_damp_special(pgmg, oracle_mod, N, cls):
    """pgmg_damp_grid: the update bitwise tests/damp_model.py's under the contract, the norm the
    model's (the oracle's sequential residual norm) exactly where that is 0, Inf or NaN and
    within solve_rule.norm_tol otherwise; the boundary is the caller's."""
    import math
    import solve_rule
    x, f = _inputs(cls, N, N, salt=7)
    h = 1.0 / (N - 1)
    for omega in (0.5, 1.0):
        what = f"damp {cls} N={N} omega={omega}"
        want, want_norm = damp_model.damp(x, f, h, omega)
        if N >= 129:
            _census_ok(cls, want, what)
        xt = _t(x)
        got_norm = pgmg.ops.damp(xt, _t(f), h, omega)
        print(f"{what}: norm {got_norm!r} model {want_norm!r}")
        sv.assert_bitwise_nan(xt.cpu().numpy(), want, what)
        if math.isnan(want_norm):
            assert math.isnan(got_norm), (what, got_norm)
        elif want_norm == 0.0 or math.isinf(want_norm):
            assert got_norm == want_norm, (what, got_norm, want_norm)
        else:
            assert solve_rule.close(got_norm, want_norm, N), (what, got_norm, want_norm)
    assert pgmg.load().pgmg_ops_release(None) == pgmg.PGMG_OK
