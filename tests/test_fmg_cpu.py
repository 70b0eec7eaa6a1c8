"""CPU: the model of pgmg_fmg (tests/fmg_model.py) — checkpoints, cubic exactness, fp32, and
the accuracy table that motivates cubic interpolation with nu = 2.

rel_error is ||phi - u|| / ||u|| as orc_rel_error computes it; "disc", the discretisation
error, is the same quantity after 40 oracle V-cycles from zero (converged to round-off).
Measured with this model (fp64, analytic f, eps 1e-7):

    N     disc      cubic nu=2   cubic nu=1   bilinear nu=2   bilinear nu=1
    33    8.04e-4   0.90 x disc  0.97         1.64            11.7
    129   5.02e-5   0.90         2.09         3.10            28.7
    257   1.25e-5   0.90         2.80         4.28            43.0
    513   3.14e-6   0.90         3.66         5.95            63.3

Bilinear interpolation's ratio grows with N (FMG theory for a second-order discretisation
asks for an interpolation order above 2); cubic with two V-cycles per level stays at 0.90.
"""
import numpy as np
import pytest

import fmg_model


@pytest.mark.parametrize("N,want_hash,sweeps,rel", [(9, "71ac910439e8ae23", 52, None),
                                                    (33, "d94fa278a609fc8b", 136, 7.2556e-4)])
def test_model_checkpoints(oracle_mod, N, want_hash, sweeps, rel):
    u, o = fmg_model.fmg_analytic(N, nu=2, eps=1e-7)
    assert oracle_mod.fnv_hash(u) == want_hash
    assert (o.sweeps, o.early_exits) == (sweeps, 0)
    if rel is not None:
        assert abs(o.rel_error(u) / rel - 1.0) < 1e-4, o.rel_error(u)


def test_cubic_reproduces_cubics_exactly():
    """(x^3 - 2x)(1 + y^3) from a 9 x 9 to a 17 x 17 grid on [0, 1]^2: max error 0.0 (the
    one-sided formulas at positions 1 and Nf-2 are cubic too)."""
    g = lambda X, Y: (X ** 3 - 2 * X) * (1 + Y ** 3)   # noqa: E731
    xc, xf = np.linspace(0, 1, 9), np.linspace(0, 1, 17)
    Xc, Yc = np.meshgrid(xc, xc)
    Xf, Yf = np.meshgrid(xf, xf)
    fine = fmg_model.cubic(g(Xc, Yc))
    assert fine.shape == (17, 17)
    assert np.max(np.abs(fine - g(Xf, Yf))) == 0.0


def test_cubic_copies_even_points_and_is_x_then_y():
    rng = np.random.default_rng(3)
    c = rng.standard_normal((7, 7))
    fine = fmg_model.cubic(c)
    assert np.array_equal(fine[0::2, 0::2], c)
    # x first on the coarse rows, then y: the even fine rows are the x-interpolated rows
    assert np.array_equal(fine[0::2, :], fmg_model._interp_rows(c))


def test_model_fp32_is_float32_throughout(oracle_mod):
    u, o = fmg_model.fmg_analytic(33, dtype="f32")
    assert u.dtype == np.float32 and o.dt is np.float32
    c = np.linspace(0, 1, 25, dtype=np.float32).reshape(5, 5)
    assert fmg_model.cubic(c).dtype == np.float32
    # within fp32 round-off of the fp64 model, not equal to it
    u64, _ = fmg_model.fmg_analytic(33)
    d = np.linalg.norm(u.astype(np.float64) - u64) / np.linalg.norm(u64)
    assert 0.0 < d < 1e-5, d


def _disc(oracle_mod, N):
    phi, o = oracle_mod.run_cycles("V", N, 40)
    return o.rel_error(phi)


@pytest.fixture(scope="module")
def table(oracle_mod):
    out = {}
    for N in (33, 129, 257):
        disc = _disc(oracle_mod, N)
        u, o = fmg_model.fmg_analytic(N, nu=2)
        out[N] = {"disc": disc, "cubic2": o.rel_error(u) / disc}
    for N in (33, 257):
        u, o = fmg_model.fmg_analytic(N, nu=2, interp="bilinear")
        out[N]["bilinear2"] = o.rel_error(u) / out[N]["disc"]
    return out


@pytest.mark.parametrize("N", [33, 129, 257])
def test_cubic_nu2_reaches_discretisation_error(table, N):
    print(N, table[N])
    assert table[N]["cubic2"] <= 1.0, table[N]


def test_bilinear_ratio_grows_with_n(table):
    """Why the interpolation is cubic: bilinear FMG falls behind the discretisation error as
    the grid grows (1.64 x at 33, 4.28 x at 257)."""
    print(table[33], table[257])
    assert table[257]["bilinear2"] > table[33]["bilinear2"]
    assert table[257]["bilinear2"] > 1.0
