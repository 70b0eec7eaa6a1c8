"""CPU: the oracle (oracle/pgmg_oracle.c) against the compiled reference on IEEE special values.

tests/golden/special_ops.npz and special_cycles.npz hold what the reference's own code
(oracle/_ref/ref_harness, modes O and P; tests/golden/make_golden.py --special-only) computes on
inputs made of signed zeros, subnormals, +-1e308, NaN and Inf: the op-level entries at N = 17 and
33, and two V- and W-cycles at N = 17, 33 and 65 on every family of tests/special_values.py, with
the reference's default n_coarse = 5 and with n_coarse = 17.  The oracle must reproduce them under
the special-value contract (special_values.assert_bitwise_nan: equal NaN masks, every other word
bitwise equal, so the sign of a zero counts), with equal sweep and exit counts.  The GPU tests
then hold the library to the oracle on the same families.

Every case first meets a census floor on the ORACLE's result (special_values.check_floor), so no
comparison passes on a grid without special words.  Two floors cannot hold at every size the
cases cover, and there the case asserts what the size allows:
  - the NaN cap of 25 %: the reference's coarsest solve is 10 sweeps, so at N <= 65 one NaN
    floods 52 - 94 % of the grid within a cycle whatever n_coarse is.  Those cases assert the
    non-finite floor and pin the NaN mask; the two-level cases at N = 257 / n_coarse = 129 stay
    under the cap (asserted per case and, per family and cycle kind, by the last test);
  - 100 subnormal words for `tiny`: every check fires at once (r^2 underflows to 0), so the
    small and the deep hierarchies see few sweeps and end with 1 - 56 subnormal words.  Those
    cases assert at least one; the cases in TINY_100 (V and W) assert the 100.

coarse_iter is the literal 10 in the reference (MultiGrid.hpp:61, :100), so the shallow
hierarchies with coarse_iter = 0 that the GPU locality tests use rest on the oracle alone.
"""
import numpy as np
import pytest

import special_values as sv
from conftest import GOLDEN

@pytest.fixture(scope="module")
def ops_z():
    return np.load(GOLDEN / "special_ops.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def cyc_z():
    return np.load(GOLDEN / "special_cycles.npz", allow_pickle=False)


@pytest.mark.parametrize("which", ["sparse", "big", "seed"])
@pytest.mark.parametrize("N", [17, 33])
def test_special_ops(oracle_mod, ops_z, N, which):
    t = f"N{N}_{which}_"
    x, f, e = ops_z[t + "x"], ops_z[t + "f"], ops_z[t + "e"]
    h, eps = 1.0 / (N - 1), 1e-7
    got = {"residual": oracle_mod.residual(x, f, h), "restrict": oracle_mod.restrict(x),
           "prolong": oracle_mod.prolong(x, e)}
    for it, key in ((1, "smooth1"), (10, "smooth10")):
        o = oracle_mod.Oracle(eps=eps)
        s = x.copy()
        o.smooth(s, f, h, it)
        got[key] = s
    seen = {"nz": 0, "sub": 0, "inf": 0, "nan": 0}
    for key, g in got.items():
        want = ops_z[t + key]
        sv.assert_bitwise_nan(g, want, f"{key} N={N} {which}")
        for k, v in sv.census(want).items():
            seen[k] += v
    # the inputs discriminate: the reference's outputs hold what the family is about
    if which == "sparse":
        assert seen["nz"] >= 4 and seen["sub"] >= 2, seen
    elif which == "big":
        assert seen["inf"] >= 1, seen
    else:
        assert seen["nan"] >= 5 and seen["inf"] >= 1, seen


_cases = sv.reference_cases
# `tiny`: the cases whose grids are large and shallow enough to end with 100 subnormal words
TINY_100 = {("V", 33, 17), ("V", 65, 5), ("V", 65, 17), ("W", 65, 17)}


@pytest.mark.parametrize("kind,N,fam,nc,alpha,eps", _cases())
def test_special_cycles(oracle_mod, cyc_z, kind, N, fam, nc, alpha, eps):
    t = f"{kind}_{N}_{fam}_nc{nc}_a{alpha}_eps{eps:g}_"
    assert t + "sweeps" in cyc_z.files, "regenerate: make_golden.py --special-only"
    cycles = len(cyc_z[t + "sweeps"])
    o = oracle_mod.Oracle(eps=eps, n_coarse=nc, alpha=alpha)
    phi0, f = sv.family(fam, N)
    f = sv.analytic_f(N) if f is None else f
    phi = phi0.copy()
    most = {"nz": 0, "sub": 0, "inf": 0, "nan": 0}
    for k in range(cycles):
        (o.v_cycle if kind == "V" else o.w_cycle)(phi, f)
        tag = f"{t} cycle {k + 1}"
        c = sv.census(phi)
        assert [c[n] for n in ("nz", "sub", "inf", "nan")] == list(cyc_z[t + "census"][k]), tag
        assert int(sv.canon_hash(phi), 16) == int(cyc_z[t + "hash"][k]), tag
        assert o.sweeps == cyc_z[t + "sweeps"][k], tag
        assert o.early_exits == cyc_z[t + "exits"][k], tag
        # the floor, on the oracle's own result
        most = {n: max(most[n], c[n]) for n in c}
        if sv.FLOOR.get(fam) == "nonfinite":
            assert c["inf"] + c["nan"] >= 1, (tag, c)
            if N == 257 and k == 0:     # the two-level cases: under the NaN cap by construction
                sv.check_floor(fam, phi)
        elif fam == "neg_zero":
            sv.check_floor(fam, phi)
    if fam == "tiny":
        assert most["sub"] >= (100 if (kind, N, nc) in TINY_100 else 1), (t, most)
    if t + "phi" in cyc_z.files:
        sv.assert_bitwise_nan(phi, cyc_z[t + "phi"], t)


def test_special_cycles_nan_families_have_cases_under_the_cap(cyc_z):
    """Each NaN / Inf family has, for V and for W, a recorded cycle whose NaN share is at most
    25 % (the reference's census, which test_special_cycles holds the oracle to), so the reference
    pins finite words next to a NaN region too."""
    under = set()
    for kind, N, fam, nc, alpha, eps in _cases():
        if sv.FLOOR.get(fam) != "nonfinite":
            continue
        for row in cyc_z[f"{kind}_{N}_{fam}_nc{nc}_a{alpha}_eps{eps:g}_census"]:
            if row[2] + row[3] >= 1 and row[3] <= 0.25 * N * N:
                under.add((kind, fam))
    want = {(k, f) for k in "VW" for f in ("nan_f", "inf_phi", "nan_frame")}
    assert under >= want, want - under
