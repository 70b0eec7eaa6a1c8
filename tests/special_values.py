"""IEEE special values for the tests: input families, a census, and the one comparison.

The contract (include/pgmg.h, "Special values"): for any input words, every output word the
reference leaves non-NaN is bitwise the reference's -- sign of zero, subnormals and +-Inf
included -- and a word is NaN exactly where the reference's is.  A NaN's sign and payload are
unspecified (x86 and CDNA produce different default NaNs and a compiler may commute operands),
so a grid that holds a NaN is compared with assert_bitwise_nan and hashed with canon_hash, never
with pgmg_solution_hash.

A plain module like solve_rule.py (no fixtures).  Used by tests/test_oracle_special.py (CPU: the
oracle against the compiled reference on these inputs), tests/test_gpu_special_ops.py and
tests/test_gpu_special_cycles.py (GPU: the library against the oracle) and by
tests/golden/make_golden.py --special-only.
"""
import numpy as np

import oracle

# f = s * analytic f: small enough that r^2 underflows to 0 and phi holds subnormals (tiny),
# large enough that r^2 overflows to Inf while every grid word stays finite (huge)
SCALE = {("tiny", "f64"): 1e-305, ("tiny", "f32"): 1e-36,
         ("huge", "f64"): 1e305, ("huge", "f32"): 1e36}

FAMILIES = ("neg_zero", "point_source", "tiny", "huge", "nan_f", "inf_phi", "nan_frame")
# what the oracle's result must hold before a comparison with it means anything
FLOOR = {"neg_zero": "nz", "tiny": "sub", "nan_f": "nonfinite", "inf_phi": "nonfinite",
         "nan_frame": "nonfinite", "nan_corner": "nonfinite"}

# doubles that fp32 cannot hold: a subnormal, one below half the least subnormal (rounds to -0),
# one just above FLT_MAX and one far above (both +Inf), 0.1 (inexact), a NaN, ties to even on both
# sides (1 + 2^-24 rounds down to 1, 1 + 3 * 2^-24 rounds up to 1 + 2^-22) and the negated set
ABI_F32_WORDS = (1e-40, -1e-46, 3.5e38, 1e39, 0.1, float("nan"), 1.0 + 2.0 ** -24,
                 1.0 + 3 * 2.0 ** -24, -1e-40, 1e-46, -3.5e38, -0.1, 0.0, -0.0)




def reference_cases():
    """(kind, N, family, n_coarse, alpha, eps) of the cycles recorded from the compiled reference
    (tests/golden/special_cycles.npz, two cycles each).  n_coarse 5 is the reference's default, 17
    a shallow hierarchy (one level at N = 17).  The reference's coarsest solve is 10 sweeps, so at
    N <= 65 one NaN floods the grid within a cycle; the two-level N = 257 / n_coarse = 129 cases
    are there so that each NaN family also has a cycle under the 25 % cap."""
    cases = []
    for kind in ("V", "W"):
        for N in (17, 33, 65):
            for fam in FAMILIES:
                cases.append((kind, N, fam, 5, 3, 1e-7))
                cases.append((kind, N, fam, 17, 2 if kind == "W" else 3, 1e-7))
            cases.append((kind, N, "neg_zero", 5, 3, 0.0))     # no check fires
        for fam in ("nan_f", "inf_phi", "nan_frame"):
            cases.append((kind, 257, fam, 129, 2 if kind == "W" else 3, 1e-7))
    return cases


def np_dtype(dtype):
    return np.float32 if dtype in ("f32", np.float32) else np.float64


def _uint(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def census(a, dtype=None):
    """{"nz", "sub", "inf", "nan"}: the counts of -0, subnormal, +-Inf and NaN words of `a` taken
    in element type `dtype` (default: the array's own; a float64 array that holds fp32 values is
    counted as fp32 with dtype="f32")."""
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.astype(np_dtype(dtype))
    tiny = np.finfo(a.dtype).tiny
    fin = np.isfinite(a)
    return {"nz": int(np.count_nonzero((a == 0) & np.signbit(a))),
            "sub": int(np.count_nonzero(fin & (a != 0) & (np.abs(a) < tiny))),
            "inf": int(np.count_nonzero(np.isinf(a))),
            "nan": int(np.count_nonzero(np.isnan(a)))}


def assert_bitwise_nan(got, want, what=""):
    """got equals want under the special-value contract: the same NaN mask, every other word
    bitwise equal.  Both arrays in one element type (float64, or both float32)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype,
                                                                  got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    gb, wb = _uint(got), _uint(want)
    bad = (gn != wn) | (~wn & (gb != wb))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        w = 8 if gb.dtype == np.uint32 else 16
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} words differ ({int((gn != wn).sum())} in the "
            f"NaN mask: {int(gn.sum())} NaN got, {int(wn.sum())} wanted); first at {i}: "
            f"got {got[i]!r} = 0x{int(gb[i]):0{w}x}, want {want[i]!r} = 0x{int(wb[i]):0{w}x}")


CANON_NAN = 0x7FF8000000000000


def canon_hash(a):
    """FNV-64 of the float64 words of `a` (the golden fixtures' hash, oracle.fnv_hash) with every
    NaN word replaced by CANON_NAN: comparable between machines whatever their NaNs look like."""
    w = np.ascontiguousarray(a, dtype=np.float64).copy()
    nan = np.isnan(w)
    w.view(np.uint64)[nan] = CANON_NAN
    return oracle.fnv_hash(w)


def analytic_f(N, dtype="f64"):
    return oracle.Oracle(dtype=dtype).rhs(N)


def family(name, N, dtype="f64"):
    """(phi0, f) of the named family as N x N arrays of `dtype`'s element type.  f is None where
    the family's right-hand side is the analytic one unchanged (the library can then regenerate
    it in-kernel); analytic_f(N, dtype) is that f."""
    dt = np_dtype(dtype)
    key = "f32" if dt is np.float32 else "f64"
    phi0 = np.zeros((N, N), dtype=dt)
    a, b = N // 3, 2 * N // 3
    if name == "neg_zero":
        return np.full((N, N), -0.0, dtype=dt), np.full((N, N), -0.0, dtype=dt)
    if name == "point_source":
        f = np.zeros((N, N), dtype=dt)
        f[a, b] = -1.0
        f[min(N // 2 + 1, N - 2), max(N // 4, 1)] = 3.0
        # a patch of -0.0 (up to 4 x 4) in the quadrant the sources leave alone
        f[b:min(b + 4, N - 1), b:min(b + 4, N - 1)] = -0.0
        return phi0, f
    if name in ("tiny", "huge"):
        return phi0, (analytic_f(N, dtype) * dt(SCALE[name, key])).astype(dt)
    if name == "nan_f":
        f = analytic_f(N, dtype)
        f[a, b] = np.nan
        return phi0, f
    if name == "inf_phi":
        phi0[b, a] = np.inf
        return phi0, None
    if name == "nan_frame":
        phi0[0, a] = np.nan
        phi0[b, N - 1] = -np.inf
        return phi0, None
    if name == "nan_corner":
        # not in FAMILIES: the four corners of phi, which no stencil of the reference reads
        phi0[0, 0], phi0[0, N - 1], phi0[N - 1, 0], phi0[N - 1, N - 1] = np.nan, -np.inf, np.inf, np.nan
        return phi0, None
    raise KeyError(name)


def abi_f32(N, finite_interior=False):
    """(phi0, f) of float64 words that fp32 cannot hold (ABI_F32_WORDS, repeated over the grid,
    frame included; f starts at another word so the two arrays differ).  finite_interior: the
    interior takes only the words that stay finite in fp32, so that a cycle on the problem
    leaves finite words to compare; the frame keeps them all."""
    w = np.array(ABI_F32_WORDS)
    k = np.arange(N * N)
    out = [w[k % len(w)].reshape(N, N).copy(), w[(k + 5) % len(w)].reshape(N, N).copy()]
    if finite_interior:
        fin = w[np.isfinite(w) & (np.abs(w) < 3e38)]
        for a, shift in zip(out, (0, 3)):
            a[1:-1, 1:-1] = fin[(k + shift) % len(fin)].reshape(N, N)[1:-1, 1:-1]
    return out[0], out[1]


def check_floor(name, ref, dtype="f64"):
    """The census floor of family `name` on the ORACLE's result `ref` (never the GPU's): a
    comparison with a result that holds no special word would pass vacuously."""
    c = census(ref, dtype)
    N = ref.shape[0]
    kind = FLOOR.get(name)
    if kind == "nz":
        assert c["nz"] >= N, (name, N, c)
    elif kind == "sub":
        assert c["sub"] >= 100, (name, N, c)
    elif kind == "nonfinite":
        assert c["inf"] + c["nan"] >= 1, (name, N, c)
        assert c["nan"] <= 0.25 * ref.size, (name, N, c)
    return c


def run_oracle(kind, name, N, calls, dtype="f64", eps=1e-7, phi0_f=None, **okw):
    """The oracle through `calls` (a list of cycle counts) of kind V / W / F on family `name`:
    [(phi as float64, sweeps, cut_exits) after every call].  phi is read-only (shared)."""
    o = oracle.Oracle(eps=eps, dtype=dtype, **okw)
    phi0, f = family(name, N, dtype) if phi0_f is None else phi0_f
    f = analytic_f(N, dtype) if f is None else np.ascontiguousarray(f, dtype=o.dt)
    phi = np.array(phi0, dtype=o.dt)
    step = {"V": o.v_cycle, "W": o.v_cycle if okw.get("alpha", 3) == 1 else o.w_cycle}.get(kind)
    out = []
    for n in calls:
        for _ in range(n):
            if kind == "F":
                o.f_cycle_outer(phi)
            else:
                step(phi, f)
        snap = phi.astype(np.float64)
        snap.setflags(write=False)
        out.append((snap, o.sweeps, o.cut_exits))
    return out
