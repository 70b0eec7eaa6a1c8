"""GPU: pgmg_batch_cycle / pgmg_batch_solve (include/pgmg.h "Batched small problems") against
tests/batch_model.py, per problem.  Every comparison of phi is bitwise, frame included; cycle
counts, check counts and stop reasons are the model's; norms agree with the model's sequential
sums within solve_rule.norm_tol(N).

The sizes are every N the entries take (each has its own path through the tail's code: 5 is the
coarsest solve alone, 9 and 17 the wave-team levels, 33 and 65 the register-row smoothers), and
batch sizes of one, a few, more than the card's 256 CUs (a CU runs a second workgroup over the
LDS the first one left) and, at N = 33, where a CU's LDS has room for four workgroups, two and
six hundred.
"""
import functools

import numpy as np
import pytest

import batch_model
import solve_rule
from conftest import assert_bitwise
from solve_rule import NONFINITE, close

pytestmark = pytest.mark.gpu


def _np_dt(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _dev(arrs, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(arrs), dtype=_np_dt(dtype))).cuda()


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _problem(N, seed, dtype="f64", frame=False):
    """(f, phi0): the robustness right-hand side of `seed` and a random start (seeded); with
    frame=True phi0's Dirichlet frame is random too, otherwise +0."""
    dt = _np_dt(dtype)
    rng = np.random.default_rng(1000 * N + seed)
    phi0 = rng.uniform(-1.0, 1.0, (N, N)).astype(dt)
    if not frame:
        phi0[0, :] = phi0[-1, :] = phi0[:, 0] = phi0[:, -1] = 0
    return batch_model.mt(N, seed, dtype), _ro(phi0)


@functools.lru_cache(maxsize=None)
def _cycle_model(N, seed, kind, n, dtype="f64", eps=1e-7, h=None, frame=False, cfg=()):
    f, phi0 = _problem(N, seed, dtype, frame)
    m = batch_model.cycle(N, f, phi0, kind, n, dtype, eps, h, **dict(cfg))
    _ro(m.phi)
    return m


def _run_cycle(pgmg, N, seeds, kind, n, dtype="f64", eps=1e-7, h=None, frame=False, cfg=()):
    """n cycles of the problems `seeds` in one batch; every problem against its model."""
    kw = dict(cfg)
    if h is not None:
        kw["h"] = h
    bs = pgmg.BatchSolver(N, dtype=dtype, eps=eps, **kw)
    probs = [_problem(N, s, dtype, frame) for s in seeds]
    phi = _dev([p for _, p in probs], dtype)
    f = _dev([ff for ff, _ in probs], dtype)
    sw, ex = bs.cycle(phi, f, n=n, kind=kind, stats=True)
    got, sw, ex = phi.cpu().numpy(), sw.cpu().numpy(), ex.cpu().numpy()
    assert_bitwise(f.cpu().numpy(), np.stack([ff for ff, _ in probs]), "f is read only")
    for b, s in enumerate(seeds):
        m = _cycle_model(N, s, kind, n, dtype, eps, h, frame, cfg)
        what = f"N={N} {kind} n={n} B={len(seeds)} problem {b} {dict(cfg)}"
        assert_bitwise(got[b], m.phi, what)
        assert (int(sw[b]), int(ex[b])) == (m.sweeps, m.exits), what
    return got, sw, ex


SEEDS7 = (12345, 1, 2, 3, 4, 5, 6)


@pytest.mark.parametrize("kind,alpha", [("V", 3), ("W", 3), ("W", 2)])
@pytest.mark.parametrize("N", [5, 9, 17, 33, 65])
def test_cycle_bitwise(pgmg, oracle_mod, N, kind, alpha):
    cfg = (("alpha", alpha),)
    for n in (1, 3):
        _run_cycle(pgmg, N, SEEDS7[:1], kind, n, cfg=cfg)
        got, sw, ex = _run_cycle(pgmg, N, SEEDS7, kind, n, cfg=cfg)
        # the same problem through a context
        f, phi0 = _problem(N, SEEDS7[0])
        with pgmg.Solver(N, alpha=alpha) as s:
            s.set_problem(phi0, f)
            (s.vcycle if kind == "V" else s.wcycle)(n)
            assert_bitwise(s.solution(), got[0], f"Solver N={N} {kind} alpha={alpha} n={n}")
            assert s.stats() == (int(sw[0]), int(ex[0]))


@pytest.mark.parametrize("N,cfg,h,eps", [
    (33, (("n_coarse", 9),), None, 1e-7),
    (65, (("n_coarse", 17),), None, 1e-7),
    (33, (("coarse_iter", 0),), None, 1e-7),
    (65, (("v1", 2), ("v2", 3)), None, 1e-7),
    (33, (), "0.7", 1e-7),
    (65, (), None, -1.0),
], ids=["n_coarse9", "n_coarse17", "coarse_iter0", "v2_3", "h0.7", "eps_never"])
def test_cycle_off_defaults(pgmg, oracle_mod, N, cfg, h, eps):
    h = 0.7 / (N - 1) if h == "0.7" else None
    for kind in ("V", "W"):
        _, _, ex = _run_cycle(pgmg, N, SEEDS7[:3], kind, 2, eps=eps, h=h, cfg=cfg)
        if eps < 0:
            assert not ex.any()


def test_cycle_default_eps_exits_fire(pgmg, oracle_mod):
    """W-cycles of the analytic right-hand side: the coarse smoothers stop early from the first
    cycle on (39 early exits in four cycles on the CPU)."""
    N = 33
    o = oracle_mod.Oracle()
    f = o.rhs(N)
    phi = np.zeros((N, N))
    for _ in range(4):
        o.w_cycle(phi, f)
    assert o.cut_exits > 20
    bs = pgmg.BatchSolver(N)
    dphi, df = _dev([np.zeros((N, N))] * 2, "f64"), _dev([f, f], "f64")
    sw, ex = bs.cycle(dphi, df, n=4, kind="W", stats=True)
    got = dphi.cpu().numpy()
    for b in range(2):
        assert_bitwise(got[b], phi, f"problem {b}")
        assert (int(sw[b]), int(ex[b])) == (o.sweeps, o.cut_exits)


@pytest.mark.parametrize("N", [9, 65])
def test_cycle_fp32(pgmg, oracle_mod, N):
    for kind in ("V", "W"):
        _run_cycle(pgmg, N, SEEDS7[:3], kind, 2, dtype="f32")


def test_cycle_keeps_a_random_frame(pgmg, oracle_mod):
    for N in (9, 65):
        got, _, _ = _run_cycle(pgmg, N, SEEDS7[:2], "V", 2, frame=True)
        for b, s in enumerate(SEEDS7[:2]):
            phi0 = _problem(N, s, "f64", True)[1]
            mask = np.ones((N, N), dtype=bool)
            mask[1:-1, 1:-1] = False
            assert_bitwise(got[b][mask], phi0[mask], f"frame N={N} problem {b}")
            assert np.count_nonzero(phi0[mask]) > 3 * N


# ---- solve mode ---------------------------------------------------------------------------------

def _solve_batch(pgmg, c, problems, history=True):
    """The batch `problems` [(f, phi0)] under case c's configuration and rule, on the device:
    (phi, namespace of numpy results)."""
    bs = pgmg.BatchSolver(c.N, dtype=c.dtype, **c.cfg)
    phi = _dev([p for _, p in problems], c.dtype)
    f = _dev([ff for ff, _ in problems], c.dtype)
    r = bs.solve(phi, f, damp=c.omega, kind=c.kind, history=history, **c.rule)
    out = {k: v.cpu().numpy() for k, v in vars(r).items()}
    return phi.cpu().numpy(), out


def _check_problem(got_phi, out, b, m, N, what):
    print(f"{what}: cycles {out['cycles'][b]} (model {m.cycles}) reason {out['reason'][b]} "
          f"res {out['res'][b]!r} (model {m.norms[-1]!r})")
    assert (int(out["cycles"][b]), int(out["checks"][b]), int(out["reason"][b])) == \
        (m.cycles, m.checks, m.reason), what
    assert_bitwise(got_phi[b], m.phi, what)
    assert close(float(out["res0"][b]), m.norms[0], N), (what, out["res0"][b], m.norms[0])
    assert close(float(out["res"][b]), m.norms[-1], N), (what, out["res"][b], m.norms[-1])
    assert (int(out["sweeps"][b]), int(out["exits"][b])) == (m.sweeps, m.exits), what
    if "history" in out:
        hist = out["history"][b]
        for i, r in enumerate(m.norms):
            assert close(float(hist[i]), r, N), (what, i, hist[i], r)
        assert np.isnan(hist[len(m.norms):]).all(), what
        assert hist[0] == out["res0"][b] and hist[len(m.norms) - 1] == out["res"][b]


@pytest.mark.parametrize("name", sorted(batch_model.SOLVE_CASES))
def test_solve_mixed_batch(pgmg, oracle_mod, name):
    c = batch_model.solve_case(name)
    got, out = _solve_batch(pgmg, c, c.problems)
    for b, m in enumerate(c.models):
        _check_problem(got, out, b, m, c.N, f"{name} problem {b}")
    assert out["history"].shape == (len(c.problems), c.rule["max_cycles"] + 1)


def test_solve_without_outputs(pgmg, oracle_mod):
    """Every result array is optional (a NULL out): phi is the same."""
    import ctypes as C
    import torch
    from importlib import import_module
    capi = import_module("pgmg_amd._capi")
    c = batch_model.solve_case("damped17")
    bs = pgmg.BatchSolver(c.N)
    phi = _dev([p for _, p in c.problems], "f64")
    f = _dev([ff for ff, _ in c.problems], "f64")
    o = capi.PgmgSolveOpts()
    pgmg.check(pgmg.load().pgmg_solve_opts_default(C.byref(o)))
    o.rtol, o.atol, o.max_cycles = c.rule["rtol"], c.rule["atol"], c.rule["max_cycles"]
    pgmg.check(pgmg.load().pgmg_batch_solve(C.byref(bs.cfg), C.byref(o), c.omega,
                                            C.c_void_p(phi.data_ptr()), C.c_void_p(f.data_ptr()),
                                            len(c.problems), None, None), "pgmg_batch_solve")
    torch.cuda.synchronize()
    got = phi.cpu().numpy()
    for b, m in enumerate(c.models):
        assert_bitwise(got[b], m.phi, f"problem {b}")


def test_permuted_batch_same_bits(pgmg, oracle_mod):
    c = batch_model.solve_case("damped65")
    got, out = _solve_batch(pgmg, c, c.problems)
    perm = [7, 2, 10, 0, 5, 9, 1, 8, 3, 6, 4]
    got2, out2 = _solve_batch(pgmg, c, [c.problems[p] for p in perm])
    for b, p in enumerate(perm):
        assert_bitwise(got2[b], got[p], f"slot {b} = problem {p}")
        for k in ("res0", "res"):
            assert out2[k][b].tobytes() == out[k][p].tobytes(), (k, b, p)
        assert out2["history"][b].tobytes() == out["history"][p].tobytes(), (b, p)
        assert (out2["cycles"][b], out2["reason"][b]) == (out["cycles"][p], out["reason"][p])


def _tiled(pgmg, c, idx, B):
    """B problems, problem b = c.problems[idx[b % len(idx)]]; each against its model and, for the
    norms, bit for bit against the first copy."""
    probs = [c.problems[idx[b % len(idx)]] for b in range(B)]
    got, out = _solve_batch(pgmg, c, probs)
    k = len(idx)
    for b in range(B):
        m = c.models[idx[b % k]]
        if b < k:
            _check_problem(got, out, b, m, c.N, f"B={B} problem {b}")
        else:   # (the full comparison once per distinct problem; the copies against the first)
            assert (got[b].view(np.uint64) == got[b % k].view(np.uint64)).all(), (B, b)
            for key in ("cycles", "checks", "reason", "sweeps", "exits"):
                assert out[key][b] == out[key][b % k], (key, b)
            for key in ("res0", "res", "history"):
                assert out[key][b].tobytes() == out[key][b % k].tobytes(), (key, b)


def test_more_problems_than_cus(pgmg, oracle_mod):
    """B = 300 at N = 65: with 256 CUs some CU runs a second workgroup over stale LDS."""
    _tiled(pgmg, batch_model.solve_case("damped65"), [0, 1, 2, 8, 9, 10], 300)


@pytest.mark.parametrize("B", [2, 600])
def test_shared_cu_at_33(pgmg, oracle_mod, B):
    """B = 2 and B = 600 at N = 33, where the LDS of a CU holds more than one workgroup."""
    _tiled(pgmg, batch_model.solve_case("damped33"), [0, 1, 2, 8, 9, 10], B)


def test_nan_problem_is_isolated(pgmg, oracle_mod):
    c = batch_model.solve_case("damped17")
    N = c.N
    fbad = np.array(c.problems[0][0])
    fbad[N // 2, N // 3] = np.nan
    bad = (fbad, c.problems[0][1])
    mbad = batch_model.solve(N, fbad, bad[1], c.kind, c.omega, c.dtype, cfg=c.cfg, **c.rule)
    assert mbad.reason == NONFINITE and mbad.cycles == 0
    probs = [c.problems[0], bad, c.problems[2], c.problems[3]]
    got, out = _solve_batch(pgmg, c, probs)
    for b, m in ((0, c.models[0]), (2, c.models[2]), (3, c.models[3])):
        _check_problem(got, out, b, m, N, f"neighbour {b}")
    assert (int(out["cycles"][1]), int(out["checks"][1]), int(out["reason"][1])) == (0, 1, NONFINITE)
    assert np.isnan(out["res"][1]) and np.isnan(out["res0"][1]) and np.isnan(out["history"][1]).all()
    nan_got, nan_want = np.isnan(got[1]), np.isnan(mbad.phi)
    assert nan_want.any() and (nan_got == nan_want).all()
    assert_bitwise(np.where(nan_got, 0.0, got[1]), np.where(nan_want, 0.0, mbad.phi), "NaN problem")


def test_solve_keeps_a_random_frame(pgmg, oracle_mod):
    c = batch_model.solve_case("damped17")
    N = c.N
    f, phi0 = _problem(N, 7, "f64", True)
    m = batch_model.solve(N, f, phi0, c.kind, c.omega, c.dtype, cfg=c.cfg, **c.rule)
    got, out = _solve_batch(pgmg, c, [c.problems[0], (f, phi0)])
    _check_problem(got, out, 1, m, N, "framed problem")
    mask = np.ones((N, N), dtype=bool)
    mask[1:-1, 1:-1] = False
    assert_bitwise(got[1][mask], phi0[mask], "frame")


def test_wrapper_refuses_other_layouts(pgmg):
    import torch
    bs = pgmg.BatchSolver(9)
    ok = torch.zeros((2, 9, 9), dtype=torch.float64, device="cuda")
    for bad in (torch.zeros((2, 9, 9), dtype=torch.float32, device="cuda"),
                torch.zeros((2, 9, 10), dtype=torch.float64, device="cuda"),
                torch.zeros((9, 9), dtype=torch.float64, device="cuda"),
                torch.zeros((3, 9, 9), dtype=torch.float64, device="cuda"),
                torch.zeros((2, 9, 18), dtype=torch.float64, device="cuda")[:, :, ::2]):
        with pytest.raises(pgmg.PgmgError):
            bs.cycle(bad, ok)
        with pytest.raises(pgmg.PgmgError):
            bs.solve(ok, bad)
    with pytest.raises(pgmg.PgmgError):
        pgmg.BatchSolver(9, dtype="f32").cycle(ok, ok)
