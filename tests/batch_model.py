"""The model of pgmg_batch_cycle and pgmg_batch_solve (include/pgmg.h "Batched small problems"),
per problem, over the CPU oracle; and the batches the GPU tests run, so that the CPU tests can
check the model's own input conditions on them.  Not a test module.

cycle():  n oracle cycles of one problem.
solve():  omega > 0: damp_model.solve_damped at the batch's mesh width; omega == 0:
          solve_rule.simulate over oracle cycles from phi0 with the oracle's sequential norms.
Both return a namespace with phi, cycles, reason, checks, norms (one per check), sweeps, exits
(also as cut_exits: the oracle's count, what pgmg_stats counts) and margin (the smallest
relative margin of any comparison the stop rule made; inf in cycle mode).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import damp_model
import oracle
import solve_rule

SEEDS = (12345, 1, 2, 3)
CFG_KEYS = ("alpha", "n_coarse", "coarse_iter", "v1", "v2")


def _dt(dtype):
    return np.float32 if dtype in ("f32", np.float32) else np.float64


def _ro(a):
    a.setflags(write=False)
    return a


def cycle(N, f, phi0=None, kind="V", n=1, dtype="f64", eps=1e-7, h=None, **cfg):
    o = oracle.Oracle(eps=eps, dtype=dtype, **cfg)
    h = 1.0 / (N - 1) if h is None else h
    ff = np.ascontiguousarray(f, dtype=o.dt)
    phi = np.zeros((N, N), dtype=o.dt) if phi0 is None else np.array(phi0, dtype=o.dt, order="C")
    step = o.v_cycle if kind == "V" or o.c.alpha == 1 else o.w_cycle
    for _ in range(n):
        step(phi, ff, h)
    return SimpleNamespace(phi=phi, cycles=n, reason=0, checks=0, norms=[], sweeps=o.sweeps,
                           exits=o.cut_exits, cut_exits=o.cut_exits, margin=math.inf)


def solve(N, f, phi0=None, kind="V", omega=0.5, dtype="f64", eps=1e-7, h=None, cfg=None, **rule):
    cfg = dict(cfg or {})
    h = 1.0 / (N - 1) if h is None else h
    if omega > 0:
        m = damp_model.solve_damped(N, f, phi0, kind, omega, dtype, eps, h0=h, **cfg, **rule)
        return SimpleNamespace(phi=m.phi, cycles=m.cycles, reason=m.reason, checks=m.checks,
                               norms=[r for _, r, _ in m.history], sweeps=m.sweeps, exits=m.exits,
                               cut_exits=m.exits, margin=m.margin)
    o = oracle.Oracle(eps=eps, dtype=dtype, **cfg)
    ff = np.ascontiguousarray(f, dtype=o.dt)
    st = SimpleNamespace(phi=np.zeros((N, N), dtype=o.dt) if phi0 is None
                         else np.array(phi0, dtype=o.dt, order="C"), k=0)
    step = o.v_cycle if kind == "V" or o.c.alpha == 1 else o.w_cycle

    def res_at(i, k):
        while st.k < k:
            step(st.phi, ff, h)
            st.k += 1
        return solve_rule.oracle_res_norm(oracle, st.phi, ff, dtype, h)

    cycles, reason, recs, margin = solve_rule.simulate(res_at, **rule)
    return SimpleNamespace(phi=st.phi, cycles=cycles, reason=reason, checks=len(recs),
                           norms=[r for _, r in recs], sweeps=o.sweeps, exits=o.cut_exits,
                           cut_exits=o.cut_exits, margin=margin)


# ---- the batches of tests/test_gpu_batch.py's solve tests -------------------------------------

@functools.lru_cache(maxsize=None)
def mt(N, seed, dtype="f64"):
    return _ro(np.ascontiguousarray(oracle.rhs_mt64(N, seed), dtype=_dt(dtype)))


def fnorm(f):
    return float(np.sqrt((np.asarray(f, dtype=np.float64) ** 2).sum()))


# name -> (N, dtype, kind, omega, cfg, rule without atol, atol as a factor of ||f_seed12345||)
SOLVE_CASES = {
    "damped17": (17, "f64", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12), 1e-6),
    "damped65": (65, "f64", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12), 1e-6),
    "damped33": (33, "f64", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12), 1e-6),
    # (undamped cycles stall at 0.94-0.96 on these right-hand sides: at 1e-6 ||f|| every problem
    # would end at max_cycles -- the stall cases below run that -- so the plain batches share a
    # target the undamped solve reaches, after different numbers of cycles)
    "plain17": (17, "f64", "V", 0.0, {}, dict(rtol=0.0, max_cycles=12), 1e-1),
    "plain65": (65, "f64", "V", 0.0, {}, dict(rtol=0.0, max_cycles=12), 1e-1),
    "every2_17": (17, "f64", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12, check_every=2), 1e-6),
    "stall17": (17, "f64", "V", 0.0, {}, dict(rtol=0.0, max_cycles=12, stall_ratio=0.9,
                                             stall_checks=2), 1e-6),
    "stall65": (65, "f64", "V", 0.0, {}, dict(rtol=0.0, max_cycles=12, stall_ratio=0.9,
                                             stall_checks=2), 1e-6),
    "w2_17": (17, "f64", "W", 0.5, {"alpha": 2}, dict(rtol=0.0, max_cycles=12), 1e-6),
    "w2_65": (65, "f64", "W", 0.5, {"alpha": 2}, dict(rtol=0.0, max_cycles=12), 1e-6),
    "f32_17": (17, "f32", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12), 1e-3),
    "f32_65": (65, "f32", "V", 0.5, {}, dict(rtol=0.0, max_cycles=12), 1e-3),
}


@functools.lru_cache(maxsize=None)
def solve_case(name):
    """The batch `name`: a namespace with N, dtype, kind, omega, cfg, rule (atol included), the
    problems [(f, phi0)] and the model's result for each (models).  The problems: the four seeds'
    f plain and scaled by 1e-3 from phi0 = 0; seed 12345's f times 1e3 (too far for max_cycles);
    seed 12345's plain f from a phi0 the model has already converged (stops at check 0); the
    all-zero problem (0 <= atol at check 0)."""
    N, dtype, kind, omega, cfg, rule, afac = SOLVE_CASES[name]
    dt = _dt(dtype)
    base = mt(N, SEEDS[0], dtype)
    rule = dict(rule, atol=afac * fnorm(base))
    zero = _ro(np.zeros((N, N), dtype=dt))
    probs = []
    for s in SEEDS:
        f = mt(N, s, dtype)
        probs.append((f, zero))
        probs.append((_ro(f * dt(1e-3)), zero))
    probs.append((_ro(base * dt(1e3)), zero))
    # a start the damped model has converged well below atol, whatever the case's own smoother
    done = solve(N, base, None, "V", 0.5, dtype, cfg={}, rtol=0.0, atol=rule["atol"] * 1e-2,
                 max_cycles=40)
    assert done.reason == solve_rule.CONVERGED
    probs.append((base, _ro(done.phi)))
    probs.append((zero, zero))
    models = [solve(N, f, p0, kind, omega, dtype, cfg=cfg, **rule) for f, p0 in probs]
    return SimpleNamespace(name=name, N=N, dtype=dtype, kind=kind, omega=omega, cfg=cfg, rule=rule,
                           problems=probs, models=models)
