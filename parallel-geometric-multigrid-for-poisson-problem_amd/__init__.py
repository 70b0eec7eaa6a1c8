"""MI355X-native geometric multigrid for the 2D Poisson problem (fp64; fp32 variant).

The hot path (Jacobi smoother, residual + norm, full-weighting restriction,
prolongation, V/W-cycles) is hand-written HIP for gfx950 in ``csrc/`` behind the C ABI
of ``include/pgmg.h`` (libpgmg.so).  This Python package is plumbing: a ctypes
wrapper used by the tests, ``bench.py`` and ``__graft_entry__``.  The C++ mirror of
the reference's own entry points (``Parallel``, ``ParallelMultiGridSolver``,
``ParallelTestRunner``, ``gpu_exec``) lives in ``host/``.

Import name: the directory name is not a Python identifier, so load it with
``_pkgload.load()`` from the repository root (registers it as ``pgmg_amd``).
"""
import ctypes as C
import pathlib
import contextlib
import subprocess

import numpy as np

from ._capi import (PGMG_FLAG_LOOPBACK, PGMG_FLAG_NO_CROSS, PGMG_FLAG_NO_GRAPH,
                    PGMG_FLAG_STORED_RHS, PGMG_FLAG_EXACT_DIST, PGMG_FLAG_SOLO,
                    PGMG_FLAG_TIME_FINE, PGMG_PRECISION_FP32, PGMG_PRECISION_FP64,
                    PGMG_FLAG_UNFUSED, PGMG_FLAG_NO_RECOMPUTE, PGMG_FLAG_NO_PIN,
                    PGMG_FLAG_NO_R2, PGMG_FLAG_HOST_TRANSPORT, PGMG_FLAG_FAST,
                    PGMG_FLAG_NO_SPEC_FIRE, PGMG_FLAG_NO_CTILE, PGMG_FLAG_NO_CARRY, PGMG_FLAG_TIME_COMM, PGMG_FLAG_NO_SHUFFLE, PGMG_FLAG_NO_SPIN,
                    PGMG_FLAG_FULL_CHECKS, PGMG_PROLONG_REFERENCE,
                    PGMG_PROLONG_SYMMETRIC, PGMG_OK, PGMG_ERR_ARG, PGMG_ERR_STATE, PgmgConfig, PgmgError,
                    PGMG_MON_RESIDUAL, PGMG_MON_ERROR, PGMG_CYCLE_V, PGMG_CYCLE_W, PGMG_CYCLE_F,
                    PGMG_STOP_CONVERGED, PGMG_STOP_MAX_CYCLES, PGMG_STOP_STALLED,
                    PGMG_STOP_NONFINITE, PgmgMonitorOut, PgmgSolveOpts, PgmgSolveInfo,
                    PgmgExtrapInfo, PgmgProjectInfo, PgmgMixedInfo, PgmgVortInfo,
                    PGMG_WALL_NOSLIP, PGMG_WALL_FREE, PgmgBoussParams, PgmgBoussInfo,
                    PGMG_TWALL_BOTTOM, PGMG_TWALL_TOP, PGMG_TWALL_LEFT, PGMG_TWALL_RIGHT, check, load)

PKG_DIR = pathlib.Path(__file__).resolve().parent

__all__ = [
    "build", "load", "Solver", "BatchSolver", "PgmgConfig", "PgmgError", "ops", "config_overrides",
    "PGMG_FLAG_NO_GRAPH", "PGMG_FLAG_TIME_FINE", "PGMG_FLAG_UNFUSED", "PGMG_FLAG_LOOPBACK", "PGMG_FLAG_NO_CROSS",
    "PGMG_PROLONG_REFERENCE", "plan_strips", "LoopbackHub", "unique_id", "rccl_latency",
    "PGMG_PROLONG_SYMMETRIC", "PGMG_PRECISION_FP64", "PGMG_PRECISION_FP32",
    "PGMG_FLAG_STORED_RHS", "PGMG_FLAG_EXACT_DIST", "PGMG_FLAG_SOLO",
    "PGMG_FLAG_NO_RECOMPUTE", "PGMG_FLAG_NO_PIN", "PGMG_FLAG_NO_R2", "PGMG_FLAG_FAST", "PGMG_FLAG_NO_SPEC_FIRE", "PGMG_FLAG_NO_CTILE", "PGMG_FLAG_NO_CARRY", "PGMG_FLAG_TIME_COMM", "PGMG_FLAG_NO_SHUFFLE", "PGMG_FLAG_NO_SPIN",
    "PGMG_FLAG_HOST_TRANSPORT", "PGMG_FLAG_FULL_CHECKS", "HostTransport", "DeviceGrid",
    "PGMG_MON_RESIDUAL", "PGMG_MON_ERROR", "PGMG_CYCLE_V", "PGMG_CYCLE_W", "PGMG_CYCLE_F",
    "PGMG_STOP_CONVERGED", "PGMG_STOP_MAX_CYCLES", "PGMG_STOP_STALLED", "PGMG_STOP_NONFINITE",
    "PgmgSolveOpts", "PgmgSolveInfo", "PgmgMonitorOut", "PgmgExtrapInfo",
    "PgmgProjectInfo", "PgmgMixedInfo", "PgmgVortInfo", "PGMG_WALL_NOSLIP", "PGMG_WALL_FREE",
    "PgmgBoussParams", "PgmgBoussInfo", "PGMG_TWALL_BOTTOM", "PGMG_TWALL_TOP", "PGMG_TWALL_LEFT",
    "PGMG_TWALL_RIGHT", "twall_mask",
]

_TWALLS = {"bottom": PGMG_TWALL_BOTTOM, "top": PGMG_TWALL_TOP, "left": PGMG_TWALL_LEFT,
           "right": PGMG_TWALL_RIGHT}


def twall_mask(adiabatic):
    """The PGMG_TWALL_* mask of `adiabatic`: an int is taken as the mask itself, otherwise the
    names of the adiabatic walls among "bottom" (y = 0), "top", "left" (x = 0) and "right"."""
    if isinstance(adiabatic, int):
        if not 0 <= adiabatic < 2 ** 32:
            raise ValueError("adiabatic: a mask is an unsigned 32-bit value")
        return adiabatic
    if isinstance(adiabatic, str):
        adiabatic = (adiabatic,)
    mask = 0
    for name in adiabatic:
        if name not in _TWALLS:
            raise ValueError(f"adiabatic: {name!r} is none of {sorted(_TWALLS)}")
        mask |= _TWALLS[name]
    return mask


def build(jobs=8, verbose=False):
    """Compile libpgmg.so (and host/gpu_exec) for gfx950 in-tree."""
    cmd = ["make", "-C", str(PKG_DIR), f"-j{jobs}", "all"]
    r = subprocess.run(cmd, capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise PgmgError(f"build failed:\n{r.stdout}\n{r.stderr}")
    return PKG_DIR / "libpgmg.so"


# Config fields applied to every Solver created inside `with config_overrides(...)`
# (flags are OR-ed in).  Tests use it to run the default plan's building blocks on small
# grids (cross_min_n, spec_segment) or an alternative plan (PGMG_FLAG_NO_RECOMPUTE, ...)
# through helpers that build their own Solvers.  Everything goes through pgmg_config.
_overrides = {}


@contextlib.contextmanager
def config_overrides(**kw):
    saved = dict(_overrides)
    for k, v in kw.items():
        if k == "flags":
            _overrides["flags"] = _overrides.get("flags", 0) | int(v)
        else:
            _overrides[k] = v
    try:
        yield
    finally:
        _overrides.clear()
        _overrides.update(saved)


def default_config(N, **kw):
    cfg = PgmgConfig()
    check(load().pgmg_config_default(C.byref(cfg), int(N)), "pgmg_config_default")
    kw = dict(kw)
    for k, v in _overrides.items():
        if k == "flags":
            kw["flags"] = kw.get("flags", 0) | v
        else:
            kw.setdefault(k, v)
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def plan_strips(N, world, rank, tail_n=65, gather_n=1025):
    """Finest-level rows [lo, hi) owned by `rank` and the number of strip-distributed
    levels (host arithmetic of the row-strip decomposition; no GPU needed)."""
    lo, hi, nd = C.c_int(), C.c_int(), C.c_int()
    check(load().pgmg_plan_strips(int(N), int(world), int(rank), int(tail_n), int(gather_n),
                                  C.byref(lo), C.byref(hi), C.byref(nd)), "pgmg_plan_strips")
    return lo.value, hi.value, nd.value


def unique_id():
    """A fresh 128-byte RCCL unique id (rank 0 creates it, then broadcasts it)."""
    buf = (C.c_ubyte * 128)()
    check(load().pgmg_comm_unique_id(buf), "pgmg_comm_unique_id")
    return bytes(buf)


def rccl_latency(device=0, reps=200):
    """Latency floor of the strips' collectives on this device (world-1 RCCL communicator):
    {"halo_group_us", "allreduce_sum_us", "allreduce_min_us"} (pgmg_rccl_latency)."""
    us = (C.c_double * 3)()
    uid = (C.c_ubyte * 128).from_buffer_copy(unique_id())
    check(load().pgmg_rccl_latency(uid, int(device), int(reps), us), "pgmg_rccl_latency")
    return {"halo_group_us": us[0], "allreduce_sum_us": us[1], "allreduce_min_us": us[2]}


from .hostcomm import HostTransport  # noqa: E402


class LoopbackHub:
    """In-process rank hub: `world` Solvers in threads of one process share one GPU
    (test transport for the strip decomposition; RCCL refuses two ranks per device)."""

    def __init__(self, world):
        h = C.c_void_p()
        check(load().pgmg_loopback_create(int(world), C.byref(h)), "pgmg_loopback_create")
        self.h = h
        self.world = world

    def fail(self, rank, at_group):
        """Test hook: rank's at_group-th transport group from now on fails (0: never)."""
        check(load().pgmg_loopback_fail(self.h, int(rank), int(at_group)), "pgmg_loopback_fail")

    def close(self):
        if self.h:
            load().pgmg_loopback_destroy(self.h)
            self.h = None


class Solver:
    """A multigrid context: level pyramid resident in HBM, cycles on a HIP stream.

    Mirrors ParallelTestRunner::run_v_cycle / ParallelMultiGridSolver::v_cycle
    (3_part_parallel/ParallelTestRunner.cu:152-186, Parallel_Mg.cu:21-60) with the
    numerics of MultigridSolver (2_part_MG/MultiGrid.hpp:57-136).
    """

    def __init__(self, N, hub=None, uid=None, dtype="f64", transport=None, **cfg):
        """hub: LoopbackHub (ranks as threads on one GPU); uid: 128-byte RCCL unique id;
        transport: a HostTransport (ranks as processes, messages through the caller's
        torch.distributed group, staged in host memory);
        dtype: "f64" (bit-exact to mg_cpu_exec) or "f32" (PGMG_PRECISION_FP32)."""
        self.lib = load()
        if dtype not in ("f64", "f32"):
            raise ValueError(f"dtype must be 'f64' or 'f32', not {dtype!r}")
        cfg.setdefault("precision", PGMG_PRECISION_FP32 if dtype == "f32" else PGMG_PRECISION_FP64)
        if hub is not None:
            cfg["flags"] = cfg.get("flags", 0) | PGMG_FLAG_LOOPBACK
            cfg["world"] = hub.world
            cfg["nccl_unique_id"] = hub.h
        elif transport is not None:
            self._transport = transport   # the callbacks must outlive the context
            cfg["flags"] = cfg.get("flags", 0) | PGMG_FLAG_HOST_TRANSPORT
            cfg.setdefault("world", transport.world)
            cfg.setdefault("rank", transport.rank)
            cfg["nccl_unique_id"] = C.cast(C.pointer(transport.struct), C.c_void_p)
        elif uid is not None:
            self._uid = (C.c_ubyte * 128)(*uid)
            cfg["nccl_unique_id"] = C.cast(self._uid, C.c_void_p)
        self.cfg = default_config(N, **cfg)
        h = C.c_void_p()
        check(self.lib.pgmg_create(C.byref(h), C.byref(self.cfg)), "pgmg_create")
        self.h = h
        self.N = int(N)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pgmg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_problem(self, phi0=None, f=None):
        N = self.N
        args = []
        for a in (phi0, f):
            if a is None:
                args.append(None)
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
                assert a.shape == (N, N), a.shape
                args.append(a)
        p = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in args]
        check(self.lib.pgmg_set_problem(self.h, p[0], p[1]), "pgmg_set_problem")

    def set_problem_device(self, phi, f=None):
        """Bind device arrays (DeviceGrid, torch tensors or raw device pointers; N*N float64
        in the reference layout) as the problem: phi is updated in place by every following
        cycle call; f None = the analytic RHS (pgmg_set_problem_device)."""
        check(self.lib.pgmg_set_problem_device(self.h, _dptr(phi), _dptr(f)),
              "pgmg_set_problem_device")

    def device_info(self):
        """(a device problem is bound, its calls run in place)"""
        b, i = C.c_int(), C.c_int()
        check(self.lib.pgmg_problem_device_info(self.h, C.byref(b), C.byref(i)),
              "pgmg_problem_device_info")
        return bool(b.value), bool(i.value)

    def vcycle(self, n=1):
        check(self.lib.pgmg_vcycle(self.h, int(n)), "pgmg_vcycle")

    def wcycle(self, n=1):
        check(self.lib.pgmg_wcycle(self.h, int(n)), "pgmg_wcycle")

    def fcycle(self, n=1):
        check(self.lib.pgmg_fcycle(self.h, int(n)), "pgmg_fcycle")

    def fmg(self, nu=2, damp=None, boundary="zero"):
        """Replace phi with the full-multigrid solution of the problem's own right-hand side
        (pgmg_fmg): f restricted down the pyramid, the coarsest level solved from zero, then per
        level the cubic interpolation of the coarser solution and `nu` V-cycles.  With
        boundary="zero" the current phi is ignored, boundary included; with "keep" its interior
        is ignored.  With nu=2 the result is at the discretisation error for about 8/3
        finest-level V-cycles of work, so a solve that starts from it needs few cycles::

            s.set_problem(None, f); s.fmg(); s.solve(rtol=1e-8)

        damp: None is pgmg_fmg exactly; an omega in (0, 1] (0.5 recommended) follows every
        V-cycle of the climb with a damping pass on that level (pgmg_fmg_damped), which removes
        the checkerboard error the undamped smoother leaves: for any right-hand side but the
        smooth analytic one the residual is about 100 times smaller.
        boundary: "zero" solves the problem with a zero Dirichlet boundary and leaves phi with
        one, whatever phi held; "keep" (pgmg_fmg_bc) solves the problem whose Dirichlet data is
        the frame of the current phi (rows and columns 0 and N-1): every level of the climb
        carries the injection of that frame, and the result's frame is bit for bit the one phi
        had.  With an all-zero frame the two give the same bits.  One GPU only."""
        if boundary not in ("zero", "keep"):
            raise ValueError(f"boundary must be 'zero' or 'keep', not {boundary!r}")
        if boundary == "keep":
            check(self.lib.pgmg_fmg_bc(self.h, int(nu), float(damp or 0.0)), "pgmg_fmg_bc")
        elif damp is None:
            check(self.lib.pgmg_fmg(self.h, int(nu)), "pgmg_fmg")
        else:
            check(self.lib.pgmg_fmg_damped(self.h, int(nu), float(damp)), "pgmg_fmg_damped")

    def fmg_interp_time(self, reps=20):
        """(mean device ms, algorithmic bytes) of the cubic interpolation pass level 1 ->
        level 0 over `reps` back to back (pgmg_fmg_interp_time; measurement, leaves phi
        changed)."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_fmg_interp_time(self.h, int(reps), C.byref(ms), C.byref(b)),
              "pgmg_fmg_interp_time")
        return ms.value, b.value

    def sync(self):
        check(self.lib.pgmg_sync(self.h), "pgmg_sync")

    def solution(self):
        out = np.empty((self.N, self.N), dtype=np.float64)
        check(self.lib.pgmg_get_solution(self.h, out.ctypes.data_as(C.c_void_p)),
              "pgmg_get_solution")
        return out

    def rhs(self):
        """The level-0 right-hand side as the context stores it (pgmg_get_rhs)."""
        out = np.empty((self.N, self.N), dtype=np.float64)
        check(self.lib.pgmg_get_rhs(self.h, out.ctypes.data_as(C.c_void_p)), "pgmg_get_rhs")
        return out

    def solution_hash(self, root=0):
        """FNV-64 of phi (hex string, the golden fixtures' format) on rank `root`; collective
        on row strips (other ranks get None)."""
        v = C.c_ulonglong()
        check(self.lib.pgmg_solution_hash(self.h, int(root), C.byref(v)), "pgmg_solution_hash")
        mine = self.cfg.world <= 1 or root < 0 or self.cfg.rank == root
        return "%016x" % v.value if mine else None

    def gather_solution(self, root, want):
        """Collective: phi gathered to rank `root` only; returns it where `want`, else None
        (row strips of a large grid without a full host copy per rank)."""
        out = np.empty((self.N, self.N), dtype=np.float64) if want else None
        ptr = out.ctypes.data_as(C.c_void_p) if want else None
        check(self.lib.pgmg_gather_solution(self.h, int(root), ptr), "pgmg_gather_solution")
        return out

    def residual_norm(self):
        v = C.c_double()
        check(self.lib.pgmg_residual_norm(self.h, C.byref(v)), "pgmg_residual_norm")
        return v.value

    def monitor(self, error=False, residual=True):
        """One pass over the current iterate where it lies (pgmg_monitor): a PgmgMonitorOut
        with res_norm and, with error=True (analytic problems), err_norm, exact_norm and
        rel_error against the analytic solution; what was not asked for is NaN.  Keeps the
        carry; collective on row strips."""
        what = (PGMG_MON_RESIDUAL if residual else 0) | (PGMG_MON_ERROR if error else 0)
        out = PgmgMonitorOut()
        check(self.lib.pgmg_monitor(self.h, what, C.byref(out)), "pgmg_monitor")
        return out

    def monitor_time(self, reps=20, error=False, residual=True):
        """(mean device ms, algorithmic bytes) of one monitor pass over `reps` back to back
        (pgmg_monitor_time; measurement)."""
        what = (PGMG_MON_RESIDUAL if residual else 0) | (PGMG_MON_ERROR if error else 0)
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_monitor_time(self.h, what, int(reps), C.byref(ms), C.byref(b)),
              "pgmg_monitor_time")
        return ms.value, b.value

    def damp(self, omega=0.5):
        """One finest-level damped-Jacobi correction phi <- phi + omega (h^2/4) r (pgmg_damp):
        the monitor's pass that also writes.  Returns the residual norm of phi BEFORE the
        update.  omega = 1/2 removes the checkerboard error the cycles' undamped smoother
        leaves.  Drops the carry; one GPU only."""
        v = C.c_double()
        check(self.lib.pgmg_damp(self.h, float(omega), C.byref(v)), "pgmg_damp")
        return v.value

    def damp_time(self, omega=0.5, reps=20):
        """(mean device ms, algorithmic bytes) of one damping pass over `reps` back to back
        (pgmg_damp_time; measurement, leaves phi changed)."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_damp_time(self.h, float(omega), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_damp_time")
        return ms.value, b.value

    def solve(self, cycle="V", rtol=1e-3, atol=0.0, max_cycles=30, check_every=1,
              stall_ratio=0.0, stall_checks=2, error=False, damp=0.0, start=None, nu=2,
              boundary="zero", order=2):
        """Cycle until the residual norm is at most max(atol, rtol * r0), the cycle cap, a
        stall or a non-finite norm (pgmg_solve; the stop rule: include/pgmg.h).  Returns the
        PgmgSolveInfo with a `.history` list of (cycle, res, rel_error), check 0 first.
        damp: 0.0 is pgmg_solve exactly; a positive omega (0.5 recommended) makes every check a
        damping pass (pgmg_solve_damped), which converges for any right-hand side; phi afterwards
        is the damped last iterate, its residual norm at most info.res.
        start: None starts from the current phi; "fmg" first replaces it with fmg(nu, damp)
        (damped when damp is positive), so check 0 -- and r0 of the rule -- is the FMG iterate's
        and info.cycles counts the cycles after it.  rtol is then relative to a residual FMG has
        already brought down (by ~1e-3 with damp=0.5): give the target as atol to compare with
        a solve from zero.
        boundary: passed to fmg with start="fmg": "zero" ignores the current phi, boundary
        included, and solves the zero-boundary problem; "keep" ignores its interior only and
        solves the problem with the Dirichlet data phi carries (ignored without start).
        order: 2 is the solve described above.  4 (pgmg_solve_extrap; fp64, one GPU) makes the
        result fourth-order accurate by Richardson extrapolation: the same damped solve, started
        from fmg(nu, damp, "keep"), on this grid and on the grid of every second point, then
        phi <- phi + cubic((phi - phi_2h) / 3) on the interior.  It needs damp > 0 and implies
        start="fmg" and boundary="keep"; state the target as atol (~1e-10 ||f||) and create the
        Solver with eps < 0 (include/pgmg.h).  Returns the fine solve's PgmgSolveInfo with
        `.history`, `.coarse` (the half-resolution solve's PgmgSolveInfo), `.coarse_sweeps`,
        `.coarse_exits`, `.extrap_ms` (device time of the two extrapolation passes) and
        `.total_ms` (host wall time of the whole call)."""
        if start not in (None, "fmg"):
            raise ValueError(f"start must be None or 'fmg', not {start!r}")
        if order not in (2, 4):
            raise ValueError(f"order must be 2 or 4, not {order!r}")
        if order == 4 and not damp > 0.0:
            raise ValueError("order=4 needs damp > 0 (0.5 recommended): undamped solves leave an "
                             "algebraic error above the h^4 term")
        if start == "fmg" and order == 2:
            self.fmg(nu, damp if damp != 0.0 else None, boundary)
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        kinds = {"V": PGMG_CYCLE_V, "W": PGMG_CYCLE_W, "F": PGMG_CYCLE_F}
        o.cycle = kinds[cycle] if cycle in kinds else int(cycle)
        o.rtol, o.atol, o.max_cycles, o.check_every = rtol, atol, int(max_cycles), int(check_every)
        o.stall_ratio, o.stall_checks = stall_ratio, int(stall_checks)
        o.monitor = PGMG_MON_RESIDUAL | (PGMG_MON_ERROR if error else 0)
        if order == 4:
            ex = PgmgExtrapInfo()
            check(self.lib.pgmg_solve_extrap(self.h, C.byref(o), int(nu), float(damp),
                                             C.byref(ex)), "pgmg_solve_extrap")
            info = ex.fine
            info.coarse, info.coarse_sweeps, info.coarse_exits = ex.coarse, ex.coarse_sweeps, ex.coarse_exits
            info.extrap_ms, info.total_ms = ex.extrap_ms, ex.elapsed_ms
            info.history = self.history()
            return info
        info = PgmgSolveInfo()
        if damp == 0.0:
            check(self.lib.pgmg_solve(self.h, C.byref(o), C.byref(info)), "pgmg_solve")
        else:
            check(self.lib.pgmg_solve_damped(self.h, C.byref(o), float(damp), C.byref(info)),
                  "pgmg_solve_damped")
        info.history = self.history()
        return info

    def gradient(self, order=4, scale=1.0, gx=None, gy=None, norm=False):
        """scale * grad(phi) of the current phi on all N x N points, frame included, in one pass
        over phi where it lies (pgmg_gradient): central differences of the given order (2 or 4)
        and one-sided ones of the same order on the frame.  scale=-1 gives E = -grad(phi).
        Order 4 only pays on the result of solve(order=4): the field of a second-order solution
        is second order whatever the stencil.  gx, gy: N x N float64 CUDA tensors (allocated when
        None).  Returns (gx, gy), or (gx, gy, sqrt(sum gx^2 + gy^2)) with norm=True.  Only reads
        the problem: keeps the carry and the statistics.  fp64 and fp32 contexts (an fp32 context
        computes in fp32 and stores the values widened); one GPU only."""
        import torch
        N = self.N
        dev = torch.device("cuda", int(self.cfg.device))
        if gx is None:
            gx = torch.empty((N, N), dtype=torch.float64, device=dev)
        if gy is None:
            gy = torch.empty((N, N), dtype=torch.float64, device=dev)
        for t in (gx, gy):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                    and t.is_contiguous()):
                raise ValueError("gx and gy must be contiguous N x N float64 CUDA tensors")
        out = C.c_double()
        check(self.lib.pgmg_gradient(self.h, int(order), float(scale), _dptr(gx), _dptr(gy),
                                     C.byref(out) if norm else None), "pgmg_gradient")
        return (gx, gy, out.value) if norm else (gx, gy)

    def gradient_time(self, order=4, reps=20):
        """(mean device ms, algorithmic bytes) of one gradient pass, both components and the
        norm, over `reps` back to back into context-owned outputs (pgmg_gradient_time;
        measurement)."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_gradient_time(self.h, int(order), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_gradient_time")
        return ms.value, b.value

    def project(self, u, v, order=4, nu=2, damp=0.5, rtol=0.0, atol=0.0, max_cycles=30,
                check_every=1, measure_after=False):
        """Make the velocity field (u, v) divergence free in place (pgmg_project): the level-0
        right-hand side becomes f = -div(u, v), formed on the device; the problem with the frame
        of the current phi as Dirichlet data is solved from fmg(nu, damp, "keep") by the damped
        solve (order 2) or by solve(order=4)'s extrapolated pair (order 4); then u -= phi_x,
        v -= phi_y with the stencils of that order.  u, v: contiguous N x N float64 CUDA tensors,
        element (j, i) at x = i h, y = j h.  State the target as atol (~1e-10 ||f||) and create
        the Solver with eps < 0, as for solve(order=4).  Returns the PgmgProjectInfo with
        `.history` (the fine solve's checks); `.div_before` is ||f||, `.div_after` the same of the
        corrected field with measure_after=True (NaN otherwise).  Afterwards phi is the potential
        and f the divergence.  fp64, one GPU, context-owned problems."""
        import torch
        N = self.N
        for t in (u, v):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
                    and tuple(t.shape) == (N, N) and t.is_contiguous()):
                raise ValueError("u and v must be contiguous N x N float64 CUDA tensors")
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        o.rtol, o.atol, o.max_cycles, o.check_every = rtol, atol, int(max_cycles), int(check_every)
        info = PgmgProjectInfo()
        check(self.lib.pgmg_project(self.h, C.byref(o), int(order), int(nu), float(damp), _dptr(u),
                                    _dptr(v), int(bool(measure_after)), C.byref(info)),
              "pgmg_project")
        info.history = self.history()
        return info

    def project_time(self, which, order=4, reps=20):
        """(mean device ms, algorithmic bytes) of one pass of project over `reps` back to back on
        context-owned arrays (pgmg_project_time; measurement): which=0 the divergence with its
        output and norm, which=1 the update of both components.  Leaves phi and f alone."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_project_time(self.h, int(which), int(order), int(reps), C.byref(ms),
                                         C.byref(b)), "pgmg_project_time")
        return ms.value, b.value

    def vorticity_step(self, dt, nu, walls=(0.0, 0.0, 0.0, 0.0), free=False, nsteps=1, damp=0.5,
                       atol=0.0, rtol=0.0, max_cycles=30, check_every=1, order=1):
        """`nsteps` time steps of 2D incompressible flow in streamfunction-vorticity form
        (order=1: explicit Euler, pgmg_vorticity_step; order=2 or 3: the strong-stability-
        preserving Runge-Kutta schemes of pgmg_vorticity_step_rk, `order` stages per step, each an
        Euler pass combined with the vorticity the step started from and followed by its own
        solve; order 3 is stable for cfl <= 1.73 and diffusion <= 1.25 whatever nu, orders 1 and 2
        need the viscosity to damp advection; cycles, sweeps and the worst residual then range
        over all stage solves).  The context's phi is the streamfunction psi (u = psi_y, v = -psi_x)
        and its f the vorticity; start with set_problem(psi0, omega0) (zeros: a cavity at rest).
        Per step: f's frame from psi by Thom's formula with the wall speeds walls = (u on y = 0,
        u on y = a, v on x = 0, v on x = a) -- or +0.0 with free=True (free slip) --, then
        f <- f + dt (nu lap(f) - (psi_y f_x - psi_x f_y)) on the interior, then the damped solve
        of -lap(psi) = f warm-started from the previous psi (state the target as atol, create the
        Solver with eps < 0).  Stability is the caller's business: at orders 1 and 2 keep `.cfl` below
        about 1 and `.diffusion` = 4 nu dt / h^2 at most 1.  Returns a namespace: steps, cycles and sweeps
        (summed), last (the last step's PgmgSolveInfo), worst_res and worst_reason, cfl, diffusion,
        step_ms, solve_ms, elapsed_ms, history (the last solve's checks).  fp64, one GPU,
        context-owned problems."""
        from types import SimpleNamespace
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        o.rtol, o.atol, o.max_cycles, o.check_every = rtol, atol, int(max_cycles), int(check_every)
        w = (C.c_double * 4)(*(float(x) for x in walls))
        info = PgmgVortInfo()
        mode = PGMG_WALL_FREE if free else PGMG_WALL_NOSLIP
        if int(order) == 1:
            check(self.lib.pgmg_vorticity_step(self.h, C.byref(o), float(damp), float(dt), float(nu),
                                               mode, w, int(nsteps), C.byref(info)),
                  "pgmg_vorticity_step")
        else:
            check(self.lib.pgmg_vorticity_step_rk(self.h, C.byref(o), float(damp), float(dt),
                                                  float(nu), mode, w, int(order), int(nsteps),
                                                  C.byref(info)), "pgmg_vorticity_step_rk")
        out = SimpleNamespace(**{name: getattr(info, name) for name, _ in PgmgVortInfo._fields_})
        out.history = self.history()
        return out

    def vorticity_rk_time(self, which, reps=20):
        """(mean device ms, algorithmic bytes) of one Runge-Kutta stage pass of vorticity_step
        (order 2 or 3) over `reps` back to back on context-owned arrays (pgmg_vorticity_rk_time;
        measurement): which=0 the stage with its copy back, which=1 the stage with the velocity
        maximum.  Leaves phi and f alone."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_vorticity_rk_time(self.h, int(which), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_vorticity_rk_time")
        return ms.value, b.value

    def vorticity_time(self, which, reps=20):
        """(mean device ms, algorithmic bytes) of one pass of vorticity_step over `reps` back to
        back on context-owned arrays (pgmg_vorticity_time; measurement): which=0 the step with
        its copy back, which=1 the step with the velocity maximum.  Leaves phi and f alone."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_vorticity_time(self.h, int(which), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_vorticity_time")
        return ms.value, b.value

    def boussinesq_step(self, T, dt, nu, kappa, buoy=(0.0, 1.0), walls=(0.0, 0.0, 0.0, 0.0),
                        free=False, adiabatic=("bottom", "top"), nsteps=1, damp=0.5, atol=0.0,
                        rtol=0.0, max_cycles=30, check_every=1, order=1):
        """`nsteps` time steps of buoyancy-driven flow (order=1: explicit Euler,
        pgmg_boussinesq_step; order=2 or 3: the strong-stability-preserving Runge-Kutta schemes of
        pgmg_boussinesq_step_rk, `order` stages per step with one (a, b) for f and T, each stage
        followed by its own solve; the buoyancy coupling oscillates on the imaginary axis, which
        order 3 covers up to sqrt(3), order 2 nearly and Euler not at all):
        vorticity_step's flow carrying the temperature T, which feeds back into the vorticity:
        f_t + u f_x + v f_y = nu lap(f) + (by T_x - bx T_y), T_t + u T_x + v T_y = kappa lap(T),
        buoy = (bx, by) (gravity along -y: (0, g beta)).  T: a contiguous N x N float64 CUDA
        tensor, updated in place; its walls named in `adiabatic` ("bottom", "top", "left", "right",
        or a PGMG_TWALL_* mask) are set by the one-sided dT/dn = 0 before every step and after the
        last, the others keep the values T came with (Dirichlet).  Both steps are one pass over
        psi, f and T.  walls, free and the solve's arguments are vorticity_step's.  Returns its
        namespace plus diffusion_t = 4 kappa dt / h^2 (keep it at most 1).  fp64, one GPU,
        context-owned problems."""
        import torch
        from types import SimpleNamespace
        N = self.N
        if not (isinstance(T, torch.Tensor) and T.is_cuda and T.dtype == torch.float64
                and tuple(T.shape) == (N, N) and T.is_contiguous()):
            raise ValueError("T must be a contiguous N x N float64 CUDA tensor")
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        o.rtol, o.atol, o.max_cycles, o.check_every = rtol, atol, int(max_cycles), int(check_every)
        p = PgmgBoussParams()
        p.dt, p.nu, p.kappa = float(dt), float(nu), float(kappa)
        p.buoy = (C.c_double * 2)(*(float(x) for x in buoy))
        p.mode = PGMG_WALL_FREE if free else PGMG_WALL_NOSLIP
        p.walls = (C.c_double * 4)(*(float(x) for x in walls))
        p.adiabatic = twall_mask(adiabatic)
        info = PgmgBoussInfo()
        if int(order) == 1:
            check(self.lib.pgmg_boussinesq_step(self.h, C.byref(o), float(damp), C.byref(p), _dptr(T),
                                                int(nsteps), C.byref(info)), "pgmg_boussinesq_step")
        else:
            check(self.lib.pgmg_boussinesq_step_rk(self.h, C.byref(o), float(damp), C.byref(p),
                                                   _dptr(T), int(order), int(nsteps), C.byref(info)),
                  "pgmg_boussinesq_step_rk")
        out = SimpleNamespace(**{name: getattr(info.flow, name) for name, _ in PgmgVortInfo._fields_})
        out.diffusion_t = info.diffusion_t
        out.history = self.history()
        return out

    def boussinesq_time(self, which, reps=20):
        """(mean device ms, algorithmic bytes) of one pass of boussinesq_step over `reps` back to
        back on context-owned arrays (pgmg_boussinesq_time; measurement): which=0 the step with
        both copies back, which=1 the step with the velocity maximum.  Leaves phi, f and every
        caller's array alone."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_boussinesq_time(self.h, int(which), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_boussinesq_time")
        return ms.value, b.value

    def boussinesq_rk_time(self, which, reps=20):
        """(mean device ms, algorithmic bytes) of one Runge-Kutta stage pass of boussinesq_step
        (order 2 or 3) over `reps` back to back on context-owned arrays (pgmg_boussinesq_rk_time;
        measurement): which=0 the stage with both copies back, which=1 the stage with the velocity
        maximum; 2 and 3 the same at the pass's other built depth.  Leaves phi, f and every
        caller's array alone."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_boussinesq_rk_time(self.h, int(which), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_boussinesq_rk_time")
        return ms.value, b.value

    def velocity(self, u=None, v=None):
        """(u, v) = (psi_y, -psi_x) of the current phi read as a streamfunction: two gradient
        passes at order 2 with one output each (pgmg_gradient: gy into u at scale 1, gx into v at
        scale -1).  u, v: N x N float64 CUDA tensors (allocated when None)."""
        import torch
        N = self.N
        dev = torch.device("cuda", int(self.cfg.device))
        if u is None:
            u = torch.empty((N, N), dtype=torch.float64, device=dev)
        if v is None:
            v = torch.empty((N, N), dtype=torch.float64, device=dev)
        for t in (u, v):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (N, N)
                    and t.is_contiguous()):
                raise ValueError("u and v must be contiguous N x N float64 CUDA tensors")
        check(self.lib.pgmg_gradient(self.h, 2, 1.0, None, _dptr(u), None), "pgmg_gradient")
        check(self.lib.pgmg_gradient(self.h, 2, -1.0, _dptr(v), None, None), "pgmg_gradient")
        return u, v

    def solve_mixed(self, rtol=0.0, atol=0.0, max_steps=8, nu=2, damp=0.5, stall_ratio=0.0,
                    stall_checks=2):
        """Mixed-precision refinement of the current phi (pgmg_solve_mixed; fp64 context, one
        GPU): phi and its residual stay in fp64, every correction is an fp32 fmg(nu, damp) of the
        scaled residual on an fp32 context this one owns, and this context runs no cycle.  Each
        step cuts the fp64 residual norm by a factor that depends on nu alone (~400 .. 3100 at
        nu=2, ~4500 .. 18000 at nu=3) down to fp64's floor, ~0.4 N^2 2^-52 ||f||: state the
        target as atol.  The stop rule is solve()'s with steps for cycles; on a stop phi is
        exactly the iterate the last norm was measured on.  Returns the PgmgSolveInfo (cycles =
        steps applied) with `.history` [(steps, res, nan)], `.inner_sweeps` (the fp32 context's
        sweeps), `.defect_ms`, `.inner_ms`, `.correct_ms` (device time, summed over the steps)
        and `.total_ms` (host wall time of the call)."""
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        o.cycle, o.check_every, o.monitor = PGMG_CYCLE_V, 1, PGMG_MON_RESIDUAL
        o.rtol, o.atol, o.max_cycles = rtol, atol, int(max_steps)
        o.stall_ratio, o.stall_checks = stall_ratio, int(stall_checks)
        mx = PgmgMixedInfo()
        check(self.lib.pgmg_solve_mixed(self.h, C.byref(o), int(nu), float(damp), C.byref(mx)),
              "pgmg_solve_mixed")
        info = mx.solve
        info.inner_sweeps = mx.inner_sweeps
        info.defect_ms, info.inner_ms, info.correct_ms = mx.defect_ms, mx.inner_ms, mx.correct_ms
        info.total_ms = mx.elapsed_ms
        info.history = self.history()
        return info

    def mixed_time(self, which, reps=20):
        """(mean device ms, algorithmic bytes) of one pass of solve_mixed over `reps` back to back
        (pgmg_mixed_time; measurement): which=0 the defect pass with its reduction, which=1 the
        correction.  Leaves phi changed."""
        ms, b = C.c_double(), C.c_double()
        check(self.lib.pgmg_mixed_time(self.h, int(which), int(reps), C.byref(ms), C.byref(b)),
              "pgmg_mixed_time")
        return ms.value, b.value

    def history(self):
        """The last solve's checks: [(cycles run before the check, res, rel_error), ...]."""
        n = C.c_int()
        check(self.lib.pgmg_history(self.h, 0, None, None, None, C.byref(n)), "pgmg_history")
        k = n.value
        cyc, res, rel = (C.c_int * k)(), (C.c_double * k)(), (C.c_double * k)()
        check(self.lib.pgmg_history(self.h, k, cyc, res, rel, C.byref(n)), "pgmg_history")
        return [(cyc[i], res[i], rel[i]) for i in range(k)]

    def stats(self):
        s, e = C.c_longlong(), C.c_longlong()
        check(self.lib.pgmg_stats(self.h, C.byref(s), C.byref(e)), "pgmg_stats")
        return s.value, e.value

    def stats_detail(self):
        """[sweeps, early exits, k_postpre post-check rare paths (-1: not cross-fused),
        k_postpre pre-check rare paths]"""
        v = (C.c_longlong * 4)()
        check(self.lib.pgmg_stats_detail(self.h, v), "pgmg_stats_detail")
        return list(v)

    def last_elapsed_ms(self):
        v = C.c_double()
        check(self.lib.pgmg_last_elapsed_ms(self.h, C.byref(v)), "pgmg_last_elapsed_ms")
        return v.value

    def levels(self):
        b, t = C.c_int(), C.c_int()
        check(self.lib.pgmg_levels(self.h, C.byref(b), C.byref(t)), "pgmg_levels")
        return b.value, t.value

    def vcycle_bytes(self):
        v = C.c_double()
        check(self.lib.pgmg_vcycle_bytes(self.h, C.byref(v)), "pgmg_vcycle_bytes")
        return v.value

    def fine_sweep_time(self):
        n, m = C.c_int(), C.c_double()
        check(self.lib.pgmg_fine_sweep_time(self.h, C.byref(n), C.byref(m)),
              "pgmg_fine_sweep_time")
        return n.value, m.value

    def fine_pass_time(self, which):
        """(count, mean ms) of finest-level kernels: 0 plain sweep, 1 k_pre, 2 k_post,
        3 k_postpre, 4 the carry pass."""
        n, m = C.c_int(), C.c_double()
        check(self.lib.pgmg_fine_pass_time(self.h, int(which), C.byref(n), C.byref(m)),
              "pgmg_fine_pass_time")
        return n.value, m.value

    @property
    def fused(self):
        v = C.c_int()
        check(self.lib.pgmg_fused(self.h, C.byref(v)), "pgmg_fused")
        return bool(v.value)

    def fine_pass_info(self, which):
        """(kernel symbol, algorithmic bytes per launch) of the launches the last
        fine_pass_time(which) averaged ("" / 0 when none was timed)."""
        buf = C.create_string_buffer(512)
        b = C.c_double()
        check(self.lib.pgmg_fine_pass_info(self.h, int(which), buf, 512, C.byref(b)),
              "pgmg_fine_pass_info")
        return buf.value.decode(errors="replace"), b.value

    def carry_info(self):
        """(calls that started from a carried pre-smooth, carries made, carries dropped)."""
        a = (C.c_longlong * 3)()
        check(self.lib.pgmg_carry_info(self.h, a), "pgmg_carry_info")
        return tuple(a)

    def sampled_info(self):
        """(finest passes launched with sampled checks, rollbacks caused only by sampled checks
        after which no cross-cycle check fired, 1 while the context sums every row again)."""
        a = (C.c_longlong * 3)()
        check(self.lib.pgmg_spec_sampled_info(self.h, a), "pgmg_spec_sampled_info")
        return tuple(a)

    def comm_stats(self):
        """(collective groups since the last call, ms inside them with PGMG_FLAG_TIME_COMM else
        -1); synchronous, resets."""
        g, m = C.c_longlong(), C.c_double()
        check(self.lib.pgmg_comm_stats(self.h, C.byref(g), C.byref(m)), "pgmg_comm_stats")
        return g.value, m.value

    def comm_ranks(self):
        """Ranks of the communicator (RCCL: ncclCommCount); 1 without strips."""
        n = C.c_int()
        check(self.lib.pgmg_comm_ranks(self.h, C.byref(n)), "pgmg_comm_ranks")
        return n.value

    def set_eps(self, eps):
        """A new early-exit threshold for the following calls (drops the carry)."""
        check(self.lib.pgmg_set_eps(self.h, float(eps)), "pgmg_set_eps")

    def fine_pass_bytes(self, which):
        """Algorithmic HBM bytes of one launch of finest-level pass `which` on this rank."""
        v = C.c_double()
        check(self.lib.pgmg_fine_pass_bytes(self.h, int(which), C.byref(v)), "pgmg_fine_pass_bytes")
        return v.value

    def dist_info(self):
        """(speculative early-exit checks (recorded, validated after the call)?, calls
        rolled back and rerun with in-stream decisions)"""
        sp, rb = C.c_int(), C.c_longlong()
        check(self.lib.pgmg_dist_info(self.h, C.byref(sp), C.byref(rb)), "pgmg_dist_info")
        return bool(sp.value), rb.value

    def spec_levels(self):
        """Bit mask: bit l = bulk level l's checks are not speculated "does not fire" (decided
        in-stream, or predicted to fire); bit 0 = no speculation at all."""
        m = C.c_ulonglong()
        check(self.lib.pgmg_spec_levels(self.h, C.byref(m)), "pgmg_spec_levels")
        return m.value

    def spec_fire_levels(self):
        """Bit mask: bit l = bulk level l's checks are predicted to fire (one-sweep passes,
        confirmed by the validation)."""
        m = C.c_ulonglong()
        check(self.lib.pgmg_spec_fire_levels(self.h, C.byref(m)), "pgmg_spec_fire_levels")
        return m.value

    def spec_visit_modes(self):
        """W-cycle plans: (does not fire, predicted to fire, in-stream) visit counts of the last
        speculative W call's bulk levels."""
        a = (C.c_longlong * 3)()
        check(self.lib.pgmg_spec_visit_modes(self.h, a), "pgmg_spec_visit_modes")
        return tuple(a)

    @property
    def elem_bytes(self):
        """8 (fp64) or 4 (fp32): bytes per grid element on the device."""
        p, e = C.c_int(), C.c_int()
        check(self.lib.pgmg_precision(self.h, C.byref(p), C.byref(e)), "pgmg_precision")
        return e.value

    def bench_sweep(self, reps):
        m = C.c_double()
        check(self.lib.pgmg_bench_sweep(self.h, int(reps), C.byref(m)), "pgmg_bench_sweep")
        return m.value


class BatchSolver:
    """Many independent Poisson problems of one size N <= 65 in one launch, one workgroup each
    (include/pgmg.h "Batched small problems").  No context: only the configuration is kept.

        bs = BatchSolver(33)                       # v1, v2, coarse_iter, n_coarse, alpha, eps, h
        out = bs.solve(phi, f, atol=1e-8, rtol=0)  # phi, f: [B, N, N] CUDA tensors, phi in place
        torch.cuda.synchronize(); out.cycles       # per-problem results, device tensors

    dtype "f64" takes float64 tensors, "f32" float32 ones."""

    def __init__(self, N, dtype="f64", **cfg):
        from ._capi import PgmgBatchConfig
        self.lib = load()
        if dtype not in ("f64", "f32"):
            raise ValueError(f"dtype must be 'f64' or 'f32', not {dtype!r}")
        self.dtype = dtype
        self.N = int(N)
        self.cfg = PgmgBatchConfig()
        check(self.lib.pgmg_batch_config_default(C.byref(self.cfg), self.N),
              "pgmg_batch_config_default")
        self.cfg.precision = PGMG_PRECISION_FP32 if dtype == "f32" else PGMG_PRECISION_FP64
        for k, v in cfg.items():
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown batch config field {k}")
            setattr(self.cfg, k, v)

    def _arrays(self, phi, f):
        """B of a matching pair of [B, N, N] device tensors; PgmgError otherwise."""
        import torch
        want = torch.float32 if self.dtype == "f32" else torch.float64
        for name, t in (("phi", phi), ("f", f)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise PgmgError(f"BatchSolver: {name} must be a CUDA tensor")
            if t.dtype != want:
                raise PgmgError(f"BatchSolver: {name} must be {want}, not {t.dtype}")
            if t.dim() != 3 or tuple(t.shape[1:]) != (self.N, self.N) or t.shape[0] < 1:
                raise PgmgError(f"BatchSolver: {name} must have shape [B, {self.N}, {self.N}], "
                                f"not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise PgmgError(f"BatchSolver: {name} must be contiguous")
        if phi.shape[0] != f.shape[0] or phi.device != f.device:
            raise PgmgError("BatchSolver: phi and f must hold the same number of problems on one device")
        return int(phi.shape[0])

    @staticmethod
    def _stream(t):
        import torch
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    @staticmethod
    def _kind(kind):
        kinds = {"V": PGMG_CYCLE_V, "W": PGMG_CYCLE_W, "F": PGMG_CYCLE_F}
        return kinds[kind] if kind in kinds else int(kind)

    def cycle(self, phi, f, n=1, kind="V", stats=False):
        """`n` V- or W-cycles of every problem, in place in phi, asynchronous on torch's current
        stream (pgmg_batch_cycle).  stats=True: returns (sweeps, exits), int64 device tensors of B
        entries, each problem's own counts."""
        import torch
        B = self._arrays(phi, f)
        sw = ex = None
        if stats:
            sw = torch.empty(B, dtype=torch.int64, device=phi.device)
            ex = torch.empty(B, dtype=torch.int64, device=phi.device)
        with torch.cuda.device(phi.device):
            check(self.lib.pgmg_batch_cycle(C.byref(self.cfg), self._kind(kind), int(n), _dptr(phi),
                                            _dptr(f), B, _dptr(sw), _dptr(ex), self._stream(phi)),
                  "pgmg_batch_cycle")
        return (sw, ex) if stats else None

    def solve(self, phi, f, rtol=1e-3, atol=0.0, max_cycles=30, check_every=1, damp=0.5,
              stall_ratio=0.0, stall_checks=2, kind="V", history=False):
        """Solve every problem to max(atol, rtol * r0) by pgmg_solve_damped's loop, each workgroup
        deciding for its own problem (pgmg_batch_solve); damp=0 is the plain solve.  Asynchronous
        on torch's current stream: returns a namespace of device tensors of B entries -- cycles,
        checks, reason (int32), res0, res (float64), sweeps, exits (int64) and, with history=True,
        history [B, max_cycles + 1] (float64, check 0 first, unused slots NaN) -- valid once the
        stream has finished (it does not synchronise)."""
        import torch
        from types import SimpleNamespace
        from ._capi import PgmgBatchOut
        B = self._arrays(phi, f)
        dev = phi.device
        o = PgmgSolveOpts()
        check(self.lib.pgmg_solve_opts_default(C.byref(o)), "pgmg_solve_opts_default")
        o.cycle = self._kind(kind)
        o.rtol, o.atol, o.max_cycles, o.check_every = rtol, atol, int(max_cycles), int(check_every)
        o.stall_ratio, o.stall_checks = stall_ratio, int(stall_checks)
        o.monitor = PGMG_MON_RESIDUAL
        res = SimpleNamespace(
            cycles=torch.empty(B, dtype=torch.int32, device=dev),
            checks=torch.empty(B, dtype=torch.int32, device=dev),
            reason=torch.empty(B, dtype=torch.int32, device=dev),
            res0=torch.empty(B, dtype=torch.float64, device=dev),
            res=torch.empty(B, dtype=torch.float64, device=dev),
            sweeps=torch.empty(B, dtype=torch.int64, device=dev),
            exits=torch.empty(B, dtype=torch.int64, device=dev))
        out = PgmgBatchOut()
        for name in ("cycles", "checks", "reason", "res0", "res", "sweeps", "exits"):
            setattr(out, name, getattr(res, name).data_ptr())
        if history:
            cap = max(int(max_cycles), 0) + 1
            res.history = torch.empty((B, cap), dtype=torch.float64, device=dev)
            out.history, out.history_cap = res.history.data_ptr(), cap
        with torch.cuda.device(dev):
            check(self.lib.pgmg_batch_solve(C.byref(self.cfg), C.byref(o), float(damp), _dptr(phi),
                                            _dptr(f), B, C.byref(out), self._stream(phi)),
                  "pgmg_batch_solve")
        return res

    def time(self, B, n=1, kind="V", reps=20):
        """Mean device ms of one launch of `n` cycles on B problems of pseudo-random right-hand
        sides in the library's own arrays (pgmg_batch_time; measurement, synchronous)."""
        ms = C.c_double()
        check(self.lib.pgmg_batch_time(C.byref(self.cfg), self._kind(kind), int(n), int(B),
                                       int(reps), C.byref(ms)), "pgmg_batch_time")
        return ms.value


def _dptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    if isinstance(t, DeviceGrid):
        return C.c_void_p(t.ptr)
    return C.c_void_p(t.data_ptr())


class DeviceGrid:
    """An N*N float64 device grid in the reference layout with guard rows
    (pgmg_alloc_grid): what ParallelTestRunner allocates with cudaMallocManaged
    (3_part_parallel/ParallelTestRunner.cu:162-163), here device memory."""

    def __init__(self, N, host=None):
        self.lib = load()
        self.N = int(N)
        p = C.c_void_p()
        check(self.lib.pgmg_alloc_grid(C.byref(p), self.N), "pgmg_alloc_grid")
        self.ptr = p.value
        if host is not None:
            self.upload(host)

    def upload(self, host):
        a = np.ascontiguousarray(host, dtype=np.float64)
        assert a.shape == (self.N, self.N), a.shape
        check(self.lib.pgmg_memcpy_h2d(C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p),
                                       a.nbytes), "pgmg_memcpy_h2d")

    def download(self):
        out = np.empty((self.N, self.N), dtype=np.float64)
        check(self.lib.pgmg_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                       out.nbytes), "pgmg_memcpy_d2h")
        return out

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.pgmg_free_grid(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _Ops:
    """Op-level entries on caller-owned device buffers (torch tensors or raw pointers),
    mirroring Parallel::Compute* (3_part_parallel/Parallel_Method.cu:144-199)."""

    @staticmethod
    def _ptr(t):
        if t is None:
            return None
        if isinstance(t, int):
            return C.c_void_p(t)
        return C.c_void_p(t.data_ptr())

    def jacobi(self, x, f, h, v, eps=1e-7, tmp=None, stream=None, count=True):
        """count=False: the reference's void ComputeJacobi shape -- no sweep count returned,
        so no device-to-host readback (the call stays asynchronous on `stream`)."""
        H, W = x.shape
        done = C.c_int()
        check(load().pgmg_jacobi(self._ptr(x), self._ptr(tmp), self._ptr(f), H, W, float(h),
                                 int(v), float(eps), C.byref(done) if count else None, stream),
              "pgmg_jacobi")
        return done.value if count else None

    def residual(self, r, x, f, h, stream=None):
        H, W = x.shape
        check(load().pgmg_residual(self._ptr(r), self._ptr(x), self._ptr(f), H, W, float(h),
                                   stream), "pgmg_residual")

    def restrict(self, fine, coarse, stream=None):
        check(load().pgmg_restrict(self._ptr(fine), self._ptr(coarse), fine.shape[0],
                                   coarse.shape[0], stream), "pgmg_restrict")

    def prolong(self, coarse, fine, mode=PGMG_PROLONG_REFERENCE, num_thread=0, stream=None):
        """num_thread > 0: the reference's launch grid (max(1, Nf // num_thread) *
        num_thread rows and columns touched, Parallel_Method.cu:191-197); 0: all of it."""
        check(load().pgmg_prolong_grid(self._ptr(coarse), self._ptr(fine), coarse.shape[0],
                                       fine.shape[0], int(mode), int(num_thread), stream),
              "pgmg_prolong_grid")

    def norm(self, v, stream=None):
        out = C.c_double()
        check(load().pgmg_norm(self._ptr(v), v.numel(), C.byref(out), stream), "pgmg_norm")
        return out.value

    def damp(self, x, f, h, omega=0.5, stream=None, norm=True):
        """One damping pass x <- x + omega (h^2/4) r on N x N float64 device arrays
        (pgmg_damp_grid; N = 2^k + 1, k >= 2).  norm=True: returns the residual norm of x before
        the update (synchronous); norm=False: returns None, asynchronous on `stream`."""
        N = x.shape[0]
        assert tuple(x.shape) == (N, N) and tuple(f.shape) == (N, N), (x.shape, f.shape)
        out = C.c_double()
        check(load().pgmg_damp_grid(self._ptr(x), self._ptr(f), N, float(h), float(omega),
                                    C.byref(out) if norm else None, stream), "pgmg_damp_grid")
        return out.value if norm else None

    def defect(self, x, f, h, g, scale=1.0, stream=None, norm=True):
        """g = float32(r * scale) on the interior, +0 on the frame, r = f - A x the fp64 residual
        at mesh width h (pgmg_defect_grid): x, f N x N float64 and g N x N float32 device arrays,
        N = 2^k + 1, k >= 2; scale finite and > 0 (a power of two keeps the scaling exact).
        norm=True: returns sqrt(sum r^2) of the unscaled r, bit for bit Solver.monitor()'s
        (synchronous); norm=False: returns None, asynchronous on `stream`."""
        N = x.shape[0]
        assert tuple(x.shape) == (N, N) and tuple(f.shape) == (N, N) and tuple(g.shape) == (N, N)
        out = C.c_double()
        check(load().pgmg_defect_grid(self._ptr(x), self._ptr(f), self._ptr(g), N, float(h),
                                      float(scale), C.byref(out) if norm else None, stream),
              "pgmg_defect_grid")
        return out.value if norm else None

    def correct(self, x, e, scale=1.0, stream=None):
        """x += float64(e) * scale on the interior of x (pgmg_correct_grid): x N x N float64, e
        N x N float32 device arrays; pass scale = 1 / s for a defect scaled by s.  The frame of x
        is never written.  Asynchronous on `stream`."""
        N = x.shape[0]
        assert tuple(x.shape) == (N, N) and tuple(e.shape) == (N, N), (x.shape, e.shape)
        check(load().pgmg_correct_grid(self._ptr(x), self._ptr(e), N, float(scale), stream),
              "pgmg_correct_grid")

    def extrapolate(self, fine, coarse, stream=None):
        """fine <- fine + cubic((fine[::2, ::2] - coarse) * K3) on the interior of fine
        (pgmg_extrap_grid): the Richardson extrapolation of two second-order solutions, fine
        Nf x Nf and coarse (Nf + 1) / 2 squared float64 device arrays, Nf = 2^k + 1, k >= 3.  The
        frame of fine is never written.  Asynchronous on `stream`."""
        Nf, Nc = fine.shape[0], coarse.shape[0]
        assert tuple(fine.shape) == (Nf, Nf) and tuple(coarse.shape) == (Nc, Nc), (fine.shape, coarse.shape)
        assert Nf == 2 * Nc - 1, (Nf, Nc)
        check(load().pgmg_extrap_grid(self._ptr(fine), self._ptr(coarse), Nf, stream),
              "pgmg_extrap_grid")

    def gradient(self, phi, h, gx=None, gy=None, order=4, scale=1.0, stream=None, norm=False):
        """(gx, gy) = scale * grad(phi) on N x N float64 device arrays (pgmg_gradient_grid;
        N = 2^k + 1, k >= 2; h finite and not 0), the outputs allocated when both are None; pass
        one of them to compute that component alone (the other is returned as None).  norm=True:
        returns (gx, gy, sqrt(sum gx^2 + gy^2)) (synchronous); otherwise asynchronous on
        `stream`."""
        import torch
        N = phi.shape[0]
        assert tuple(phi.shape) == (N, N), phi.shape
        if gx is None and gy is None:
            gx, gy = torch.empty_like(phi), torch.empty_like(phi)
        for t in (gx, gy):
            assert t is None or tuple(t.shape) == (N, N), t.shape
        out = C.c_double()
        check(load().pgmg_gradient_grid(self._ptr(phi), self._ptr(gx), self._ptr(gy), N, float(h),
                                        int(order), float(scale), C.byref(out) if norm else None,
                                        stream), "pgmg_gradient_grid")
        return (gx, gy, out.value) if norm else (gx, gy)

    def divergence(self, u, v, h, out=None, order=4, scale=1.0, stream=None, norm=False):
        """out = scale * (du/dx + dv/dy) on N x N float64 device arrays (pgmg_divergence_grid;
        N = 2^k + 1, k >= 2; h finite and not 0), by the line differences of ops.gradient.
        norm=False: returns out (allocated when None), asynchronous on `stream`.  norm=True:
        returns (out, sqrt(sum out^2)), synchronous; with out=None nothing is stored and out is
        returned as None."""
        import torch
        N = u.shape[0]
        assert tuple(u.shape) == (N, N) and tuple(v.shape) == (N, N), (u.shape, v.shape)
        if out is None and not norm:
            out = torch.empty_like(u)
        assert out is None or tuple(out.shape) == (N, N), out.shape
        n = C.c_double()
        check(load().pgmg_divergence_grid(self._ptr(u), self._ptr(v), self._ptr(out), N, float(h),
                                          int(order), float(scale), C.byref(n) if norm else None,
                                          stream), "pgmg_divergence_grid")
        return (out, n.value) if norm else out

    def gradient_add(self, phi, h, u=None, v=None, order=4, scale=1.0, stream=None):
        """u += scale * phi_x, v += scale * phi_y in place on N x N float64 device arrays
        (pgmg_gradient_add_grid), the added values exactly ops.gradient's; either of u, v may be
        None.  Asynchronous on `stream`."""
        N = phi.shape[0]
        assert tuple(phi.shape) == (N, N), phi.shape
        for t in (u, v):
            assert t is None or tuple(t.shape) == (N, N), t.shape
        check(load().pgmg_gradient_add_grid(self._ptr(phi), N, self._ptr(u), self._ptr(v), N,
                                            float(h), int(order), float(scale), stream),
              "pgmg_gradient_add_grid")

    def vorticity_step(self, psi, w, out, h, dt, nu, vmax=False, stream=None):
        """out = w + dt (nu lap(w) - (psi_y w_x - psi_x w_y)) on the interior, w's frame on the
        frame (pgmg_vorticity_grid): N x N float64 device arrays, N = 2^k + 1, k >= 2; h finite
        and not 0; out must not overlap psi or w.  vmax=False: returns out, asynchronous on
        `stream`; vmax=True: returns (out, max |psi_x| + |psi_y| over the interior), synchronous."""
        N = psi.shape[0]
        assert tuple(psi.shape) == (N, N) and tuple(w.shape) == (N, N) and tuple(out.shape) == (N, N)
        m = C.c_double()
        check(load().pgmg_vorticity_grid(self._ptr(psi), self._ptr(w), self._ptr(out), N, float(h),
                                         float(dt), float(nu), C.byref(m) if vmax else None, stream),
              "pgmg_vorticity_grid")
        return (out, m.value) if vmax else out

    def vorticity_stage(self, psi, w, w0, out, h, dt, nu, a, b, vmax=False, stream=None):
        """out = a * w0 + b * e on the interior, e = ops.vorticity_step's value of w under psi, and
        w's frame on the frame: a Runge-Kutta stage in Shu-Osher form (pgmg_vorticity_stage_grid).
        N x N float64 device arrays, N = 2^k + 1, k >= 2; a and b finite; w0 may be w; out must
        overlap none of psi, w and w0.  vmax as in ops.vorticity_step."""
        N = psi.shape[0]
        for t in (psi, w, w0, out):
            assert tuple(t.shape) == (N, N), t.shape
        m = C.c_double()
        check(load().pgmg_vorticity_stage_grid(self._ptr(psi), self._ptr(w), self._ptr(w0),
                                               self._ptr(out), N, float(h), float(dt), float(nu),
                                               float(a), float(b), C.byref(m) if vmax else None,
                                               stream), "pgmg_vorticity_stage_grid")
        return (out, m.value) if vmax else out

    def wall_vorticity(self, psi, w, h, walls=(0.0, 0.0, 0.0, 0.0), free=False, stream=None):
        """The frame of w from psi by Thom's formula, in place (pgmg_wall_vorticity_grid): walls =
        (u on y = 0, u on y = a, v on x = 0, v on x = a); free=True writes +0.0 on the whole frame
        (free slip).  The corners become +0.0.  Asynchronous on `stream`."""
        N = psi.shape[0]
        assert tuple(psi.shape) == (N, N) and tuple(w.shape) == (N, N), (psi.shape, w.shape)
        ws = (C.c_double * 4)(*(float(x) for x in walls))
        check(load().pgmg_wall_vorticity_grid(self._ptr(psi), self._ptr(w), N, float(h),
                                              PGMG_WALL_FREE if free else PGMG_WALL_NOSLIP, ws,
                                              stream), "pgmg_wall_vorticity_grid")
        return w

    def boussinesq_step(self, psi, w, T, w_out, T_out, h, dt, nu, kappa, buoy, vmax=False, stream=None):
        """w_out = w + dt ((nu lap(w) - (psi_y w_x - psi_x w_y)) + (by T_x - bx T_y)) and T_out = T
        + dt (kappa lap(T) - (psi_y T_x - psi_x T_y)) on the interior, the frames of w and T on the
        frames, in one pass (pgmg_boussinesq_grid): N x N float64 device arrays, N = 2^k + 1,
        k >= 2; h finite and not 0; buoy = (bx, by); an output must not overlap an input or the
        other output.  vmax=False: returns (w_out, T_out), asynchronous on `stream`; vmax=True:
        returns (w_out, T_out, max |psi_x| + |psi_y| over the interior), synchronous."""
        N = psi.shape[0]
        for t in (psi, w, T, w_out, T_out):
            assert tuple(t.shape) == (N, N), t.shape
        m = C.c_double()
        b = (C.c_double * 2)(*(float(x) for x in buoy))
        check(load().pgmg_boussinesq_grid(self._ptr(psi), self._ptr(w), self._ptr(T),
                                          self._ptr(w_out), self._ptr(T_out), N, float(h), float(dt),
                                          float(nu), float(kappa), b, C.byref(m) if vmax else None,
                                          stream), "pgmg_boussinesq_grid")
        return (w_out, T_out, m.value) if vmax else (w_out, T_out)

    def boussinesq_stage(self, psi, w, T, w0, T0, w_out, T_out, h, dt, nu, kappa, buoy, a, b,
                         vmax=False, stream=None):
        """w_out = a * w0 + b * ew and T_out = a * T0 + b * et on the interior, ew and et
        ops.boussinesq_step's values of w and T under psi, and the frames of w and T on the frames:
        a Runge-Kutta stage in Shu-Osher form (pgmg_boussinesq_stage_grid).  N x N float64 device
        arrays, N = 2^k + 1, k >= 2; a and b finite; w0 may be w and T0 may be T; an output must
        not overlap an input or the other output.  vmax as in ops.boussinesq_step."""
        N = psi.shape[0]
        for t in (psi, w, T, w0, T0, w_out, T_out):
            assert tuple(t.shape) == (N, N), t.shape
        m = C.c_double()
        bb = (C.c_double * 2)(*(float(x) for x in buoy))
        check(load().pgmg_boussinesq_stage_grid(self._ptr(psi), self._ptr(w), self._ptr(T),
                                                self._ptr(w0), self._ptr(T0), self._ptr(w_out),
                                                self._ptr(T_out), N, float(h), float(dt), float(nu),
                                                float(kappa), bb, float(a), float(b),
                                                C.byref(m) if vmax else None, stream),
              "pgmg_boussinesq_stage_grid")
        return (w_out, T_out, m.value) if vmax else (w_out, T_out)

    def wall_scalar(self, T, adiabatic, stream=None):
        """The adiabatic walls of T by the second-order one-sided dT/dn = 0, in place
        (pgmg_wall_scalar_grid): adiabatic names the walls ("bottom", "top", "left", "right") or is
        a PGMG_TWALL_* mask; the other walls and the four corners keep their values.  Asynchronous
        on `stream`."""
        N = T.shape[0]
        assert tuple(T.shape) == (N, N), T.shape
        check(load().pgmg_wall_scalar_grid(self._ptr(T), N, twall_mask(adiabatic), stream),
              "pgmg_wall_scalar_grid")
        return T

    def release(self, stream=None):
        """Wait for `stream` and free the scratch set the ops keep for it (pgmg_ops_release)."""
        check(load().pgmg_ops_release(stream), "pgmg_ops_release")

    def rhs(self, f, h, a=1.0, p=1.0, q=1.0, stream=None):
        H, W = f.shape
        check(load().pgmg_rhs(self._ptr(f), W, H, float(h), float(a), float(p), float(q),
                              stream), "pgmg_rhs")


ops = _Ops()
