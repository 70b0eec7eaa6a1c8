"""CPU: pgmg_fmg_bc is part of the C ABI -- declared in include/pgmg.h, exported by the library
and bound with its signature (tests/test_capi.py enumerates the header; this names the entry)."""
import ctypes as C

from test_capi import declared_symbols


def test_fmg_bc_is_declared_exported_and_bound(pgmg):
    from importlib import import_module
    assert "pgmg_fmg_bc" in declared_symbols()
    lib = pgmg.load()
    assert hasattr(lib, "pgmg_fmg_bc")
    sig = {n: (r, a) for n, r, a in import_module("pgmg_amd._capi").SIGNATURES}
    res, args = sig["pgmg_fmg_bc"]
    assert res is C.c_int and args[1:] == [C.c_int, C.c_double], (res, args)
    # a null context is refused by the argument check, before anything touches a device
    assert lib.pgmg_fmg_bc(None, 2, 0.0) == pgmg.PGMG_ERR_ARG


def test_python_boundary_defaults_to_zero(pgmg):
    import inspect
    assert inspect.signature(pgmg.Solver.fmg).parameters["boundary"].default == "zero"
    assert inspect.signature(pgmg.Solver.solve).parameters["boundary"].default == "zero"
