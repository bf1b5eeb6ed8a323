"""CPU: the limit map's part of the C-ABI (mpcekf_limit_map / _get / _end, mpcekf_step_ex_map) is
declared, exported and bound at ABI 5; a NULL context is an error, not a crash; the header spells
the rule out; the Python wrapper shapes its tables and refuses bad ones before the library is
called.  The refusals that need a live context are in tests/test_gpu_limit_map.py."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_limit_map", "mpcekf_limit_map_get", "mpcekf_limit_map_end", "mpcekf_step_ex_map")
FIELDS = ("Crate", "u_max", "du_min", "du_max", "v_max", "phise_min")
E_ARG = -1


def test_header_declares_and_spells_the_rule_out():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)
    doc = HEADER[HEADER.index("mapped over the SOC estimate"):HEADER.index("int mpcekf_step_ex_map(")]
    for line in ("xz = (z - z_lo) / (z_hi - z_lo)", "sz = xzc * (double)(nz - 1)", "jz = min((int)sz, nz - 2)",
                 "fz = interp_z ? 0.0 : sz - (double)jz", "a   = tab[jt][jz]   + fz * (tab[jt][jz+1]   - tab[jt][jz])",
                 "b   = tab[jt+1][jz] + fz * (tab[jt+1][jz+1] - tab[jt+1][jz])", "val = a + ft * (b - a)",
                 "u_min = -Q * val", "[nsets][nfields][nt][nz]", "soc row", "previous fused step", "one-step lag",
                 "temp[t]", "mpcekf_thermal_schedule's lookup bit for bit", "exclude each other",
                 "mpcekf_clear_limits returns MPCEKF_E_STATE", "mpcekf_thermal_end ends a map that has nt >= 2",
                 "stage route", "lim [nsteps][nfields][ncells]"):
        assert line in doc, line
    assert re.search(r"MPCEKF_LM_Z_LAST = 0,.*?MPCEKF_LM_NEVAL,.*?MPCEKF_LM_NCLAMP_Z,.*?MPCEKF_LM_NCLAMP_T,.*?MPCEKF_NLM",
                     HEADER, re.S)


def test_lib_exports_and_binds(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    assert lib.ABI_VERSION == 5 == L.mpcekf_abi_version()
    for s in NEW:
        assert s in lib.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int, s
    assert len(L.mpcekf_limit_map.argtypes) == 14
    assert len(L.mpcekf_step_ex_map.argtypes) == len(L.mpcekf_step_ex_charger.argtypes) + 1
    assert lib.LIMIT_MAP_FIELDS == ("z_last", "neval", "nclamp_z", "nclamp_t")
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert list(inspect.signature(M.Context.limit_map).parameters) == ["self", "z_lo", "z_hi", "T_lo", "T_hi", "sets",
                                                                       "interp_z", "z0", "tables"]
    assert inspect.signature(M.Context.limit_map).parameters["tables"].kind is inspect.Parameter.VAR_KEYWORD
    assert callable(M.Context.limit_map_get) and callable(M.Context.limit_map_end) and callable(M.mscc_map)
    assert "limit_map" in inspect.signature(M.Context.step).parameters
    for g in (M.runMPC, M.run_summary):
        assert "limit_map" in inspect.signature(g).parameters and "limit_map" in g.__doc__


def test_null_context_is_an_error(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    ids = np.array([1, 6], dtype=np.int32)
    tab = np.ones((1, 2, 2, 3))
    assert L.mpcekf_limit_map(None, 2, lib.iptr(ids), 3, 0.0, 1.0, 2, 20.0, 40.0, 0, 1, lib.dptr(tab), None, None) == E_ARG
    assert b"null ctx" in L.mpcekf_last_error()
    vals = np.zeros((1, 1))
    assert L.mpcekf_limit_map_get(None, 1, lib.iptr(ids[:1]), lib.dptr(vals)) == E_ARG
    assert b"null ctx" in L.mpcekf_last_error()
    assert L.mpcekf_limit_map_end(None) == E_ARG
    assert b"null ctx" in L.mpcekf_last_error()
    assert L.mpcekf_step_ex_map(None, 1, None, None, None, 0, *([None] * 11), 0) == E_ARG
    assert b"null ctx" in L.mpcekf_last_error()


def test_wrapper_shapes_its_tables(P):
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    f = M.Context._map_arrays
    ids, tab, soc, hold, z0 = f(4, None, "hold", None, dict(Crate=[2.0, 1.0, 0.5]))
    assert ids.dtype == np.int32 and ids.tolist() == [1] and soc is None and hold == 1 and z0 is None
    assert tab.shape == (1, 1, 1, 3) and tab.dtype == np.float64 and tab.flags.c_contiguous
    # [nsets][nt][nz] beside [nt][nz] and [nz]: smaller tables serve every set and temperature;
    # the layout is [nsets][nfields][nt][nz]
    three = np.arange(12.0).reshape(2, 2, 3)
    ids, tab, soc, hold, z0 = f(4, np.array([0, 1, 1, 0]), "linear", 0.25,
                                dict(phise_min=[0.1, 0.09, 0.08], Crate=three, v_max=three[0] + 2.0))
    assert ids.tolist() == [6, 1, 5] and tab.shape == (2, 3, 2, 3) and tab.flags.c_contiguous and hold == 0
    assert all(tab[s, 0, t].tolist() == [0.1, 0.09, 0.08] for s in range(2) for t in range(2))
    assert np.array_equal(tab[:, 1], three) and np.array_equal(tab[0, 2], three[0] + 2.0) and np.array_equal(tab[1, 2], tab[0, 2])
    assert soc.dtype == np.int32 and soc.tolist() == [0, 1, 1, 0] and z0.tolist() == [0.25] * 4
    for kw, msg in ((dict(), "no field given"), (dict(Crate_=[1, 2]), "field 'Crate_' cannot be mapped"),
                    (dict(target_soc=[90, 80]), "field 'target_soc' cannot be mapped"),
                    (dict(z_max=[0.9, 0.8]), "field 'z_max' cannot be mapped"),
                    (dict(Crate=2.0), r"Crate must be a \[nz\], \[nt\]\[nz\] or \[nsets\]\[nt\]\[nz\] table, got shape \(\)"),
                    (dict(Crate=np.zeros((2, 2, 2, 2))), r"Crate must be a \[nz\]"),
                    (dict(Crate=[2.0, 1.0], v_max=[4.1, 4.0, 3.9]), r"v_max has shape \(3,\)"),
                    (dict(Crate=three, v_max=np.ones((3, 3))), r"v_max has shape \(3, 3\)")):
        with pytest.raises(ValueError, match="limit_map: " + msg):
            f(4, None, "linear", None, kw)
    for bad in (np.zeros(3, dtype=int), np.zeros((4, 1), dtype=int), np.zeros(4)):
        with pytest.raises(ValueError, match="limit_map: sets must be a length-4 integer array"):
            f(4, bad, "linear", None, dict(Crate=three))
    with pytest.raises(ValueError, match="limit_map: interp_z = 'cubic'"):
        f(4, None, "cubic", None, dict(Crate=three))
    with pytest.raises(ValueError, match="limit_map: z0 must be a scalar or a length-4 array"):
        f(4, None, "hold", np.zeros(3), dict(Crate=three))
    # on a Context object with no library context behind it: refused before the handle is touched
    ctx = M.Context.__new__(M.Context)
    ctx.n, ctx.h, ctx.L = 4, None, None
    with pytest.raises(ValueError, match="cannot be mapped"):
        ctx.limit_map(0.0, 1.0, z_tol=[0.9, 0.8])
    with pytest.raises(ValueError, match="need T_lo and T_hi"):
        ctx.limit_map(0.0, 1.0, Crate=three)
    with pytest.raises(KeyError, match="unknown limit_map row 'val'"):
        ctx.step(1, limit_map=("val",))
    with pytest.raises(KeyError, match="limit_map_get: unknown field 'z'"):
        ctx.limit_map_get("z")
    ctx.h = None
