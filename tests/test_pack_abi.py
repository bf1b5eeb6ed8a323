"""CPU: the series strings' part of the C-ABI (mpcekf_pack_begin / _get / _end,
mpcekf_step_ex_pack) is declared, exported and bound at ABI 5; the MPCEKF_PK_* ids are what the
Python layer names; the ctypes prototypes match the header's parameter lists; a NULL context is
an error, not a crash; the Python wrapper validates its arguments before the library is called;
the header spells the rule out."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_pack_begin", "mpcekf_pack_get", "mpcekf_pack_end", "mpcekf_step_ex_pack")
FIELDS = ("nlim", "steps", "headroom")
E_ARG = -1


def test_header_declares_enum_and_entry_points():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    m = re.search(r"enum \{\s*MPCEKF_PK_NLIM = 0,(.*?)MPCEKF_NPK\s*\}", HEADER, re.S)
    assert m, "MPCEKF_PK_* enum"
    assert ["NLIM"] + re.findall(r"MPCEKF_PK_(\w+)", m.group(1)) == [f.upper() for f in FIELDS]
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)
    # the rule is spelled out where the enum is defined: tests/pack_ref.py restates it from there
    doc = HEADER[:HEADER.index("MPCEKF_PK_NLIM = 0")].rsplit("/* ----", 1)[1]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for line in ("String g is the cells [g*S, (g+1)*S)", "largest u_c among the cells whose u_c is not NaN",
                 "-0.0 == +0.0", "Ties go to the lowest in-string index", "bit for bit", "s.uk_1 is not touched",
                 "Its limiter is -1", "one rounded subtraction and one rounded addition per step",
                 "Only finite terms are added", "S = 1 is the identity", "initMPC.m:66-67",
                 "The stage route (mpcekf_mpc_step(_ex)) is not coupled"):
        assert line in doc, line


def _params(name):
    """The C parameter list of `name` in the header, one type string per parameter."""
    m = re.search(rf"\bint {name}\s*\((.*?)\);", HEADER, re.S)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\w+$", "", p.replace("*", " * ")).replace(" ", ""))   # drop the parameter's name
    return out


def test_lib_exports_and_binds_as_the_header_declares(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    assert lib.ABI_VERSION == 5 == L.mpcekf_abi_version()
    assert lib.PACK_FIELDS == FIELDS
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    # header type -> the ctypes the binding may use for it (output rows may be host or device: void *)
    ok = {"mpcekf_ctx*": (C.c_void_p,), "int32_t": (C.c_int32,), "constint32_t*": (ip,), "double*": (dp, C.c_void_p),
          "constdouble*": (dp, C.c_void_p), "int32_t*": (ip, C.c_void_p), "constmpcekf_traj*": (C.POINTER(lib.Traj),)}
    for s in NEW:
        assert s in lib.EXPORTS and hasattr(L, s), s
        f = getattr(L, s)
        assert f.restype is C.c_int, s
        want = _params(s)
        assert len(f.argtypes) == len(want), (s, want)
        for i, (a, w) in enumerate(zip(f.argtypes, want)):
            assert a in ok[w], (s, i, w, a)
    assert _params("mpcekf_step_ex_pack") == ["mpcekf_ctx*", "int32_t", "constdouble*", "constmpcekf_traj*",
                                              "constint32_t*", "int32_t", "double*", "double*", "double*", "double*",
                                              "int32_t*", "int32_t"]
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert M.Context.PACK_FIELDS == FIELDS
    for name in ("pack_begin", "pack_get", "pack_end"):
        assert callable(getattr(M.Context, name)), name
    assert list(inspect.signature(M.Context.pack_begin).parameters) == ["self", "series"]
    for f in (M.Context.step, M.runMPC, M.run_summary):
        assert inspect.signature(f).parameters["pack"].default is None


def test_null_arguments_are_errors(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    ids = np.array([0, 2], dtype=np.int32)
    vals = np.zeros((3, 4))
    for f, args in ((L.mpcekf_pack_begin, (None, 2)),
                    (L.mpcekf_pack_get, (None, 2, lib.iptr(ids), lib.dptr(vals))),
                    (L.mpcekf_pack_end, (None,)),
                    (L.mpcekf_step_ex_pack, (None, 1, None, None, None, 0, None, None, None, None, None, 0))):
        assert f(*args) == E_ARG
        assert b"null ctx" in L.mpcekf_last_error()


def test_python_validation_needs_no_device(P):
    """On a Context object with no library context behind it: a touch of the handle would be an
    AttributeError / a crash, not the KeyError asked for."""
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    ctx = M.Context.__new__(M.Context)
    ctx.n, ctx.h, ctx.L, ctx.rom = 6, None, None, P.make_synth_rom()
    with pytest.raises(KeyError, match="unknown pack row 'u'"):
        ctx.step(1, pack=("ucmd", "u"))
    with pytest.raises(KeyError, match="margin"):
        ctx.pack_get(fields=("nlim", "margin"))
    ctx.h = None
