"""CPU: the balancer's part of the C-ABI (mpcekf_balance_begin / _get / _end,
mpcekf_step_ex_balance) is declared, exported and bound at ABI 5; the MPCEKF_BL_* / MPCEKF_BLP_*
ids are what the Python layer names; the ctypes prototypes match the header's parameter lists; a
NULL context is an error, not a crash; the Python wrapper validates its arguments before the
library is called; the header spells the rule out."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_balance_begin", "mpcekf_balance_get", "mpcekf_balance_end", "mpcekf_step_ex_balance")
FIELDS = ("steps_on", "q_bleed", "switches", "dz_max", "dz_last", "steps")
PARAMS = ("i_bleed", "dz_on", "dz_off")
E_ARG = -1


def test_header_declares_enums_and_entry_points():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    m = re.search(r"enum \{\s*MPCEKF_BL_STEPS_ON = 0,(.*?)MPCEKF_NBL\s*\}", HEADER, re.S)
    assert m, "MPCEKF_BL_* enum"
    assert ["STEPS_ON"] + re.findall(r"MPCEKF_BL_(\w+)", m.group(1)) == [f.upper() for f in FIELDS]
    m = re.search(r"enum \{\s*MPCEKF_BLP_I_BLEED = 0,(.*?)MPCEKF_NBLP\s*\}", HEADER, re.S)
    assert m and ["I_BLEED"] + re.findall(r"MPCEKF_BLP_(\w+)", m.group(1)) == [p.upper() for p in PARAMS]
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)
    # the pack's three fields stand as they were
    assert re.search(r"enum \{ MPCEKF_PK_NLIM = 0, MPCEKF_PK_STEPS, MPCEKF_PK_HEADROOM, MPCEKF_NPK \}", HEADER)
    # the rule is spelled out where the enums are defined: tests/balance_ref.py restates it from there
    doc = HEADER[:HEADER.index("MPCEKF_BLP_I_BLEED = 0")].rsplit("/* ----", 1)[1]
    doc = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", doc))
    for line in ("A cell is valid when neither u_c nor z_c is NaN",
                 "on a tie the lowest in-string index wins, and zmin_g is that cell's z_c bit for bit",
                 "If the string has no valid cell, zmin_g is NaN",
                 "d = z_c - zmin_g, one rounded subtraction",
                 "if d >= dz_on: on = 1 else if d <= dz_off: on = 0 else: on keeps its value",
                 "For a cell that is not valid, on = 0",
                 "The cell is bleeding when on && i_bleed_c > 0",
                 "b_c = i_bleed_c when bleeding, else +0.0",
                 "e_c = u_c - b_c (one rounded subtraction) when compensate && bleeding && u_c < 0",
                 "Otherwise e_c = u_c bit for bit",
                 "m_g = e_lim, bit for bit",
                 "a_c = m_g + b_c (one rounded addition) for a bleeding cell",
                 "HEADROOM += m_g - e_c",
                 "It starts at 0, is reset by begin and persists across calls",
                 "i_bleed = 0 everywhere leaves every bit of the same pack context without a balancer",
                 "A dz_on that no cell reaches leaves every bit too",
                 "S = 1 is the identity, because d = 0 < dz_on",
                 "Not modelled: a voltage-based criterion, a bleed current that depends on the cell voltage (v / R), "
                 "the bleeder's own heat in the thermal model, active (charge-shuttling) balancing, the stage route"):
        assert line in doc, line
    assert "balancing or bypass currents" not in HEADER       # the pack section no longer lists it as open


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
    assert lib.BALANCE_FIELDS == FIELDS and lib.BALANCE_PARAMS == PARAMS
    assert lib.PACK_FIELDS == ("nlim", "steps", "headroom")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ok = {"mpcekf_ctx*": (C.c_void_p,), "int32_t": (C.c_int32,), "constint32_t*": (ip, C.c_void_p),
          "double*": (dp, C.c_void_p), "constdouble*": (dp, C.c_void_p), "int32_t*": (ip, C.c_void_p),
          "constmpcekf_traj*": (C.POINTER(lib.Traj),)}
    for s in NEW:
        assert s in lib.EXPORTS and hasattr(L, s), s
        f = getattr(L, s)
        assert f.restype is C.c_int, s
        want = _params(s)
        assert len(f.argtypes) == len(want), (s, want)
        for i, (a, w) in enumerate(zip(f.argtypes, want)):
            assert a in ok[w], (s, i, w, a)
    assert _params("mpcekf_balance_begin") == ["mpcekf_ctx*", "constdouble*", "int32_t"]
    # mpcekf_step_ex_pack's parameter list plus the two rows
    pk, bl = _params("mpcekf_step_ex_pack"), _params("mpcekf_step_ex_balance")
    assert bl == pk[:-1] + ["double*", "double*"] + pk[-1:]
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert M.Context.BALANCE_FIELDS == FIELDS and M.Context.BALANCE_PARAMS == PARAMS
    for name in ("balance_begin", "balance_get", "balance_end"):
        assert callable(getattr(M.Context, name)), name
    sig = inspect.signature(M.Context.balance_begin).parameters
    assert list(sig) == ["self", "i_bleed", "dz_on", "dz_off", "compensate"]
    assert sig["dz_off"].default is None and sig["compensate"].default is True


def test_null_and_range_arguments_are_errors(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    ids = np.array([0, 2], dtype=np.int32)
    vals = np.full((3, 4), 7.0)
    tr = lib.Traj()
    for f, args in ((L.mpcekf_balance_begin, (None, lib.dptr(vals), 1)),
                    (L.mpcekf_balance_get, (None, 2, lib.iptr(ids), lib.dptr(vals))),
                    (L.mpcekf_balance_end, (None,)),
                    (L.mpcekf_step_ex_balance, (None, 3, None, C.byref(tr), None, 0, None, None, None, None, None,
                                                vals.ctypes.data_as(C.c_void_p), None, 0))):
        assert f(*args) == E_ARG
        assert b"null ctx" in L.mpcekf_last_error()
    assert (vals == 7.0).all()                              # a refused call writes nothing


def test_python_validation_needs_no_device(P):
    """On a Context object with no library context behind it: a touch of the handle would be an
    AttributeError / a crash, not the error asked for."""
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    ctx = M.Context.__new__(M.Context)
    ctx.n, ctx.h, ctx.L, ctx.rom = 6, None, None, P.make_synth_rom()
    with pytest.raises(ValueError, match="balance_begin: i_bleed must be a scalar or a length-6 array"):
        ctx.balance_begin(np.zeros(5), 0.01)
    with pytest.raises(ValueError, match="balance_begin: dz_off must be a scalar or a length-6 array"):
        ctx.balance_begin(0.1, 0.01, dz_off=np.zeros((6, 1)))
    for bad in (-0.1, float("nan"), np.r_[np.zeros(5), -1.0]):
        with pytest.raises(ValueError, match="balance_begin: i_bleed: a current >= 0"):
            ctx.balance_begin(bad, 0.01)
    for bad in (0.0, -0.01, float("nan")):
        with pytest.raises(ValueError, match="balance_begin: dz_on: a SOC fraction > 0"):
            ctx.balance_begin(0.1, bad)
    for bad in (-0.001, 0.011, float("nan")):
        with pytest.raises(ValueError, match=r"balance_begin: dz_off: a SOC fraction in \[0, dz_on\]"):
            ctx.balance_begin(0.1, 0.01, dz_off=bad)
    for bad in (2, -1, 0.5, None, "yes"):
        with pytest.raises(ValueError, match="balance_begin: compensate = "):
            ctx.balance_begin(0.1, 0.01, compensate=bad)
    with pytest.raises(KeyError, match="balance_get: unknown field 'on'"):
        ctx.balance_get(fields=("steps", "on"))
    with pytest.raises(KeyError, match="step: unknown pack row 'on'"):
        ctx.step(2, pack=("bleed", "on"))
    with pytest.raises(ValueError, match="step: the balancer's rows"):
        ctx.step(2, pack=("bleed",), aging=("rate",))
    p, comp = M.Context._balance_args(6, 0.1, np.linspace(0.01, 0.02, 6))
    assert p.shape == (3, 6) and (p[0] == 0.1).all() and (p[2] == p[1] / 2).all() and comp == 1    # dz_off = dz_on / 2
    p, comp = M.Context._balance_args(6, np.arange(6.0), 0.01, 0.0, False)
    assert (p[0] == np.arange(6.0)).all() and (p[2] == 0).all() and comp == 0
    # the wrappers check their balance dict before they create a context
    rom = ctx.rom
    soc0 = np.full(6, 30.0)
    with pytest.raises(KeyError, match=r"runMPC: unknown pack\['balance'\] key 'i'"):
        M.runMPC(rom, soc0, 25.0, 4, pack=dict(series=3, balance=dict(i=0.1, dz_on=0.01)))
    with pytest.raises(KeyError, match=r"run_summary: pack\['balance'\] needs 'dz_on'"):
        M.run_summary(rom, soc0, 25.0, 4, pack=dict(series=3, balance=dict(i_bleed=0.1)))
    with pytest.raises(ValueError, match="balance_begin: dz_on"):
        M.runMPC(rom, soc0, 25.0, 4, pack=dict(series=3, balance=dict(i_bleed=0.1, dz_on=0.0)))
