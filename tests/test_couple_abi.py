"""CPU: the C-ABI of heat conduction between neighbouring cells of a pack string
(mpcekf_thermal_couple / _couple_get / _couple_end, mpcekf_step_ex_couple) is declared, exported
and bound at ABI 5; the MPCEKF_TCR_* ids are what the Python layer names; the ctypes prototypes
match the header's parameter lists; a NULL context is an error, not a crash; the Python wrapper
validates its arguments before the library is called; the header spells the rule out."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_thermal_couple", "mpcekf_thermal_couple_get", "mpcekf_thermal_couple_end", "mpcekf_step_ex_couple")
FIELDS = ("NB_SUM", "DT_MAX", "DT_MAX_STEP")
E_ARG = -1


def test_header_declares_enum_and_entry_points():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    m = re.search(r"enum \{\s*MPCEKF_TCR_NB_SUM = 0,(.*?)MPCEKF_NTCR\s*\}", HEADER, re.S)
    assert m, "MPCEKF_TCR_* enum"
    assert ["NB_SUM"] + re.findall(r"MPCEKF_TCR_(\w+)", m.group(1)) == list(FIELDS)
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)
    # the rule is spelled out where the enum is defined: tests/couple_ref.py restates it from there
    doc = HEADER[:HEADER.index("MPCEKF_TCR_NB_SUM = 0")].rsplit("/* ----", 1)[1]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for line in ("r_link[c] is the thermal resistance in K/W between cell c and cell c+1",
                 "only when both cells are in the same string", "+inf means no link", "p = c mod S",
                 "not values already advanced in this launch", "qn = +0.0; nl = 0",
                 "if p > 0 and isfinite(r_link[c-1]): dl = Tl - T; qn = qn + dl / r_link[c-1]; nl += 1",
                 "if p < S - 1 and isfinite(r_link[c]): dr = Tr - T; qn = qn + dr / r_link[c]; nl += 1",
                 "Tn = nl == 0 ? T + ((q - loss) * Ts) / Cth", ": T + (((q - loss) + qn) * Ts) / Cth",
                 "the uncoupled line, bit for bit", "no contraction", "IEEE division",
                 "its neighbours still conduct to and from it", "exact negatives",
                 "the two flows over a link cancel exactly", "only on steps with nl > 0",
                 "the left link is examined first", "replaced only on a strict >",
                 "The stage route does not advance the model"):
        assert re.sub(r"\s+", " ", line) in re.sub(r"\s+", " ", doc), line


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
    # mpcekf_step_ex_aging's list plus cond, before outputs_on_device
    aging = _params("mpcekf_step_ex_aging")
    assert _params("mpcekf_step_ex_couple") == aging[:-1] + ["double*", "int32_t"]
    assert _params("mpcekf_thermal_couple") == ["mpcekf_ctx*", "constdouble*"]
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert M.Context.COUPLE_FIELDS == FIELDS
    for name in ("thermal_couple", "thermal_couple_get", "thermal_couple_end"):
        assert callable(getattr(M.Context, name)), name
    assert list(inspect.signature(M.Context.thermal_couple).parameters) == ["self", "R_link"]
    assert inspect.signature(M.Context.thermal_couple_get).parameters["fields"].default is None


def test_null_arguments_are_errors(P):
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    ids = np.array([0, 2], dtype=np.int32)
    vals = np.zeros((3, 4))
    r = np.ones(4)
    for f, args in ((L.mpcekf_thermal_couple, (None, lib.dptr(r))),
                    (L.mpcekf_thermal_couple_get, (None, 2, lib.iptr(ids), lib.dptr(vals))),
                    (L.mpcekf_thermal_couple_end, (None,)),
                    (L.mpcekf_step_ex_couple, (None, 1, None, None, None, 0, None, None, None, None, None, None, None, 0))):
        assert f(*args) == E_ARG
        assert b"null ctx" in L.mpcekf_last_error()


def test_python_validation_needs_no_device(P):
    """On a Context object with no library context behind it: a touch of the handle would be an
    AttributeError / a crash, not the error asked for."""
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    ctx = M.Context.__new__(M.Context)
    ctx.n, ctx.h, ctx.L, ctx.rom = 6, None, None, P.make_synth_rom()
    with pytest.raises(KeyError, match="unknown thermal row 'flow'"):
        ctx.step(1, thermal=("temp", "flow"))
    with pytest.raises(KeyError, match="DT_MIN"):
        ctx.thermal_couple_get(fields=("NB_SUM", "DT_MIN"))
    with pytest.raises(ValueError, match="scalar or a length-6 array"):
        ctx.thermal_couple(np.ones(5))
    with pytest.raises(ValueError, match="scalar or a length-6 array"):
        ctx.thermal_couple(np.ones((6, 1)))
    for bad in (0.0, -1.0, np.nan, -np.inf, [1, 1, 1, np.nan, 1, 1], [1, 1, 1, 1, 1, 0.0]):
        with pytest.raises(ValueError, match="R_link must be > 0"):
            ctx.thermal_couple(bad)
    r = M.Context._couple_links(6, np.inf)            # +inf: no link, accepted; a scalar is every link
    assert r.shape == (6,) and np.isinf(r).all() and r.dtype == np.float64
    with pytest.raises(ValueError, match="pass pack=dict"):      # before a context is created
        M.runMPC(ctx.rom, np.full(6, 10.0), 25.0, 1, thermal=dict(Cth=1.0, Rth=1.0, Tamb=25.0, ocv=[3, 4], couple=1.0))
    with pytest.raises(ValueError, match="R_link must be > 0"):
        M.run_summary(ctx.rom, np.full(6, 10.0), 25.0, 1, thermal=dict(Cth=1.0, Rth=1.0, Tamb=25.0, ocv=[3, 4], couple=-2.0),
                      pack=dict(series=2))
    ctx.h = None
