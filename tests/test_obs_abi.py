"""CPU: the obs part of the C-ABI (ABI v5) is declared, exported and bound, and the MATLAB
gateway's 'plantobs' / 'obsslots' commands refuse bad arguments with the gateway's error
identifier before any device call (there is no GPU here)."""
import os
import re

import numpy as np
import pytest

import mexshim
import obs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()
NEW = ("mpcekf_obs_layout", "mpcekf_plant_step_obs", "mpcekf_plant_step_obs_async", "mpcekf_plant_obs_slots",
       "mpcekf_plant_obs_slots_async")


def test_header_declares_entry_points_and_enum():
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", HEADER), s
    m = re.search(r"enum \{\s*MPCEKF_OBS_negSOC = 0,(.*?)MPCEKF_OBS_COUNT\s*\}", HEADER, re.S)
    assert m, "MPCEKF_OBS_* enum"
    names = ["negSOC"] + re.findall(r"MPCEKF_OBS_(\w+)", m.group(1))
    assert tuple(names) == obs_ref.OBS_FIELDS and len(names) == 25
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)


def test_lib_binds_every_new_entry_point(P):
    from importlib import import_module
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    assert lib.ABI_VERSION == 5 == L.mpcekf_abi_version()
    for s in NEW:
        assert s in lib.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert L.mpcekf_plant_step_obs_async.argtypes == L.mpcekf_plant_step_obs.argtypes
    assert L.mpcekf_plant_obs_slots_async.argtypes == L.mpcekf_plant_obs_slots.argtypes
    assert lib.OBS_COUNT == 25 and import_module("mpc-ekf4fastcharge_amd.rom").OBS_FIELDS == obs_ref.OBS_FIELDS
    # OB_step's obs= keyword exists and defaults to the call as it was
    import inspect
    sig = inspect.signature(import_module("mpc-ekf4fastcharge_amd.mpcekf").Context.OB_step)
    assert sig.parameters["obs"].default is False


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)


def test_gateway_obs_commands_check_arguments(shim):
    """Bad handle, a wrong vector length, too many outputs, a slot out of range: all
    mpcekf:arg, none dereferences the handle."""
    for cmd, args in (("plantobs", (np.zeros(4),)), ("obsslots", (np.array([[1.0]]),))):
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args)
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args)
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd)
    with pytest.raises(shim.MexError, match="mpcekf:arg: plantobs: at most 2 outputs"):
        shim.mex("plantobs", DEAD, np.zeros(4), nargout=3)
    with pytest.raises(shim.MexError, match="mpcekf:arg: obsslots: at most 1 output"):
        shim.mex("obsslots", DEAD, np.array([[1.0]]), nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: obsslots: idx: expected at least 1"):   # wrong length
        shim.mex("obsslots", DEAD, np.zeros((0, 0)))
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage"):
        shim.mex("obsslots", DEAD)
    for bad in (0.0, -1.0, 1.5, float("nan"), 3e9):                                           # slot out of range
        with pytest.raises(shim.MexError, match="mpcekf:arg: obsslots: idx.* is not a slot"):
            shim.mex("obsslots", DEAD, np.array([[1.0, bad]]))
    with pytest.raises(shim.MexError, match="mpcekf:arg: idx: expected 2 real doubles"):
        shim.mex("obsslots", DEAD, np.array([[1, 2]], dtype=np.int32))


# the names assigned to ``obs.`` in the reference's OB_step.m:226-228 and 289-356, in order of
# first assignment: what 'plantobs' returns as struct fields
REFERENCE_OBS_FIELDS = [
    "negSOC", "posSOC", "cellSOC",
    "negIfdl", "posIfdl", "negIfdl0", "posIfdl3",
    "negIf", "posIf", "negIf0", "posIf3",
    "negIdl", "posIdl",
    "negThetass", "posThetass", "negThetass0", "posThetass3",
    "negPhise", "posPhise", "negPhise0",
    "Phie", "Thetae",
    "negPhis", "posPhis",
    "Vcell",
]


def test_gateway_struct_field_names_are_the_references():
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"obs_names\[MPCEKF_OBS_COUNT\] = \{(.*?)\};", src, re.S)
    assert m, "plantobs field name table"
    assert re.findall(r'"(\w+)"', m.group(1)) == REFERENCE_OBS_FIELDS == list(obs_ref.OBS_FIELDS)
    # the drop-in fills the same names when initCfg.obsFields asks for them
    drop = open(os.path.join(ROOT, "matlab", "dropin", "OB_step.m")).read()
    assert "obsFields" in drop and "'plantobs'" in drop and "'obsslots'" in drop
