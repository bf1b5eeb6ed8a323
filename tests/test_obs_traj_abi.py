"""CPU: the fused loop's obs trajectory is declared, exported and bound (mpcekf_step_ex_obs,
still ABI v5), Context.step / runMPC take obs=None, and the MATLAB gateway's 'stepobs'
refuses bad arguments with the gateway's error identifier before it looks at the handle
(there is no GPU here)."""
import inspect
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpcekf.h")).read()


def test_header_declares_step_ex_obs():
    m = re.search(r"\bint mpcekf_step_ex_obs\s*\((.*?)\);", HEADER, re.S)
    assert m, "mpcekf_step_ex_obs"
    args = " ".join(m.group(1).split())
    assert args == ("mpcekf_ctx *ctx, int32_t nsteps, const double *tc_degC, const mpcekf_traj *traj, "
                    "const int32_t *slots, int32_t nslots, double *obs, int32_t outputs_on_device")
    assert re.search(r"#define MPCEKF_ABI_VERSION 5\b", HEADER)          # additive: the version stays
    assert re.search(r"\bint mpcekf_step_ex\s*\(", HEADER)


def test_lib_binds_step_ex_obs(P):
    import ctypes as C
    from importlib import import_module
    lib = import_module("mpc-ekf4fastcharge_amd._lib")
    L = lib.load()
    assert lib.ABI_VERSION == 5 == L.mpcekf_abi_version()
    assert "mpcekf_step_ex_obs" in lib.EXPORTS and hasattr(L, "mpcekf_step_ex_obs")
    at = L.mpcekf_step_ex_obs.argtypes
    assert at is not None and len(at) == 8
    assert at[:4] == L.mpcekf_step_ex.argtypes[:4] and at[7] == L.mpcekf_step_ex.argtypes[4]
    assert at[4] == C.POINTER(C.c_int32) and at[5] == C.c_int32
    assert L.mpcekf_step_ex_obs.restype == C.c_int
    # a null context is refused by the shared implementation, as mpcekf_step_ex refuses it
    assert L.mpcekf_step_ex_obs(None, 1, None, None, None, 0, None, 0) == L.mpcekf_step_ex(None, 1, None, None, 0) == -1


def test_python_signatures_default_to_the_call_as_it_was(P):
    from importlib import import_module
    M = import_module("mpc-ekf4fastcharge_amd.mpcekf")
    assert inspect.signature(M.Context.step).parameters["obs"].default is None
    assert inspect.signature(M.runMPC).parameters["obs"].default is None
    sd = inspect.signature(M.Context.step_device).parameters
    assert sd["obs"].default == 0 and tuple(sd["obs_slots"].default) == ()
    # the parameters that were there keep their places and defaults
    assert list(inspect.signature(M.Context.step).parameters)[:4] == ["self", "nsteps", "outputs", "tc"]
    assert list(sd)[:7] == ["self", "nsteps", "u", "v", "soc", "phise", "nexec"]


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
IDX = np.array([[1.0, 20.0]])


def test_gateway_stepobs_checks_arguments(shim):
    """A dead handle, a non-handle, a missing or empty idx, slot indices that are no 1-based
    integers, too many outputs: all mpcekf:arg, none dereferences the handle."""
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
        shim.mex("stepobs", DEAD, 2.0, IDX, nargout=6)
    with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
        shim.mex("stepobs", 1.0, 2.0, IDX, nargout=6)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepobs: missing handle"):
        shim.mex("stepobs")
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepobs', h, nsteps, idx"):   # missing idx
        shim.mex("stepobs", DEAD, 2.0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepobs: idx: expected at least 1"):    # empty idx
        shim.mex("stepobs", DEAD, 2.0, np.zeros((0, 0)))
    for bad in (1.5, 0.0, -1.0, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: stepobs: idx.* is not a slot"):
            shim.mex("stepobs", DEAD, 2.0, np.array([[1.0, bad]]))
    with pytest.raises(shim.MexError, match="mpcekf:arg: idx: expected 2 real doubles"):
        shim.mex("stepobs", DEAD, 2.0, np.array([[1, 2]], dtype=np.int32))
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepobs: at most 6 outputs"):
        shim.mex("stepobs", DEAD, 2.0, IDX, nargout=7)


def test_gateway_and_dropin_name_the_command():
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    assert m and '"stepobs"' in m.group(1)
    assert "mpcekf_step_ex_obs(" in src
    drop = open(os.path.join(ROOT, "matlab", "dropin", "mpcekf_session.m")).read()
    assert "obsFields" in drop and "'stepobs'" in drop
