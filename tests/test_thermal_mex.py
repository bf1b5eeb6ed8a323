"""CPU: the MATLAB gateway's thermal commands ('thermalbegin', 'thermalget', 'thermalend',
'stepthermal') refuse bad arguments with the gateway's error identifier before they look at the
handle, through the MEX API shim (tests/mex)."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
PAR = np.array([[50.0, 3.0, 25.0]] * 4)
OCV = np.linspace(3.0, 4.2, 11)


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_thermal_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, parameters / table / t0 of the wrong
    class, a table of fewer than 2 entries, an nsteps that is no count: all mpcekf:arg, and none
    dereferences the handle."""
    ok = {"thermalbegin": (PAR, OCV), "thermalget": (), "thermalend": (), "stepthermal": (2.0,)}
    nout = {"thermalbegin": 0, "thermalget": 1, "thermalend": 0, "stepthermal": 7}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("thermalbegin", "thermalend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: thermalget: at most 1 output"):
        shim.mex("thermalget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepthermal: at most 7 outputs"):
        shim.mex("stepthermal", DEAD, 2.0, nargout=8)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'thermalbegin', h, params, ocv"):
        shim.mex("thermalbegin", DEAD, PAR, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: thermalbegin: params: expected a real double ncells x 3"):
        shim.mex("thermalbegin", DEAD, PAR.astype(np.int32), OCV, nargout=0)
    for bad in (OCV.astype(np.float32), OCV[:1].copy(), np.zeros((0, 0))):
        with pytest.raises(shim.MexError, match="mpcekf:arg: thermalbegin: ocv: expected 2 or more real doubles"):
            shim.mex("thermalbegin", DEAD, PAR, bad, nargout=0)
    with pytest.raises(shim.MexError, match=r"mpcekf:arg: thermalbegin: t0: expected \[\] or ncells real doubles"):
        shim.mex("thermalbegin", DEAD, PAR, OCV, np.full((1, 4), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for t0 passes the checks
        shim.mex("thermalbegin", DEAD, PAR, OCV, np.zeros((0, 0)), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepthermal', h, nsteps"):
        shim.mex("stepthermal", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepthermal", DEAD, bad, nargout=0)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
