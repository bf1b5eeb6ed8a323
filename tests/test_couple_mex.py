"""CPU: the MATLAB gateway's coupling commands ('thermalcouple', 'thermalcoupleget',
'thermalcoupleend', 'stepexcouple') refuse bad arguments with the gateway's error identifier
before they look at the handle, through the MEX API shim (tests/mex)."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
LINKS = np.full((4, 1), 2.0)


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_couple_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, links of the wrong class, an nsteps
    that is no count: all mpcekf:arg, and none dereferences the handle."""
    ok = {"thermalcouple": (LINKS,), "thermalcoupleget": (), "thermalcoupleend": (), "stepexcouple": (2.0,)}
    nout = {"thermalcouple": 0, "thermalcoupleget": 1, "thermalcoupleend": 0, "stepexcouple": 8}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("thermalcouple", "thermalcoupleend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: thermalcoupleget: at most 1 output"):
        shim.mex("thermalcoupleget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepexcouple: at most 8 outputs .*temp, heat, cond"):
        shim.mex("stepexcouple", DEAD, 2.0, nargout=9)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'thermalcouple', h, r_link"):
        shim.mex("thermalcouple", DEAD, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: thermalcouple: r_link: expected ncells real doubles"):
        shim.mex("thermalcouple", DEAD, np.full((4, 1), 2, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: thermalcouple: r_link: expected ncells real doubles"):
        shim.mex("thermalcouple", DEAD, np.full((4, 1), 2 + 1j), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepexcouple', h, nsteps"):
        shim.mex("stepexcouple", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexcouple", DEAD, bad, nargout=0)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
    # the existing thermal step keeps its seven outputs; the cond row has its own command
    assert "[u,v,soc,phise,nexec,temp,heat,cond] = mpcekf_mex('stepexcouple'" in src
