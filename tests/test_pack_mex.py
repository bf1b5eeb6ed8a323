"""CPU: the MATLAB gateway's pack commands ('packbegin', 'packget', 'packend', 'stepexpack')
refuse bad arguments with the gateway's error identifier before they look at the handle, through
the MEX API shim (tests/mex)."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_pack_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, a series that is no positive
    integer, an nsteps that is no count, a tc of the wrong class: all mpcekf:arg, and none
    dereferences the handle."""
    ok = {"packbegin": (96.0,), "packget": (), "packend": (), "stepexpack": (2.0,)}
    nout = {"packbegin": 0, "packget": 1, "packend": 0, "stepexpack": 7}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("packbegin", "packend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: packget: at most 1 output"):
        shim.mex("packget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepexpack: at most 7 outputs"):
        shim.mex("stepexpack", DEAD, 2.0, nargout=8)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'packbegin', h, series"):
        shim.mex("packbegin", DEAD, nargout=0)
    for bad in (0.0, -4.0, 2.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: packbegin: series = .* is not a positive integer"):
            shim.mex("packbegin", DEAD, bad, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # an int32 scalar passes
        shim.mex("packbegin", DEAD, np.array([[4]], dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepexpack', h, nsteps"):
        shim.mex("stepexpack", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexpack", DEAD, bad, nargout=0)
    with pytest.raises(shim.MexError, match=r"mpcekf:arg: stepexpack: tc: expected \[\] or ncells x nsteps real doubles"):
        shim.mex("stepexpack", DEAD, 2.0, np.full((4, 2), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for tc passes the checks
        shim.mex("stepexpack", DEAD, 2.0, np.zeros((0, 0)), nargout=0)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
