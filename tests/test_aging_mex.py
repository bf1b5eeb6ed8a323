"""CPU: the MATLAB gateway's aging commands ('agingbegin', 'agingget', 'agingend',
'stepexaging') refuse bad arguments with the gateway's error identifier before they look at the
handle, through the MEX API shim (tests/mex)."""
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


def test_gateway_aging_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, params of the wrong shape or class,
    sources outside 1..3, a source or reaction that is no index, an nsteps that is no count, a tc
    of the wrong class: all mpcekf:arg, and none dereferences the handle."""
    par = np.zeros((4, 10))
    ok = {"agingbegin": (par, 1.0), "agingget": (1.0, 1.0), "agingend": (), "stepexaging": (2.0,)}
    nout = {"agingbegin": 0, "agingget": 1, "agingend": 0, "stepexaging": 6}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("agingbegin", "agingend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: agingget: at most 1 output"):
        shim.mex("agingget", DEAD, 1.0, 1.0, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepexaging: at most 6 outputs"):
        shim.mex("stepexaging", DEAD, 2.0, nargout=7)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'agingbegin', h, params, sources"):
        shim.mex("agingbegin", DEAD, par, nargout=0)
    for bad in (np.zeros((4, 10), dtype=np.float32), np.zeros((0, 0))):
        with pytest.raises(shim.MexError, match="mpcekf:arg: agingbegin: params: expected a real double"):
            shim.mex("agingbegin", DEAD, bad, 1.0, nargout=0)
    for bad in (np.zeros((4, 7)), np.zeros((4, 25))):
        with pytest.raises(shim.MexError, match="mpcekf:arg: agingbegin: params: 4 x .*5 columns per reaction, 1..4 reactions"):
            shim.mex("agingbegin", DEAD, bad, 1.0, nargout=0)
    for bad in (0.0, 4.0, 1.5, float("nan")):
        with pytest.raises(shim.MexError, match="mpcekf:arg: agingbegin: sources = .* is not 1 .est., 2 .plant. or 3 .both."):
            shim.mex("agingbegin", DEAD, par, bad, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'agingget', h, source, react"):
        shim.mex("agingget", DEAD, 1.0, nargout=1)
    for bad in (0.0, 3.0, 1.5):
        with pytest.raises(shim.MexError, match="mpcekf:arg: agingget: source = .* is not 1 .est. or 2 .plant."):
            shim.mex("agingget", DEAD, bad, 1.0, nargout=1)
    for bad in (0.0, 5.0, 1.5, float("nan")):
        with pytest.raises(shim.MexError, match="mpcekf:arg: agingget: react = .* is not a reaction 1..4"):
            shim.mex("agingget", DEAD, 2.0, bad, nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepexaging', h, nsteps"):
        shim.mex("stepexaging", DEAD, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: nsteps: expected a non-negative integer"):
            shim.mex("stepexaging", DEAD, bad, nargout=0)
    with pytest.raises(shim.MexError, match=r"mpcekf:arg: stepexaging: tc: expected \[\] or ncells x nsteps real doubles"):
        shim.mex("stepexaging", DEAD, 2.0, np.full((4, 2), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for tc passes the checks
        shim.mex("stepexaging", DEAD, 2.0, np.zeros((0, 0)), nargout=0)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
