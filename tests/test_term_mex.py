"""CPU: the MATLAB gateway's termination commands ('termbegin', 'termget', 'termend',
'stepuntil') refuse bad arguments with the gateway's error identifier before they look at the
handle, through the MEX API shim (tests/mex); the drop-in session names an op for each."""
import os
import re

import numpy as np
import pytest

import mexshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = np.array([[0xDEADBEEF]], dtype=np.uint64)
PAR = np.full((4, 3), np.nan)


@pytest.fixture(scope="module")
def shim():
    mexshim.build()
    return mexshim


def test_gateway_term_commands_check_arguments(shim):
    """Bad handle, missing handle, outputs that do not exist, a hold or chunk that is no positive
    integer, a max_steps that is no count, params or a tc of the wrong class: all mpcekf:arg, and
    none dereferences the handle."""
    ok = {"termbegin": (PAR, 2.0), "termget": (), "termend": (), "stepuntil": (40.0, 8.0)}
    nout = {"termbegin": 0, "termget": 1, "termend": 0, "stepuntil": 2}
    for cmd, args in ok.items():
        with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):
            shim.mex(cmd, DEAD, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match="mpcekf:arg: expected a uint64 handle"):
            shim.mex(cmd, 1.0, *args, nargout=nout[cmd])
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: missing handle"):
            shim.mex(cmd, nargout=nout[cmd])
    for cmd in ("termbegin", "termend"):
        with pytest.raises(shim.MexError, match=f"mpcekf:arg: {cmd}: no output"):
            shim.mex(cmd, DEAD, *ok[cmd], nargout=1)
    with pytest.raises(shim.MexError, match="mpcekf:arg: termget: at most 1 output"):
        shim.mex("termget", DEAD, nargout=2)
    with pytest.raises(shim.MexError, match="mpcekf:arg: stepuntil: at most 2 outputs"):
        shim.mex("stepuntil", DEAD, 40.0, 8.0, nargout=3)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'termbegin', h, params, hold"):
        shim.mex("termbegin", DEAD, PAR, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: termbegin: params: expected ncells x 3 real doubles"):
        shim.mex("termbegin", DEAD, np.zeros((4, 3), dtype=np.int32), 1.0, nargout=0)
    for bad in (0.0, -4.0, 2.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: termbegin: hold = .* is not a positive integer"):
            shim.mex("termbegin", DEAD, PAR, bad, nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # an int32 scalar passes
        shim.mex("termbegin", DEAD, PAR, np.array([[3]], dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: usage: .*'stepuntil', h, max_steps, chunk"):
        shim.mex("stepuntil", DEAD, 40.0, nargout=0)
    for bad in (-1.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: max_steps: expected a non-negative integer"):
            shim.mex("stepuntil", DEAD, bad, 8.0, nargout=0)
    for bad in (0.0, -8.0, 1.5, float("nan"), 3e9):
        with pytest.raises(shim.MexError, match="mpcekf:arg: stepuntil: chunk = .* is not a positive integer"):
            shim.mex("stepuntil", DEAD, 40.0, bad, nargout=0)
    with pytest.raises(shim.MexError, match=r"mpcekf:arg: stepuntil: tc: expected \[\] or ncells real doubles"):
        shim.mex("stepuntil", DEAD, 40.0, 8.0, np.full((4, 1), 25, dtype=np.int32), nargout=0)
    with pytest.raises(shim.MexError, match="mpcekf:arg: not a live mpcekf context"):     # [] for tc passes the checks
        shim.mex("stepuntil", DEAD, 0.0, 1.0, np.zeros((0, 0)), nargout=2)
    src = open(os.path.join(ROOT, "matlab", "mpcekf_mex.c")).read()
    m = re.search(r"with_handle\[\] = \{(.*?)\};", src, re.S)
    for cmd in ok:
        assert m and f'"{cmd}"' in m.group(1), cmd
    for call in ("mpcekf_term_begin(h,", "mpcekf_term_get(h,", "mpcekf_term_end(h)", "mpcekf_step_until(h,"):
        assert call in src, call


def test_session_has_an_op_for_each_command():
    src = open(os.path.join(ROOT, "matlab", "dropin", "mpcekf_session.m")).read()
    for cmd in ("termbegin", "termget", "termend", "stepuntil"):
        assert f"case '{cmd}'" in src and f"mpcekf_mex('{cmd}', P.h" in src, cmd
